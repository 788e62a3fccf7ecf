/* C-ABI test of the refinement and the mixed-precision solve through
 * libdlaf_c.so, 1x1 grid, n = 48, nb = 16, three right-hand sides.
 *
 * A is the (2,-1) Toeplitz matrix (||A||_inf = 4, kappa_1 = 1200), the
 * solution x_true has small integer entries, so b = A x_true is exact. The
 * upper triangle of the buffers of A and of its factor holds 1e30: nothing
 * may read it.
 *
 * porfs, on the solution of potrs with one entry pushed off by 1e-10:
 *   berr <= 4 eps, and ||x - x_true||_inf / ||x_true||_inf <= ferr <= 1e-10
 *   (the bound is about kappa n eps; the push is gone).
 * sposv: 0 <= iter <= 8, info = 0, and the criterion of its loop,
 *   ||b - A x||_inf <= ||x||_inf ||A||_inf 2^-53 sqrt(n), with the residual in
 *   long double; a and b come back unchanged. An entry of 1e39 gives -2. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dlaf_c.h"

#define N 48
#define NB 16
#define NRHS 3

static int fails = 0;

static void check(const char* what, int ok) {
  printf("%s: %s\n", what, ok ? "ok" : "MISMATCH");
  if (!ok) ++fails;
}

static double entry(int i, int j) {
  return i == j ? 2.0 : (i == j + 1 || j == i + 1) ? -1.0 : 0.0;
}

int main(void) {
  const double eps = 2.220446049250313e-16;
  const int desc[9] = {1, 0, N, N, NB, NB, 0, 0, N};
  const int descb[9] = {1, 0, N, NRHS, NB, NB, 0, 0, N};
  const size_t abytes = (size_t)N * N * sizeof(double);
  const size_t bbytes = (size_t)N * NRHS * sizeof(double);
  double* a = malloc(abytes);
  double* a0 = malloc(abytes);
  double* af = malloc(abytes);
  double* b = malloc(bbytes);
  double* b0 = malloc(bbytes);
  double* x = malloc(bbytes);
  double* xt = malloc(bbytes);
  double ferr[NRHS], berr[NRHS];
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i)
      a[i + (long)j * N] = j > i ? 1e30 : entry(i, j); /* column-major */
  for (int j = 0; j < NRHS; ++j)
    for (int i = 0; i < N; ++i)
      xt[i + (long)j * N] = (double)((i * 7 + j * 3) % 11 - 5);
  for (int j = 0; j < NRHS; ++j)
    for (int i = 0; i < N; ++i) {
      double s = 0.0;
      for (int k = 0; k < N; ++k) s += entry(i, k) * xt[k + (long)j * N];
      b[i + (long)j * N] = s;
    }
  memcpy(a0, a, abytes);
  memcpy(af, a, abytes);
  memcpy(b0, b, bbytes);
  memcpy(x, b, bbytes);

  int info = -1, iter = -99;
  dlaf_pdpotrf('L', N, af, 1, 1, desc, &info);
  check("pdpotrf info", info == 0);
  dlaf_pdpotrs('L', N, NRHS, af, 1, 1, desc, x, 1, 1, descb, &info);
  check("pdpotrs info", info == 0);
  x[N / 2 + (long)1 * N] += 1e-10;
  dlaf_pdporfs('L', N, NRHS, a, 1, 1, desc, af, 1, 1, desc, b, 1, 1, descb, x,
               1, 1, descb, ferr, berr, &info);
  check("pdporfs info", info == 0);
  check("pdporfs reads a", memcmp(a, a0, abytes) == 0);
  check("pdporfs reads b", memcmp(b, b0, bbytes) == 0);
  for (int j = 0; j < NRHS; ++j) {
    double err = 0.0, xmax = 0.0;
    for (int i = 0; i < N; ++i) {
      const double d = fabs(x[i + (long)j * N] - xt[i + (long)j * N]);
      if (d > err) err = d;
      if (fabs(xt[i + (long)j * N]) > xmax) xmax = fabs(xt[i + (long)j * N]);
    }
    printf("column %d: berr = %.3e ferr = %.3e true = %.3e\n", j, berr[j],
           ferr[j], err / xmax);
    check("pdporfs berr <= 4 eps", berr[j] <= 4.0 * eps);
    check("pdporfs true error <= ferr", err / xmax <= ferr[j]);
    check("pdporfs ferr <= 1e-10", ferr[j] <= 1e-10);
  }

  memset(x, 0, bbytes);
  dlaf_pdsposv('L', N, NRHS, a, 1, 1, desc, b, 1, 1, descb, x, 1, 1, descb,
               &iter, &info);
  printf("pdsposv iter = %d info = %d\n", iter, info);
  check("pdsposv iter in [0, 8]", iter >= 0 && iter <= 8);
  check("pdsposv info", info == 0);
  check("pdsposv reads a", memcmp(a, a0, abytes) == 0);
  check("pdsposv reads b", memcmp(b, b0, bbytes) == 0);
  for (int j = 0; j < NRHS; ++j) {
    long double res = 0.0L;
    double xmax = 0.0;
    for (int i = 0; i < N; ++i) {
      long double s = b[i + (long)j * N];
      for (int k = 0; k < N; ++k)
        s -= (long double)entry(i, k) * x[k + (long)j * N];
      if (fabsl(s) > res) res = fabsl(s);
      if (fabs(x[i + (long)j * N]) > xmax) xmax = fabs(x[i + (long)j * N]);
    }
    check("pdsposv criterion",
          res <= (long double)(xmax * 4.0 * (eps / 2.0) * sqrt((double)N)));
  }

  a[(N - 1) + (long)(N - 1) * N] = 1e39;
  dlaf_pdsposv('L', N, NRHS, a, 1, 1, desc, b, 1, 1, descb, x, 1, 1, descb,
               &iter, &info);
  check("pdsposv overflow iter = -2", iter == -2);
  check("pdsposv overflow info", info == 0);

  dlaf_finalize();
  if (fails) {
    printf("%d mismatches\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
