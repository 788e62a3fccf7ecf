/* C-ABI test of the condition estimates and the Cholesky solve through
 * libdlaf_c.so, 1x1 grid, n = 48, nb = 16.
 *
 * The (2,-1) Toeplitz matrix has one-norm 4 and its inverse, with entries
 * min(i,j) (n + 1 - max(i,j)) / (n + 1), one-norm 24 * 25 / 2 = 300: pocon
 * must return 1 / 1200 (the estimator is exact there). The upper triangle of
 * the buffer holds 1e30: potrf 'L' and pocon must not read it.
 *
 * The all-ones lower triangle L has ||L||_1 = 48 and the bidiagonal inverse
 * (1 on the diagonal, -1 below it) with ||L^-1||_1 = 2: rcond = 1 / 96,
 * checked with the estimator band rcond (1 - delta) <= est <= 3 rcond,
 * delta = 100 n eps kappa_1. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "dlaf_c.h"

#define N 48
#define NB 16
#define NRHS 3

static int fails = 0;

static void check(const char* what, int ok) {
  printf("%s: %s\n", what, ok ? "ok" : "MISMATCH");
  if (!ok) ++fails;
}

int main(void) {
  const double eps = 2.220446049250313e-16;
  const int desc[9] = {1, 0, N, N, NB, NB, 0, 0, N};
  const int descb[9] = {1, 0, N, NRHS, NB, NB, 0, 0, N};
  double* a = calloc((size_t)N * N, sizeof(double));
  double* full = calloc((size_t)N * N, sizeof(double));
  double* l = calloc((size_t)N * N, sizeof(double));
  double* b = calloc((size_t)N * NRHS, sizeof(double));
  double* b0 = calloc((size_t)N * NRHS, sizeof(double));
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      long k = i + (long)j * N; /* column-major */
      double v = i == j ? 2.0 : (i == j + 1 || j == i + 1) ? -1.0 : 0.0;
      full[k] = v;
      a[k] = j > i ? 1e30 : v;
      l[k] = j > i ? 1e30 : 1.0;
    }
  for (int j = 0; j < NRHS; ++j)
    for (int i = 0; i < N; ++i)
      b[i + (long)j * N] = b0[i + (long)j * N] = sin(1.0 + i + 7.0 * j);

  int info = -1;
  double rcond = -1.0;
  const double anorm = dlaf_pdlansy('1', 'L', N, a, 1, 1, desc);
  check("pdlansy = 4", anorm == 4.0);
  dlaf_pdpotrf('L', N, a, 1, 1, desc, &info);
  check("pdpotrf info", info == 0);
  dlaf_pdpocon('L', N, a, 1, 1, desc, anorm, &rcond, &info);
  printf("pdpocon rcond = %.17g (want %.17g)\n", rcond, 1.0 / 1200.0);
  check("pdpocon info", info == 0);
  check("pdpocon 1/1200", fabs(rcond * 1200.0 - 1.0) <= 1e-12);

  dlaf_pdpotrs('L', N, NRHS, a, 1, 1, desc, b, 1, 1, descb, &info);
  check("pdpotrs info", info == 0);
  /* ||A x - b||_inf <= 100 n eps (||A||_inf ||x||_inf + ||b||_inf) */
  double res = 0.0, xmax = 0.0, bmax = 0.0;
  for (int j = 0; j < NRHS; ++j)
    for (int i = 0; i < N; ++i) {
      double s = -b0[i + (long)j * N];
      for (int k = 0; k < N; ++k) s += full[i + (long)k * N] * b[k + (long)j * N];
      if (fabs(s) > res) res = fabs(s);
      if (fabs(b[i + (long)j * N]) > xmax) xmax = fabs(b[i + (long)j * N]);
      if (fabs(b0[i + (long)j * N]) > bmax) bmax = fabs(b0[i + (long)j * N]);
    }
  printf("pdpotrs residual = %.3e\n", res);
  check("pdpotrs residual", res <= 100.0 * N * eps * (4.0 * xmax + bmax));

  const double truth = 1.0 / 96.0, delta = 100.0 * N * eps * 96.0;
  const char norms[2] = {'1', 'I'};
  for (int k = 0; k < 2; ++k) {
    dlaf_pdtrcon(norms[k], 'L', 'N', N, l, 1, 1, desc, &rcond, &info);
    printf("pdtrcon %c rcond = %.17g (truth %.17g)\n", norms[k], rcond, truth);
    check("pdtrcon info", info == 0);
    check("pdtrcon band",
          truth * (1.0 - delta) <= rcond && rcond <= 3.0 * truth);
  }

  dlaf_finalize();
  if (fails) {
    printf("%d mismatches\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
