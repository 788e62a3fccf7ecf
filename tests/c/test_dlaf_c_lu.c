/* C-ABI test of the LU entry points through libdlaf_c.so, 1x1 grid, n = 96,
 * nb = 32.
 *
 * A is the (2,-1) Toeplitz matrix with its rows reversed: ||A||_1 = 4, and
 * since a row permutation of a matrix permutes the columns of its inverse,
 * ||A^-1||_1 is the Toeplitz one, n (n + 2) / 8 = 1176: gecon must return
 * 1 / 4704 (the estimator is exact there). Partial pivoting undoes the
 * reversal: ipiv[j] = n - j (1-based) for the first half of the rows. The
 * rows of the Toeplitz matrix sum to 1, 0, ..., 0, 1, so A x = e_1 + e_n has
 * x = 1. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "dlaf_c.h"

#define N 96
#define NB 32

static int fails = 0;

static void check(const char* what, int ok) {
  printf("%s: %s\n", what, ok ? "ok" : "MISMATCH");
  if (!ok) ++fails;
}

static double toeplitz_reversed(int i, int j) {
  const int r = N - 1 - i;
  return r == j ? 2.0 : (r == j + 1 || j == r + 1) ? -1.0 : 0.0;
}

int main(void) {
  const int desc[9] = {1, 0, N, N, NB, NB, 0, 0, N};
  const int descb[9] = {1, 0, N, 1, NB, NB, 0, 0, N};
  double* a = calloc((size_t)N * N, sizeof(double));
  double* a2 = calloc((size_t)N * N, sizeof(double));
  dlaf_complex_z* z = calloc((size_t)N * N, sizeof(dlaf_complex_z));
  double* b = calloc(N, sizeof(double));
  double* b2 = calloc(N, sizeof(double));
  dlaf_complex_z* zb = calloc(N, sizeof(dlaf_complex_z));
  int* ipiv = calloc(N, sizeof(int));
  int* ipiv2 = calloc(N, sizeof(int));
  int* zpiv = calloc(N, sizeof(int));
  double* zr = (double*)z;
  double* zbr = (double*)zb;
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      long k = i + (long)j * N; /* column-major */
      a[k] = a2[k] = toeplitz_reversed(i, j);
      /* i A: the same pivots, the solution of (iA) x = i (e_1 + e_n) is 1 */
      zr[2 * k] = 0.0;
      zr[2 * k + 1] = a[k];
    }
  b[0] = b[N - 1] = b2[0] = b2[N - 1] = 1.0;
  zbr[1] = zbr[2 * (N - 1) + 1] = 1.0;

  int info = -1;
  double rcond = -1.0;
  const double anorm = dlaf_pdlange('1', N, N, a, 1, 1, desc);
  check("pdlange = 4", anorm == 4.0);
  dlaf_pdgetrf(N, N, a, 1, 1, desc, ipiv, &info);
  check("pdgetrf info", info == 0);
  int piv_ok = 1;
  for (int j = 0; j < N / 2; ++j) piv_ok &= ipiv[j] == N - j;
  for (int j = 0; j < N; ++j) piv_ok &= ipiv[j] >= j + 1 && ipiv[j] <= N;
  check("pdgetrf pivots undo the reversal", piv_ok);

  dlaf_pdgecon('1', N, a, 1, 1, desc, anorm, &rcond, &info);
  printf("pdgecon rcond = %.17g (want %.17g)\n", rcond, 1.0 / 4704.0);
  check("pdgecon info", info == 0);
  check("pdgecon 1/4704", fabs(rcond * 4704.0 - 1.0) <= 1e-12);

  dlaf_pdgetrs('N', N, 1, a, 1, 1, desc, ipiv, b, 1, 1, descb, &info);
  check("pdgetrs info", info == 0);
  double err = 0.0;
  for (int i = 0; i < N; ++i) err = fmax(err, fabs(b[i] - 1.0));
  printf("pdgetrs max |x - 1| = %.3e\n", err);
  check("pdgetrs x = 1", err <= 1e-12);

  dlaf_pdgesv(N, 1, a2, 1, 1, desc, ipiv2, b2, 1, 1, descb, &info);
  check("pdgesv info", info == 0);
  int same = 1;
  for (int i = 0; i < N; ++i) same &= b2[i] == b[i] && ipiv2[i] == ipiv[i];
  for (long k = 0; k < (long)N * N; ++k) same &= a2[k] == a[k];
  check("pdgesv = pdgetrf + pdgetrs, bitwise", same);

  dlaf_pzgetrf(N, N, z, 1, 1, desc, zpiv, &info);
  check("pzgetrf info", info == 0);
  same = 1;
  for (int i = 0; i < N; ++i) same &= zpiv[i] == ipiv[i];
  check("pzgetrf pivots = pdgetrf pivots", same);
  dlaf_pzgetrs('N', N, 1, z, 1, 1, desc, zpiv, zb, 1, 1, descb, &info);
  check("pzgetrs info", info == 0);
  err = 0.0;
  for (int i = 0; i < N; ++i)
    err = fmax(err, fmax(fabs(zbr[2 * i] - 1.0), fabs(zbr[2 * i + 1])));
  printf("pzgetrs max |x - 1| = %.3e\n", err);
  check("pzgetrs x = 1", err <= 1e-12);

  /* a zero column: info names it, gesv leaves b alone */
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i)
      a2[i + (long)j * N] = j == 40 ? 0.0 : toeplitz_reversed(i, j);
  for (int i = 0; i < N; ++i) b2[i] = 3.0 + i;
  dlaf_pdgesv(N, 1, a2, 1, 1, desc, ipiv2, b2, 1, 1, descb, &info);
  check("pdgesv singular info = 41", info == 41);
  same = 1;
  for (int i = 0; i < N; ++i) same &= b2[i] == 3.0 + i;
  check("pdgesv singular leaves b", same);

  dlaf_finalize();
  if (fails) {
    printf("%d mismatches\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
