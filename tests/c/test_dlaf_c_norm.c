/* C-ABI test of the matrix-norm entry points through libdlaf_c.so.
 *
 * The (2,-1) Toeplitz matrix of order n has max norm 2, one- and infinity-
 * norm 4 (any interior row or column: 1 + 2 + 1) and Frobenius norm
 * sqrt(4 n + 2 (n - 1)). The Hermitian variant puts -i / +i on the
 * off-diagonals (same moduli). lansy / lanhe / lantr get 1e30 in the
 * triangle they must not read; the lower triangle alone has one-norm 3 and
 * Frobenius norm sqrt(4 n + (n - 1)), with a unit diagonal 2 and
 * sqrt(n + (n - 1)). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dlaf_c.h"

#define N 48
#define NB 16

static int fails = 0;

static void expect(const char* what, double got, double want, double rel) {
  double err = fabs(got - want);
  printf("%s = %.17g (want %.17g)\n", what, got, want);
  if (!(err <= rel * want)) {
    printf("  MISMATCH\n");
    ++fails;
  }
}

int main(void) {
  double* ad = calloc((size_t)N * N, sizeof(double));
  double* al = calloc((size_t)N * N, sizeof(double));
  dlaf_complex_z* az = calloc((size_t)N * N, sizeof(dlaf_complex_z));
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      long k = i + (long)j * N; /* column-major */
      if (i == j) {
        ad[k] = al[k] = az[k].re = 2.0;
      } else if (i == j + 1) {
        ad[k] = al[k] = -1.0;
        az[k].im = -1.0;
      } else if (j == i + 1) {
        ad[k] = -1.0;
        al[k] = 1e30; /* upper triangle: must not be read */
        az[k].re = 1e30;
      } else if (j > i) {
        al[k] = 1e30;
        az[k].re = 1e30;
      }
    }
  const int desc[9] = {1, 0, N, N, NB, NB, 0, 0, N};
  const double fro = sqrt(4.0 * N + 2.0 * (N - 1));
  const double eps = 2.220446049250313e-16;

  expect("pdlange M", dlaf_pdlange('M', N, N, ad, 1, 1, desc), 2.0, 0.0);
  expect("pdlange 1", dlaf_pdlange('1', N, N, ad, 1, 1, desc), 4.0, 0.0);
  expect("pdlange O", dlaf_pdlange('O', N, N, ad, 1, 1, desc), 4.0, 0.0);
  expect("pdlange I", dlaf_pdlange('I', N, N, ad, 1, 1, desc), 4.0, 0.0);
  expect("pdlange F", dlaf_pdlange('F', N, N, ad, 1, 1, desc), fro, 4 * eps);
  expect("pdlange E", dlaf_pdlange('E', N, N, ad, 1, 1, desc), fro, 4 * eps);

  expect("pdlansy M", dlaf_pdlansy('M', 'L', N, al, 1, 1, desc), 2.0, 0.0);
  expect("pdlansy 1", dlaf_pdlansy('1', 'L', N, al, 1, 1, desc), 4.0, 0.0);
  expect("pdlansy I", dlaf_pdlansy('I', 'L', N, al, 1, 1, desc), 4.0, 0.0);
  expect("pdlansy F", dlaf_pdlansy('F', 'L', N, al, 1, 1, desc), fro, 4 * eps);

  expect("pzlanhe M", dlaf_pzlanhe('M', 'L', N, az, 1, 1, desc), 2.0, 0.0);
  expect("pzlanhe 1", dlaf_pzlanhe('1', 'L', N, az, 1, 1, desc), 4.0, 0.0);
  expect("pzlanhe F", dlaf_pzlanhe('F', 'L', N, az, 1, 1, desc), fro, 4 * eps);

  /* the stored lower triangle alone, as a general matrix */
  for (long k = 0; k < (long)N * N; ++k)
    if (az[k].re == 1e30) az[k].re = 0.0;
  expect("pzlange M", dlaf_pzlange('M', N, N, az, 1, 1, desc), 2.0, 0.0);
  expect("pzlange 1", dlaf_pzlange('1', N, N, az, 1, 1, desc), 3.0, 0.0);

  expect("pdlantr M", dlaf_pdlantr('M', 'L', 'N', N, N, al, 1, 1, desc), 2.0,
         0.0);
  expect("pdlantr 1", dlaf_pdlantr('1', 'L', 'N', N, N, al, 1, 1, desc), 3.0,
         0.0);
  expect("pdlantr I", dlaf_pdlantr('I', 'L', 'N', N, N, al, 1, 1, desc), 3.0,
         0.0);
  expect("pdlantr F", dlaf_pdlantr('F', 'L', 'N', N, N, al, 1, 1, desc),
         sqrt(4.0 * N + (N - 1)), 4 * eps);
  expect("pdlantr 1 unit", dlaf_pdlantr('1', 'L', 'U', N, N, al, 1, 1, desc),
         2.0, 0.0);
  expect("pdlantr F unit", dlaf_pdlantr('F', 'L', 'U', N, N, al, 1, 1, desc),
         sqrt((double)N + (N - 1)), 4 * eps);

  dlaf_finalize();
  if (fails) {
    printf("%d mismatches\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
