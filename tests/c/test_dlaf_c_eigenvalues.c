/* C-ABI test of the eigenvalues-only entry points through libdlaf_c.so.
 *
 * The (2,-1) Toeplitz matrix of order n has eigenvalues
 * 2 - 2 cos(k pi / (n+1)), k = 1..n. The Hermitian variant puts -i / +i on
 * the off-diagonals (same moduli, same spectrum); the generalized variants
 * use B = 2 I, which halves every eigenvalue. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dlaf_c.h"

#define N 48
#define NB 16

static const double kPi = 3.14159265358979323846;

static int check(const char* what, const double* w, double scale) {
  double err = 0.0;
  for (int k = 0; k < N; ++k) {
    double ref = scale * (2.0 - 2.0 * cos((k + 1) * kPi / (N + 1)));
    double e = fabs(w[k] - ref);
    if (e > err) err = e;
    if (k && w[k] < w[k - 1]) {
      printf("%s: not ascending at %d\n", what, k);
      return 1;
    }
  }
  printf("%s max error %.3e\n", what, err);
  return err > 1e-11 * N * 4.0;
}

static void fill_d(double* a, double* b) {
  memset(a, 0, sizeof(double) * N * N);
  memset(b, 0, sizeof(double) * N * N);
  for (int i = 0; i < N; ++i) {
    a[i + (long)i * N] = 2.0;
    b[i + (long)i * N] = 2.0;
    if (i + 1 < N) {
      a[i + 1 + (long)i * N] = -1.0;
      a[i + (long)(i + 1) * N] = -1.0;
    }
  }
}

static void fill_z(dlaf_complex_z* a, dlaf_complex_z* b) {
  memset(a, 0, sizeof(dlaf_complex_z) * N * N);
  memset(b, 0, sizeof(dlaf_complex_z) * N * N);
  for (int i = 0; i < N; ++i) {
    a[i + (long)i * N].re = 2.0;
    b[i + (long)i * N].re = 2.0;
    if (i + 1 < N) {
      a[i + 1 + (long)i * N].im = -1.0;
      a[i + (long)(i + 1) * N].im = 1.0;
    }
  }
}

int main(void) {
  if (dlaf_initialize(0, NULL) != 0) return 1;
  int ctx = dlaf_create_grid(1, 1, 'R');
  if (ctx < 0) return 2;
  struct DLAF_descriptor d = {N, N, NB, NB, 0, 0, 1, 1, N};

  double* ad = malloc(sizeof(double) * N * N);
  double* bd = malloc(sizeof(double) * N * N);
  dlaf_complex_z* az = malloc(sizeof(dlaf_complex_z) * N * N);
  dlaf_complex_z* bz = malloc(sizeof(dlaf_complex_z) * N * N);
  double w[N];

  fill_d(ad, bd);
  if (dlaf_symmetric_eigenvalues_d(ctx, 'L', ad, d, w) != 0) return 3;
  if (check("symmetric_eigenvalues_d", w, 1.0)) return 4;

  fill_z(az, bz);
  if (dlaf_hermitian_eigenvalues_z(ctx, 'L', az, d, w) != 0) return 5;
  if (check("hermitian_eigenvalues_z", w, 1.0)) return 6;

  fill_d(ad, bd);
  if (dlaf_symmetric_generalized_eigenvalues_d(ctx, 'L', ad, d, bd, d, w) != 0)
    return 7;
  if (check("symmetric_generalized_eigenvalues_d", w, 0.5)) return 8;

  fill_z(az, bz);
  if (dlaf_hermitian_generalized_eigenvalues_z(ctx, 'L', az, d, bz, d, w) != 0)
    return 9;
  if (check("hermitian_generalized_eigenvalues_z", w, 0.5)) return 10;

  dlaf_free_grid(ctx);
  dlaf_finalize();
  printf("OK\n");
  return 0;
}
