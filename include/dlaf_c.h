/* C API of dlaf_amd — counterpart of the reference's include/dlaf_c/
 * (grid.h, desc.h, init.h, factorization/cholesky.h, inverse/cholesky.h,
 * eigensolver/eigensolver.h, eigensolver/gen_eigensolver.h).
 *
 * The library (libdlaf_c.so) embeds a Python interpreter and forwards to
 * the dlaf_amd package, which runs the native HIP/CDNA4 algorithms; the
 * caller's buffers are wrapped without copies (column-major, leading
 * dimension ld, ScaLAPACK convention).
 *
 * Grids: nprow x npcol contexts. For multi-process grids launch one
 * process per rank with the torchrun-style rendezvous environment set
 * (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT); dlaf_create_grid then
 * initializes torch.distributed inside the embedded runtime (RCCL when a
 * GPU is visible, gloo otherwise) and nprow*npcol must equal WORLD_SIZE.
 * The reference builds grids from an MPI_Comm / BLACS context
 * (src/c_api/grid.cpp); this framework's rank rendezvous is the launcher
 * environment instead of MPI — there is no MPI/BLACS interop in the
 * MI355X-native design. Buffers are the caller's rank-local ScaLAPACK
 * block-cyclic panels, exactly as in the reference shims.
 */
#ifndef DLAF_C_H
#define DLAF_C_H

#ifdef __cplusplus
extern "C" {
#endif

struct DLAF_descriptor {
  int m, n, mb, nb;
  int isrc, jsrc;
  int i, j;
  int ld;
};

typedef struct { float re, im; } dlaf_complex_c;
typedef struct { double re, im; } dlaf_complex_z;

/* init / teardown of the embedded runtime (reference: dlaf_c/init.h) */
int dlaf_initialize(int argc, const char* const* argv);
void dlaf_finalize(void);

/* grid management (reference: dlaf_c/grid.h); see header comment for
 * multi-process grids */
int dlaf_create_grid(int nprow, int npcol, char order);
void dlaf_free_grid(int ctx);

/* Cholesky factorization, lower triangle in place (dlaf_c/factorization/cholesky.h) */
int dlaf_cholesky_factorization_s(int ctx, char uplo, float* a, struct DLAF_descriptor desc);
int dlaf_cholesky_factorization_d(int ctx, char uplo, double* a, struct DLAF_descriptor desc);
int dlaf_cholesky_factorization_c(int ctx, char uplo, dlaf_complex_c* a, struct DLAF_descriptor desc);
int dlaf_cholesky_factorization_z(int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desc);

/* A^-1 from the Cholesky factor (dlaf_c/inverse/cholesky.h) */
int dlaf_inverse_from_cholesky_factor_s(int ctx, char uplo, float* a, struct DLAF_descriptor desc);
int dlaf_inverse_from_cholesky_factor_d(int ctx, char uplo, double* a, struct DLAF_descriptor desc);
int dlaf_inverse_from_cholesky_factor_c(int ctx, char uplo, dlaf_complex_c* a, struct DLAF_descriptor desc);
int dlaf_inverse_from_cholesky_factor_z(int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desc);

/* symmetric / Hermitian eigensolver (dlaf_c/eigensolver/eigensolver.h):
 * eigenvalues into w (ascending), eigenvectors into z. */
int dlaf_symmetric_eigensolver_s(int ctx, char uplo, float* a, struct DLAF_descriptor desca,
                                 float* w, float* z, struct DLAF_descriptor descz);
int dlaf_symmetric_eigensolver_d(int ctx, char uplo, double* a, struct DLAF_descriptor desca,
                                 double* w, double* z, struct DLAF_descriptor descz);
int dlaf_hermitian_eigensolver_c(int ctx, char uplo, dlaf_complex_c* a, struct DLAF_descriptor desca,
                                 float* w, dlaf_complex_c* z, struct DLAF_descriptor descz);
int dlaf_hermitian_eigensolver_z(int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
                                 double* w, dlaf_complex_z* z, struct DLAF_descriptor descz);

/* partial spectrum [il, iu): 0-based half-open like the reference's
 * eigenvalues_index_begin/end */
int dlaf_symmetric_eigensolver_partial_spectrum_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor desca,
    double* w, double* z, struct DLAF_descriptor descz, long il, long iu);
int dlaf_hermitian_eigensolver_partial_spectrum_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor descz, long il, long iu);

/* generalized eigensolver A x = lambda B x (dlaf_c/eigensolver/gen_eigensolver.h);
 * the _factorized variants take B already Cholesky-factorized. */
int dlaf_symmetric_generalized_eigensolver_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor desca,
    double* b, struct DLAF_descriptor descb,
    double* w, double* z, struct DLAF_descriptor descz);
int dlaf_symmetric_generalized_eigensolver_factorized_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor desca,
    double* b, struct DLAF_descriptor descb,
    double* w, double* z, struct DLAF_descriptor descz);
int dlaf_hermitian_generalized_eigensolver_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
    dlaf_complex_z* b, struct DLAF_descriptor descb,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor descz);
int dlaf_hermitian_generalized_eigensolver_factorized_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
    dlaf_complex_z* b, struct DLAF_descriptor descb,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor descz);

/* eigenvalues only (ScaLAPACK jobz='N'): all n eigenvalues into w, ascending,
 * by Sturm bisection on the tridiagonal; no eigenvectors are formed. a (and
 * b, as in the eigensolver variants) is overwritten. */
int dlaf_symmetric_eigenvalues_d(int ctx, char uplo, double* a,
                                 struct DLAF_descriptor desca, double* w);
int dlaf_hermitian_eigenvalues_z(int ctx, char uplo, dlaf_complex_z* a,
                                 struct DLAF_descriptor desca, double* w);
int dlaf_symmetric_generalized_eigenvalues_d(
    int ctx, char uplo, double* a, struct DLAF_descriptor desca,
    double* b, struct DLAF_descriptor descb, double* w);
int dlaf_hermitian_generalized_eigenvalues_z(
    int ctx, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
    dlaf_complex_z* b, struct DLAF_descriptor descb, double* w);

/* ScaLAPACK-style shims (dlaf_pdpotrf etc.): desca is the 9-int ScaLAPACK
 * descriptor (DTYPE_, CTXT_, M_, N_, MB_, NB_, RSRC_, CSRC_, LLD_). */
void dlaf_pdpotrf(char uplo, int n, double* a, int ia, int ja, const int desca[9], int* info);
void dlaf_pspotrf(char uplo, int n, float* a, int ia, int ja, const int desca[9], int* info);
void dlaf_pzpotrf(char uplo, int n, dlaf_complex_z* a, int ia, int ja, const int desca[9], int* info);
void dlaf_pcpotrf(char uplo, int n, dlaf_complex_c* a, int ia, int ja, const int desca[9], int* info);
void dlaf_pdpotri(char uplo, int n, double* a, int ia, int ja, const int desca[9], int* info);
void dlaf_pdsyevd(char uplo, int n, double* a, int ia, int ja, const int desca[9],
                  double* w, double* z, int iz, int jz, const int descz[9], int* info);
void dlaf_pzheevd(char uplo, int n, dlaf_complex_z* a, int ia, int ja, const int desca[9],
                  double* w, dlaf_complex_z* z, int iz, int jz, const int descz[9], int* info);
void dlaf_pdsygvd(char uplo, int n, double* a, int ia, int ja, const int desca[9],
                  double* b, int ib, int jb, const int descb[9],
                  double* w, double* z, int iz, int jz, const int descz[9], int* info);


/* Matrix norms (ScaLAPACK p?lange / p?lansy / p?lanhe / p?lantr) of the
 * leading m x n (n x n) part of a, which is only read. norm: 'M' max |a_ij|,
 * '1' or 'O' one-norm, 'I' infinity-norm, 'F' or 'E' Frobenius. lansy / lanhe
 * read the uplo triangle only; lantr ignores the other triangle and with
 * diag = 'U' counts the diagonal as 1. ia = ja = 1. Returns NaN on error. */
double dlaf_pdlange(char norm, int m, int n, const double* a, int ia, int ja,
                    const int desca[9]);
double dlaf_pzlange(char norm, int m, int n, const dlaf_complex_z* a, int ia,
                    int ja, const int desca[9]);
double dlaf_pdlansy(char norm, char uplo, int n, const double* a, int ia,
                    int ja, const int desca[9]);
double dlaf_pzlanhe(char norm, char uplo, int n, const dlaf_complex_z* a,
                    int ia, int ja, const int desca[9]);
double dlaf_pdlantr(char norm, char uplo, char diag, int m, int n,
                    const double* a, int ia, int ja, const int desca[9]);

/* Condition estimates and the Cholesky solve (ScaLAPACK p?pocon / p?trcon /
 * p?potrs without the workspace arguments); a is only read, ia = ja = 1.
 * pocon: a holds the Cholesky factor left by p?potrf in its uplo triangle,
 * anorm is the one-norm of the matrix before it was factored (p?lansy /
 * p?lanhe); trcon: norm '1' / 'O' or 'I'. *rcond is the estimated reciprocal
 * condition number (0 for a singular matrix, 1 for n = 0). potrs overwrites b
 * (n x nrhs) with the solution of A X = B. *info = 0 on success. */
void dlaf_pdpocon(char uplo, int n, const double* a, int ia, int ja,
                  const int desca[9], double anorm, double* rcond, int* info);
void dlaf_pzpocon(char uplo, int n, const dlaf_complex_z* a, int ia, int ja,
                  const int desca[9], double anorm, double* rcond, int* info);
void dlaf_pdtrcon(char norm, char uplo, char diag, int n, const double* a,
                  int ia, int ja, const int desca[9], double* rcond,
                  int* info);
void dlaf_pztrcon(char norm, char uplo, char diag, int n,
                  const dlaf_complex_z* a, int ia, int ja, const int desca[9],
                  double* rcond, int* info);
void dlaf_pdpotrs(char uplo, int n, int nrhs, const double* a, int ia, int ja,
                  const int desca[9], double* b, int ib, int jb,
                  const int descb[9], int* info);

/* Refinement and the mixed-precision solve (p?porfs without the workspace
 * arguments; dsposv / zcposv over block-cyclic buffers); every i / j = 1.
 * porfs: a holds the Hermitian positive definite matrix, af its Cholesky
 * factor as left by p?potrf, b the right-hand sides (all three only read);
 * x (n x nrhs), a solution as p?potrs returns it, is refined in place.
 * ferr[nrhs] receives estimated bounds on the relative forward error of each
 * column, berr[nrhs] the componentwise relative backward errors.
 * sposv: factors in single precision and refines in double; x receives the
 * solution, a and b are only read (unlike LAPACK, no factor is left in a).
 * *iter >= 0 is the number of refinement steps; < 0 means that the solution
 * comes from a double precision factorization: -2 an entry overflows single
 * precision, -3 the single precision factorization failed, -31 no
 * convergence in 30 steps. *info = 0 on success, > 0 the order of the
 * leading minor that is not positive definite. */
void dlaf_pdporfs(char uplo, int n, int nrhs, const double* a, int ia, int ja,
                  const int desca[9], const double* af, int iaf, int jaf,
                  const int descaf[9], const double* b, int ib, int jb,
                  const int descb[9], double* x, int ix, int jx,
                  const int descx[9], double* ferr, double* berr, int* info);
void dlaf_pzporfs(char uplo, int n, int nrhs, const dlaf_complex_z* a, int ia,
                  int ja, const int desca[9], const dlaf_complex_z* af,
                  int iaf, int jaf, const int descaf[9],
                  const dlaf_complex_z* b, int ib, int jb, const int descb[9],
                  dlaf_complex_z* x, int ix, int jx, const int descx[9],
                  double* ferr, double* berr, int* info);
void dlaf_pdsposv(char uplo, int n, int nrhs, const double* a, int ia, int ja,
                  const int desca[9], const double* b, int ib, int jb,
                  const int descb[9], double* x, int ix, int jx,
                  const int descx[9], int* iter, int* info);
void dlaf_pzcposv(char uplo, int n, int nrhs, const dlaf_complex_z* a, int ia,
                  int ja, const int desca[9], const dlaf_complex_z* b, int ib,
                  int jb, const int descb[9], dlaf_complex_z* x, int ix,
                  int jx, const int descx[9], int* iter, int* info);

/* LU with partial pivoting (ScaLAPACK p?getrf / p?getrs / p?gecon / p?gesv
 * without the workspace arguments) on a 1 x 1 grid; every i / j = 1, m = n.
 * getrf overwrites a with its factors (unit-lower L below the diagonal, U on
 * and above it); ipiv[n] receives 1-based global row indices: row j was
 * interchanged with row ipiv[j - 1]. *info = 0, or the index of the first
 * exactly-zero pivot (the factorization is completed regardless), or -1 on a
 * bad argument. getrs overwrites b (n x nrhs) with the solution of
 * op(A) X = B, trans 'N' / 'T' / 'C'; a and ipiv as getrf left them, only
 * read. gecon: norm '1' / 'O' or 'I', anorm that norm of the matrix before
 * it was factored (p?lange); *rcond is the estimated reciprocal condition
 * number (0 for a singular U, 1 for n = 0). gesv = getrf, then getrs unless
 * *info > 0 (b is then left untouched). */
void dlaf_pdgetrf(int m, int n, double* a, int ia, int ja, const int desca[9],
                  int* ipiv, int* info);
void dlaf_pzgetrf(int m, int n, dlaf_complex_z* a, int ia, int ja,
                  const int desca[9], int* ipiv, int* info);
void dlaf_pdgetrs(char trans, int n, int nrhs, const double* a, int ia, int ja,
                  const int desca[9], const int* ipiv, double* b, int ib,
                  int jb, const int descb[9], int* info);
void dlaf_pzgetrs(char trans, int n, int nrhs, const dlaf_complex_z* a, int ia,
                  int ja, const int desca[9], const int* ipiv,
                  dlaf_complex_z* b, int ib, int jb, const int descb[9],
                  int* info);
void dlaf_pdgecon(char norm, int n, const double* a, int ia, int ja,
                  const int desca[9], double anorm, double* rcond, int* info);
void dlaf_pdgesv(int n, int nrhs, double* a, int ia, int ja,
                 const int desca[9], int* ipiv, double* b, int ib, int jb,
                 const int descb[9], int* info);

#ifdef __cplusplus
}
#endif
#endif /* DLAF_C_H */
