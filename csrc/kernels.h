// Every native entry point of the extension, declared once.
//
// Design (see SURVEY.md §2.4/§2.5 for the reference per-tile op inventory this
// replaces): instead of one kernel launch per tile task, the hot ops are FUSED —
// one launch processes a whole list of tile-triples described by GemmDesc records,
// so a full trailing update / panel solve / back-transform sweep is a single
// kernel with >> 256 workgroups (MI355X: 256 CUs over 8 XCDs).
//
// Entry points are templates on the element type S: double, float,
// cplx<double>, cplx<float> (cplx.h; layout-identical to torch's interleaved
// complex). Each is defined in its .hip file under its qualified name
// (`dlaf::name`) and explicitly instantiated there, so a definition that
// drifts from the declaration here fails to compile.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cplx.h"

// op codes (match dlaf_amd.types.Op encoding used by the Python layer)
#define OP_N 0
#define OP_T 1
#define OP_C 2

// One fused-GEMM work item: C[c_off] += alpha * op(A[c_off]) * op(B[b_off]).
// Offsets are in ELEMENTS from the base pointers. A K-loop over `ktiles`
// operand tiles with the given element strides runs inside the kernel.
struct GemmDesc {
  int64_t c_off;
  int64_t a_off;
  int64_t b_off;
  int64_t ktiles;     // number of K tiles (>=1); total K = ktiles * K_param
  int64_t a_kstride;  // element stride between consecutive K tiles of A
  int64_t b_kstride;  // element stride between consecutive K tiles of B
};

namespace dlaf {

// Diagonal-block size of the tile Cholesky (dinv blocks are kPotrfBsz^2).
// 64 for every dtype: the factor+invert kernels then need ~73 KiB LDS in
// double (~147 KiB in cplx<double>) and can co-reside with trailing-update
// GEMM blocks on a CU — a 128-block (160 KiB) kernel can never be scheduled
// next to them and serializes the lookahead.
constexpr int kPotrfBsz = 64;

// ---- fused batched GEMM (MFMA f64 / f32), csrc/gemm_tiles.hip ----
// C (M x N, ldc), op(A) (M x K), op(B) (K x N); K is the per-tile K extent.
// Full-tile, non-aliased batches run on the glds kernel (gemm_tiles_v2),
// everything else on the guarded register-staged kernel. Real S: OP_C == OP_T,
// and `inplace` selects the wide-BN instantiation that makes X = X*op(B) safe
// in place (C block == A block); required whenever C aliases A.
template <typename T>
void gemm_tiles(const GemmDesc* descs, int ndesc, const T* A, const T* B, T* C,
                int M, int N, int K, int lda, int ldb, int ldc, int opA,
                int opB, T alpha, T beta, hipStream_t stream, int inplace);
// Complex S (opA/opB support OP_C). `inplace` is accepted and ignored: a 64x64
// block per workgroup is in-place safe only while N <= 64, which the Python
// layer guarantees by staging A otherwise (tile_ops.gemm_fused).
template <typename T>
void gemm_tiles(const GemmDesc* descs, int ndesc, const cplx<T>* A,
                const cplx<T>* B, cplx<T>* C, int M, int N, int K, int lda,
                int ldb, int ldc, int opA, int opB, cplx<T> alpha, cplx<T> beta,
                hipStream_t stream, int inplace);

// ---- glds full-tile fast path, csrc/gemm_tiles_v2.hip ----
// Launches and returns true when the shape qualifies (real: M%128, N%64,
// K%16 all zero; complex: M%64, N%64, K%16; K > 0); else returns false and
// launches nothing. C must not alias A or B.
template <typename T>
bool gemm_tiles_v2(const GemmDesc* descs, int ndesc, const T* A, const T* B,
                   T* C, int M, int N, int K, int lda, int ldb, int ldc,
                   int opA, int opB, T alpha, T beta, hipStream_t stream);
template <typename T>
bool gemm_tiles_v2(const GemmDesc* descs, int ndesc, const cplx<T>* A,
                   const cplx<T>* B, cplx<T>* C, int M, int N, int K, int lda,
                   int ldb, int ldc, int opA, int opB, cplx<T> alpha,
                   cplx<T> beta, hipStream_t stream);

// ---- bt window-chain group apply (one launch per sweep group), bt_apply.hip
// S = double or cplx<double>. Returns false when (b, G, R) has no kernel.
template <typename S>
bool bt_apply_group(S* E, int64_t nE, int64_t npad, const S* V, const S* VTt,
                    int64_t base0, int b, int G, int R, int nwin,
                    hipStream_t stream);

// ---- single-tile factorization building blocks, csrc/factor.hip ----
// Fused single-workgroup [factor +] invert of one diagonal block: factors the
// leading n x n (n <= kPotrfBsz, if do_factor) in place and writes its inverse
// into the kPotrfBsz x kPotrfBsz block Tout (identity-extended).
template <typename S>
void potrf_invert_block(S* A, int n, int ld, S* Tout, int do_factor,
                        hipStream_t stream);

// In-place lower Cholesky of the leading n x n of a tile (row stride ld) in
// ceil(n / kPotrfBsz) stream-ordered launches (decomposition: potrf_plan.h).
// dinv[d] (kPotrfBsz^2 elements each) receives the identity-extended inverse
// of diagonal block d; `side` is a workspace of potrf_plan::side_elems()
// elements that needs no clearing and carries nothing between calls. The
// strict upper triangle of the tile is neither read nor written. The first
// failed pivot leaves a NaN on its diagonal; columns before it are exact.
template <typename S>
void potrf_tile_fused(S* A, int n, int ld, S* dinv, S* side,
                      hipStream_t stream);

// Column-parallel inverse of a lower-triangular n x n block (arbitrary n;
// single LDS-resident workgroup when it fits): T = L^-1, T may not alias L.
template <typename S>
void trtri_lower(const S* L, S* T, int n, int ldl, int ldt, int unit_diag,
                 hipStream_t stream);

// ---- single-launch panel TRSM, csrc/trsm_panel.hip ----
// S = double or float. Every tile t at base + tile_offs[t] (mb x nb, row
// stride ld; tile_offs device-resident, in elements) is overwritten with
// X * tril(L)^-T by the blocked recurrence over kPotrfBsz-wide column blocks
//   X[:, d] = (X[:, d] - X[:, :d] * L[d, :d]^T) * dinv[d]^T,
// dinv[d] the identity-extended inverse of diagonal block d as potrf_tile_fused
// writes it. L is read strictly below its block diagonal only: its diagonal
// blocks and strict upper triangle never reach the result. One plain launch
// of ntiles * ceil(mb / strip) workgroups, each owning its rows for the whole
// solve (no workgroup reads what another writes); nothing is read back and
// ntiles <= 0 launches nothing. Any mb, nb >= 1; rows and columns outside
// mb x nb are neither read into a result nor written. Tiles may not overlap
// each other, L or dinv. The strip height (16 or 32 rows) comes from
// trsm_panel_strip, a function of (ntiles, mb) alone, so a given call shape
// always takes the same summation order; trsm_panel_fused_strip takes it
// explicitly (tools/microbench.py).
int trsm_panel_strip(int ntiles, int mb);
template <typename S>
void trsm_panel_fused(S* base, const int64_t* tile_offs, int ntiles,
                      const S* L, int ldl, const S* dinv, int mb, int nb,
                      int ld, hipStream_t stream);
template <typename S>
void trsm_panel_fused_strip(S* base, const int64_t* tile_offs, int ntiles,
                            const S* L, int ldl, const S* dinv, int mb, int nb,
                            int ld, int strip, hipStream_t stream);

// ---- GPU bulge chase band -> tridiagonal, csrc/chase_gpu.hip ----
template <typename S>
void chase_gpu(S* a, int64_t ld, int64_t size, int64_t b, S* vstore,
               const int64_t* offsets, int32_t* done, int32_t* abortf,
               hipStream_t stream);

// ---- cooperative whole-panel QR, csrc/panel_qr.hip ----
// Returns 0 on success, else the hipError of the cooperative launch.
// norms/wraw must be zeroed by the caller.
template <typename S>
int panel_qr(S* P, long m, int nb, long ldp, S* taus,
             typename ScalarTraits<S>::real_t* norms, S* wraw,
             hipStream_t stream);

// ---- D&C secular-equation roots, csrc/secular.hip ----
void secular_roots(const double* d, const double* z2, int k, double rho,
                   long long* sidx, double* mu, hipStream_t stream);

// ---- tridiagonal eigenvalues by Sturm bisection, csrc/bisect.hip ----
// e2[i] = e[i]^2 (n-1 entries); gl/gu/pivmin as sturm::interval computes them.
// w[k - k_begin] = eigenvalue k (ascending) for k in [k_begin, k_end);
// count[j] = number of eigenvalues strictly below x[j]. n <= 0 or an empty
// range launches nothing. d/e2 are staged through LDS kBisectChunk at a time.
constexpr int kBisectChunk = 1024;
void tridiag_bisect(const double* d, const double* e2, int n, int k_begin,
                    int k_end, double gl, double gu, double pivmin, double* w,
                    hipStream_t stream);
void sturm_count(const double* d, const double* e2, int n, double pivmin,
                 const double* x, int nx, long long* count, hipStream_t stream);

// ---- shifted tridiagonal solves for inverse iteration, csrc/invit.hip ----
// (T - lam[j] I) y_j = x_j for columns j < k, in place on X (row i of column
// j at X[i*ldx + j]), by the pivoted LU of tridiag_lu.h with pivot floor tol.
// e has n-1 entries (not squared). work holds the U rows as [3, n, cols],
// cols >= k. n <= 0 or k <= 0 launches nothing.
void tridiag_shifted_solve(const double* d, const double* e, int n,
                           const double* lam, int k, double tol, double* X,
                           long long ldx, double* work, long long cols,
                           hipStream_t stream);

// ---- matrix norms over the local tile storage, csrc/norms.hip ----
// One pass over a [tiles_r, tiles_c, mb, nb] storage: rows[tiles_r * mb] and
// cols[tiles_c * nb] get the absolute sums per LOCAL row / column, scal[4] =
// (max |a|, Blue's small, medium, big sums of squares). Local tile l sits at
// global tile g0 + l * gs; elements at global (row, col) outside (m, n) or
// outside the structure's triangle count as absent. structure: 0 general,
// 1 hermitian (off-diagonal a_ij stands for a_ji too: its |a_ij| goes to the
// row AND the column sum, twice into the squares; the diagonal counts
// |Re a_ii| once, in the column sum), 2 triangular (unit_diag: diagonal = 1).
// uplo: 0 Lower, 1 Upper. work holds matrix_norms_work_size() doubles and
// needs no clearing. tiles_r <= 0 or tiles_c <= 0 launches nothing.
constexpr int kNormStripRows = 64;
int64_t matrix_norms_work_size(int tiles_r, int tiles_c, int mb, int nb);
template <typename S>
void matrix_norms(const S* a, int tiles_r, int tiles_c, int mb, int nb,
                  int64_t m, int64_t n, int gr0, int grs, int gc0, int gcs,
                  int structure, int uplo, int unit_diag, double* rows,
                  double* cols, double* scal, double* work,
                  hipStream_t stream);

// ---- triangular solve for one vector over the tile storage, csrc/trsv.hip
// op(T) x = b in place on x [nt * nb], T the uplo (0 Lower, 1 Upper) triangle
// of the local [nt, nt, nb, nb] storage a, op = OP_N / OP_T / OP_C. dinv
// [nt, nb, nb] holds the full-tile inverses of the diagonal tiles (built with
// the Unit / NonUnit choice, so the stored diagonal is never read here); work
// holds nb elements. Rows and columns at or beyond n (the identity padding of
// a partial last tile) are neither read into a sum nor written. 2 * nt plain
// launches on the stream; nt <= 0 or n <= 0 launches nothing.
template <typename S>
void trsv_tiles(const S* a, const S* dinv, S* x, S* work, int nt, int nb,
                int64_t n, int uplo, int op, hipStream_t stream);

// ---- Hermitian matrix-vector product over the tile storage, csrc/hemv.hip
// y = A x and, when yabs is not null, yabs = |A| |x| (CABS1) from the same
// pass; A is the Hermitian matrix whose uplo (0 Lower, 1 Upper) triangle is
// in the local [nt, nt, nb, nb] storage a, x / y / yabs hold nt * nb
// elements. Every stored element of the triangle is read once; the other
// triangle, the imaginary part of the diagonal and rows and columns at or
// beyond n are never read into a sum, and y / yabs are not written at or
// beyond n. work holds hemv_work_size() doubles and needs no clearing. Two
// plain launches on the stream; nt <= 0 or n <= 0 launches nothing.
constexpr int kHemvStripRows = 64;
int64_t hemv_work_size(int nt, int nb);
template <typename S>
void hemv_tiles(const S* a, const S* x, S* y,
                typename ScalarTraits<S>::real_t* yabs, int nt, int nb,
                int64_t n, int uplo, double* work, hipStream_t stream);

// ---- LU with partial pivoting over the tile storage, csrc/lu_panel.hip ----
// lu_panel factors tile column k of the square [nt, nt, nb, nb] storage a in
// place: rows k*nb .. n-1, columns k*nb .. min((k+1)*nb, n)-1, pivot = the
// first row of the largest CABS1 value (LAPACK's i?amax). ipiv[g] (0-based
// row, >= g) is written for the panel's columns g; *info receives g + 1 of the
// first exactly-zero pivot while it is still 0 (the column is left unscaled
// and the factorization goes on). The interchanges are applied to the
// panel's own columns only. ws / wsrow hold lu_panel_work_elems(n) elements /
// lu_panel_work_rows(n) int32 and need no clearing. One launch per column
// plus four per inner block of kLuW columns, all on the stream; nothing is
// read back. Rows and columns at or beyond n are neither read into a result
// nor written. k*nb >= n launches nothing.
constexpr int kLuW = 32;
constexpr int kLuRows = 256;
int64_t lu_panel_work_elems(int64_t n);
int64_t lu_panel_work_rows(int64_t n);
template <typename S>
void lu_panel(S* a, int nt, int nb, int64_t n, int k, int32_t* ipiv,
              int32_t* info, S* ws, int32_t* wsrow, hipStream_t stream);

// Row interchanges on a [lr, lc, mb, nbc] storage: for s in [s0, s1) (from
// s1-1 down when reverse), rows s and ipiv[s] (0-based) swap in the element
// columns [c0, c1). One thread per column; a pivot outside the storage's
// rows is skipped. An empty range launches nothing.
template <typename S>
void laswp_tiles(S* a, int lr, int lc, int mb, int nbc, const int32_t* ipiv,
                 int64_t s0, int64_t s1, int64_t c0, int64_t c1, int reverse,
                 hipStream_t stream);

}  // namespace dlaf
