// LU with partial pivoting: the panel factorization and the row interchanges
// over the tile storage.
//
// Storage is [lr, lc, nb, nb], row-major tiles: element (r, c) sits at
// ((r / nb) * lc + c / nb) * nb * nb + (r % nb) * nb + c % nb.
//
// lu_panel factors tile column k (rows k*nb .. n-1, columns k*nb ..
// min((k+1)*nb, n)-1) in inner blocks of kLuW columns. No workgroup ever
// waits on another: everything that crosses workgroups crosses a kernel
// boundary of the stream.
//
//   step kernel, ONE launch per column. Workgroup i owns the kLuRows row
//   locations k*nb + i*kLuRows .. of the panel for the whole panel and is the
//   only reader and writer of those rows of the block. Launch j (column
//   g = b0 + j of the block that starts at b0)
//     1. reduces, redundantly in every workgroup and in one fixed order, the
//        candidates the previous launch left in the workspace: (CABS1 value,
//        row), larger value first, lower row on ties (i?amax's rule);
//     2. takes the pivot row's and the old top row's block values FROM THE
//        WORKSPACE; the owner of the pivot location stores the old top row
//        there, the owner of location g stores the pivot row;
//     3. scales its rows below g by the pivot (not when it is exactly zero:
//        the column stays unscaled, ?getf2's way) and applies the rank-1
//        update to the block columns right of g;
//     4. writes its best candidate for column g+1 (value, row, that row's
//        block values) into the OTHER half of the workspace; the owner of row
//        g+1 adds that row as the next top row.
//   The launch before a block's first column only does step 4. Workgroup 0
//   records ipiv[g] and the first zero pivot (info, 1-based); both stay on
//   the device. Every element and every workspace slot has one writer per
//   launch, so two runs give the same bits.
//
//   After a block: its interchanges go to the panel's other columns
//   (laswp_tiles), the block row right of it is solved against the block's
//   unit-lower triangle (one thread per column), and the rest of the panel
//   gets  A22 -= L21 * U12  from a plain LDS-staged kernel.
//
// Rows and columns at or beyond n (the identity padding of a partial last
// tile) are never searched, swapped, read into a result or written.
// Everything is computed in the working precision of S.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "kernels.h"

namespace dlaf {
namespace {

constexpr int kW = kLuW;
constexpr int kRows = kLuRows;   // threads per step workgroup, one row each
constexpr int kUpdRows = 32;     // rows per workgroup of the panel update
constexpr int kUpdCols = 64;     // columns per workgroup of the panel update
constexpr int kSolveCols = 64;   // columns per workgroup of the block-row solve

template <typename T>
__device__ inline T cabs1(T v) { return v < T(0) ? -v : v; }
template <typename T>
__device__ inline T cabs1(cplx<T> v) { return cabs1(v.re) + cabs1(v.im); }

template <typename T>
__device__ inline bool is_zero(T v) { return v == T(0); }
template <typename T>
__device__ inline bool is_zero(cplx<T> v) { return v.re == T(0) && v.im == T(0); }

template <typename T>
__device__ inline T divide(T x, T p) { return x / p; }
template <typename T>
__device__ inline cplx<T> divide(cplx<T> x, cplx<T> p) {
  const T d = p.re * p.re + p.im * p.im;
  return {(x.re * p.re + x.im * p.im) / d, (x.im * p.re - x.re * p.im) / d};
}

__device__ inline int64_t elem_off(int64_t r, int64_t c, int lc, int nb) {
  return ((r / nb) * lc + c / nb) * (int64_t)nb * nb + (r % nb) * (int64_t)nb +
         c % nb;
}

// Workspace: two halves (parity of the launch); each holds nwg candidate
// records and the top row, kW + 1 elements each: the row's block values, then
// the CABS1 value in the real part. wsrow[half][wg] is the candidate's row.
template <typename S>
__device__ inline S* ws_rec(S* ws, int half, int nwg, int rec) {
  return ws + ((int64_t)half * (nwg + 1) + rec) * (kW + 1);
}

// (value, row) reduction over the workgroup: larger value, then lower row.
// Every thread returns the winner. A value below zero means "no candidate".
template <typename R>
__device__ inline void best_of_block(R& v, int64_t& r, R* sv, int64_t* sr) {
  const int t = threadIdx.x;
  sv[t] = v;
  sr[t] = r;
  __syncthreads();
  for (int s = kRows / 2; s > 0; s >>= 1) {
    if (t < s) {
      const R ov = sv[t + s];
      const int64_t orow = sr[t + s];
      if (ov > sv[t] || (ov == sv[t] && orow < sr[t])) {
        sv[t] = ov;
        sr[t] = orow;
      }
    }
    __syncthreads();
  }
  v = sv[0];
  r = sr[0];
  __syncthreads();
}

// jj < 0: search only (candidates for the block's first column).
template <typename S>
__global__ __launch_bounds__(kRows) void lu_step_kernel(
    S* a, int lc, int nb, int64_t n, int64_t g0, int64_t b0, int wcur, int jj,
    int nwg, S* ws, int32_t* wsrow, int half_in, int32_t* ipiv,
    int32_t* info) {
  using R = typename ScalarTraits<S>::real_t;
  __shared__ R sv[kRows];
  __shared__ int64_t sr[kRows];
  __shared__ S sh_p[kW], sh_t[kW];

  const int t = threadIdx.x;
  const int wg = blockIdx.x;
  const int64_t r = g0 + (int64_t)wg * kRows + t;
  const bool valid = r < n;
  S* rowp = valid ? a + elem_off(r, b0, lc, nb) : nullptr;

  if (jj >= 0) {
    const int64_t g = b0 + jj;
    // 1. the winner among the candidates of the previous launch
    R bv = R(-1);
    int64_t br = INT64_MAX;
    for (int w = t; w < nwg; w += kRows) {
      const R v = ScalarTraits<S>::real(ws_rec(ws, half_in, nwg, w)[kW]);
      const int64_t row = wsrow[half_in * nwg + w];
      if (v > bv || (v == bv && row < br)) {
        bv = v;
        br = row;
      }
    }
    best_of_block(bv, br, sv, sr);
    // row g is always a candidate, so there is a winner; stay in bounds anyway
    const int64_t p = (bv >= R(0) && br >= g && br < n) ? br : g;
    const int pwg = (int)((p - g0) / kRows);
    // 2. pivot row and old top row, from the workspace
    if (t < wcur) {
      sh_p[t] = ws_rec(ws, half_in, nwg, pwg)[t];
      sh_t[t] = ws_rec(ws, half_in, nwg, nwg)[t];
    }
    __syncthreads();
    const S piv = sh_p[jj];
    const bool zero_piv = is_zero(piv);
    if (wg == 0 && t == 0) {
      ipiv[g] = (int32_t)p;
      if (zero_piv && *info == 0) *info = (int32_t)(g + 1);
    }
    if (valid && p != g) {
      if (r == p)
        for (int c = 0; c < wcur; ++c) rowp[c] = sh_t[c];
      else if (r == g)
        for (int c = 0; c < wcur; ++c) rowp[c] = sh_p[c];
    }
    // 3. scale and rank-1 update of the rows below g
    if (valid && r > g && !zero_piv) {
      const S l = divide(rowp[jj], piv);
      rowp[jj] = l;
      for (int c = jj + 1; c < wcur; ++c) rowp[c] = rowp[c] - l * sh_p[c];
    }
  }

  // 4. candidates for the next column
  const int jn = jj + 1;
  if (jn >= wcur) return;
  const int64_t gn = b0 + jn;
  R v = R(-1);
  int64_t row = INT64_MAX;
  if (valid && r >= gn) {
    v = cabs1(rowp[jn]);
    row = r;
  }
  __syncthreads();  // this workgroup's row stores, before other lanes read them
  best_of_block(v, row, sv, sr);
  const int half_out = half_in ^ 1;
  S* rec = ws_rec(ws, half_out, nwg, wg);
  if (t < wcur && v >= R(0)) rec[t] = a[elem_off(row, b0, lc, nb) + t];
  if (t == 0) {
    rec[kW] = ScalarTraits<S>::from_real(v);
    wsrow[half_out * nwg + wg] = (int32_t)(v >= R(0) ? row : INT_MAX);
  }
  if (gn >= g0 + (int64_t)wg * kRows && gn < g0 + (int64_t)(wg + 1) * kRows &&
      t < wcur)
    ws_rec(ws, half_out, nwg, nwg)[t] = a[elem_off(gn, b0, lc, nb) + t];
}

// U12 = L11^-1 A12 inside the diagonal tile: L11 the unit-lower wcur x wcur
// block at (lb0, lb0), A12 its block row, columns [lb0 + wcur, ncols). One
// thread per column; the column lives in the thread's own LDS lane, so the
// loops need no unrolling and nothing spills.
template <typename S>
__global__ __launch_bounds__(kSolveCols) void lu_rowsolve_kernel(
    S* __restrict__ tile, int nb, int lb0, int wcur, int ncols) {
  __shared__ S Ls[kW][kW + 1];
  __shared__ S Xs[kW][kSolveCols];
  const int t = threadIdx.x;
  for (int idx = t; idx < wcur * kW; idx += kSolveCols) {
    const int i = idx / kW, tt = idx % kW;
    if (tt < i) Ls[i][tt] = tile[(int64_t)(lb0 + i) * nb + lb0 + tt];
  }
  __syncthreads();
  const int c = lb0 + wcur + blockIdx.x * kSolveCols + t;
  if (c >= ncols) return;
  for (int i = 0; i < wcur; ++i) Xs[i][t] = tile[(int64_t)(lb0 + i) * nb + c];
  for (int i = 1; i < wcur; ++i) {
    S acc = Xs[i][t];
    for (int tt = 0; tt < i; ++tt) acc = acc - Ls[i][tt] * Xs[tt][t];
    Xs[i][t] = acc;
    tile[(int64_t)(lb0 + i) * nb + c] = acc;
  }
}

// A22 -= L21 U12: rows [r0, n) of the panel, columns [c0, c1) of tile column
// kc; L21 = columns [b0, b0 + wcur) of those rows, U12 = rows [b0, b0 + wcur)
// of those columns.
template <typename S>
__global__ __launch_bounds__(256) void lu_update_kernel(
    S* __restrict__ a, int lc, int nb, int64_t n, int64_t b0, int wcur,
    int64_t r0, int64_t c0, int64_t c1) {
  __shared__ S Us[kW][kUpdCols];
  __shared__ S Ls[kUpdRows][kW + 1];
  const int t = threadIdx.x;
  const int64_t cb = c0 + (int64_t)blockIdx.x * kUpdCols;
  const int64_t rb = r0 + (int64_t)blockIdx.y * kUpdRows;
  for (int idx = t; idx < kW * kUpdCols; idx += 256) {
    const int tt = idx / kUpdCols, cc = idx % kUpdCols;
    Us[tt][cc] = (tt < wcur && cb + cc < c1)
                     ? a[elem_off(b0 + tt, cb + cc, lc, nb)]
                     : ScalarTraits<S>::zero();
  }
  for (int idx = t; idx < kUpdRows * kW; idx += 256) {
    const int ri = idx / kW, tt = idx % kW;
    Ls[ri][tt] = (tt < wcur && rb + ri < n)
                     ? a[elem_off(rb + ri, b0 + tt, lc, nb)]
                     : ScalarTraits<S>::zero();
  }
  __syncthreads();
  const int tx = t % kUpdCols, ty = t / kUpdCols;
  const int64_t c = cb + tx;
  if (c >= c1) return;
  constexpr int kPer = kUpdRows / (256 / kUpdCols);
  for (int i = 0; i < kPer; ++i) {
    const int ri = ty * kPer + i;
    const int64_t r = rb + ri;
    if (r >= n) break;
    S* p = a + elem_off(r, c, lc, nb);
    S acc = *p;
#pragma unroll
    for (int tt = 0; tt < kW; ++tt) acc = acc - Ls[ri][tt] * Us[tt][tx];
    *p = acc;
  }
}

// One thread per column: walks the pivots in order, so the lanes of a wave
// move along one tile row and no two threads touch the same element.
template <typename S>
__global__ __launch_bounds__(256) void laswp_kernel(
    S* __restrict__ a, int lc, int mb, int nbc, int64_t nrows,
    const int32_t* __restrict__ ipiv, int64_t s0, int64_t s1, int64_t c0,
    int64_t c1, int reverse) {
  const int64_t c = c0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= c1) return;
  const int64_t tsz = (int64_t)mb * nbc;
  S* col = a + (c / nbc) * tsz + c % nbc;
  for (int64_t i = 0; i < s1 - s0; ++i) {
    const int64_t s = reverse ? s1 - 1 - i : s0 + i;
    const int64_t p = ipiv[s];
    if (p == s || p < 0 || p >= nrows) continue;
    S* x = col + (s / mb) * lc * tsz + (s % mb) * nbc;
    S* y = col + (p / mb) * lc * tsz + (p % mb) * nbc;
    const S tmp = *x;
    *x = *y;
    *y = tmp;
  }
}

}  // namespace

int64_t lu_panel_work_elems(int64_t n) {
  const int64_t nwg = (std::max<int64_t>(n, 1) + kRows - 1) / kRows;
  return 2 * (nwg + 1) * (kW + 1);
}
int64_t lu_panel_work_rows(int64_t n) {
  return 2 * ((std::max<int64_t>(n, 1) + kRows - 1) / kRows);
}

template <typename S>
void laswp_tiles(S* a, int lr, int lc, int mb, int nbc, const int32_t* ipiv,
                 int64_t s0, int64_t s1, int64_t c0, int64_t c1, int reverse,
                 hipStream_t stream) {
  if (s1 <= s0 || c1 <= c0 || lr <= 0 || lc <= 0) return;
  const unsigned grid = (unsigned)((c1 - c0 + 255) / 256);
  hipLaunchKernelGGL(laswp_kernel<S>, dim3(grid), dim3(256), 0, stream, a, lc,
                     mb, nbc, (int64_t)lr * mb, ipiv, s0, s1, c0, c1, reverse);
}

template <typename S>
void lu_panel(S* a, int nt, int nb, int64_t n, int k, int32_t* ipiv,
              int32_t* info, S* ws, int32_t* wsrow, hipStream_t stream) {
  const int64_t g0 = (int64_t)k * nb;
  if (g0 >= n) return;
  const int64_t cend = std::min<int64_t>(g0 + nb, n);  // panel columns end
  const int nwg = (int)((n - g0 + kRows - 1) / kRows);
  S* dtile = a + ((int64_t)k * nt + k) * (int64_t)nb * nb;
  int half = 0;
  for (int64_t b0 = g0; b0 < cend; b0 += kW) {
    const int wcur = (int)std::min<int64_t>(kW, cend - b0);
    for (int jj = -1; jj < wcur; ++jj) {
      hipLaunchKernelGGL(lu_step_kernel<S>, dim3(nwg), dim3(kRows), 0, stream,
                         a, nt, nb, n, g0, b0, wcur, jj, nwg, ws, wsrow, half,
                         ipiv, info);
      half ^= 1;
    }
    // the block's interchanges on the panel's other columns
    laswp_tiles(a, nt, nt, nb, nb, ipiv, b0, b0 + wcur, g0, b0, 0, stream);
    const int64_t c0 = b0 + wcur;
    if (c0 >= cend) continue;
    laswp_tiles(a, nt, nt, nb, nb, ipiv, b0, b0 + wcur, c0, cend, 0, stream);
    const int ncols = (int)(cend - g0);
    const int lb0 = (int)(b0 - g0);
    hipLaunchKernelGGL(lu_rowsolve_kernel<S>,
                       dim3((unsigned)((cend - c0 + kSolveCols - 1) /
                                       kSolveCols)),
                       dim3(kSolveCols), 0, stream, dtile, nb, lb0, wcur,
                       ncols);
    dim3 grid((unsigned)((cend - c0 + kUpdCols - 1) / kUpdCols),
              (unsigned)((n - c0 + kUpdRows - 1) / kUpdRows));
    hipLaunchKernelGGL(lu_update_kernel<S>, grid, dim3(256), 0, stream, a, nt,
                       nb, n, b0, wcur, c0, c0, cend);
  }
}

#define DLAF_LU_INST(S)                                                       \
  template void lu_panel<S>(S*, int, int, int64_t, int, int32_t*, int32_t*,   \
                            S*, int32_t*, hipStream_t);                       \
  template void laswp_tiles<S>(S*, int, int, int, int, const int32_t*,        \
                               int64_t, int64_t, int64_t, int64_t, int,       \
                               hipStream_t);
DLAF_LU_INST(float)
DLAF_LU_INST(double)
DLAF_LU_INST(cplx<float>)
DLAF_LU_INST(cplx<double>)
#undef DLAF_LU_INST

}  // namespace dlaf
