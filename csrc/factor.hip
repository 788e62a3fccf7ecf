// Single-tile factorization building blocks for CDNA4.
//
// * potrf_invert_block: single-workgroup LDS-resident Cholesky of one diagonal
//   block fused with its inversion.
// * potrf_tile_fused: the tile Cholesky of an nb x nb tile, right-looking over
//   64-column blocks, one launch per block column: every workgroup of launch d
//   recomputes the two panel blocks it needs against dinv[d-1] and updates its
//   own trailing block, and the diagonal workgroup goes on to factor and
//   invert it (csrc/potrf_plan.h has the decomposition and the ownership of
//   every write). Replaces the reference's rocSOLVER potrf call (SURVEY.md
//   §2.4).
// * trtri_lower: column-parallel lower-triangular inverse (thread-per-column
//   forward substitution). Triangular solves everywhere in the library are
//   GEMMs against these block inverses — the standard GPU TRSM trade.
#include <algorithm>

#include "kernels.h"
#include "potrf_plan.h"

namespace {

// Single-workgroup LDS-resident variant for blocks (n <= 128 real / 64
// complex): staging through LDS removes the global-latency-bound serial chain
// of the naive version (measured 21.8 ms -> tens of us for a 512 tile's
// blocks). One thread per column, forward substitution in LDS.
template <typename S, int BSZ>
__launch_bounds__(256) __global__ void trtri_block_lds_k(const S* L, S* T,
                                                         int n, int ldl,
                                                         int ldt,
                                                         int unit_diag) {
  using TR = ScalarTraits<S>;
  __shared__ S Ts[BSZ][BSZ + 1];  // the own-write substitution chain (latency-critical)
  const int tid = threadIdx.x;
  const int j = tid;
  if (j < n) {
    for (int i = 0; i < j; ++i) Ts[i][j] = TR::zero();
    const S djj = unit_diag ? TR::from_real(1) : TR::recip(L[(int64_t)j * ldl + j]);
    Ts[j][j] = djj;
    for (int i = j + 1; i < n; ++i) {
      S acc = TR::zero();
      const S* Lrow = L + (int64_t)i * ldl;  // L2-shared across all columns
      for (int p = j; p < i; ++p) acc += Lrow[p] * Ts[p][j];
      const S dii = unit_diag ? TR::from_real(1) : TR::recip(L[(int64_t)i * ldl + i]);
      Ts[i][j] = -(dii * acc);
    }
  }
  __syncthreads();
  for (int e = tid; e < BSZ * BSZ; e += 256) {
    const int i = e / BSZ, j2 = e % BSZ;
    if (i < n && j2 < n) T[(int64_t)i * ldt + j2] = Ts[i][j2];
  }
}

// ---- 64 x 64 factor + invert core -----------------------------------------
//
// LDS images have a leading dimension of kImgLd = 65 elements, odd in units
// of the element size: rows r and r+1 of one column sit one element apart in
// the bank row, so a column-direction access by up to 32 (8-byte elements) or
// 16 (16-byte elements) consecutive rows is conflict-free.
constexpr int kB = dlaf::kPotrfBsz;  // 64
constexpr int kImgLd = kB + 1;
static_assert(kB == 64, "the core below is written for 64 x 64 blocks");

template <typename S>
using Img = S (*)[kImgLd];

// value of lane `src` (the same for the whole wave, a constant once the
// caller's loops are unrolled) as a wave-uniform value: no LDS round trip
template <typename S>
__device__ __forceinline__ S read_lane(S v, int src) {
  constexpr int NW = sizeof(S) / 4;
  int w[NW];
  __builtin_memcpy(w, &v, sizeof(S));
#pragma unroll
  for (int q = 0; q < NW; ++q) w[q] = __builtin_amdgcn_readlane(w[q], src);
  __builtin_memcpy(&v, w, sizeof(S));
  return v;
}

// 1 / a on the critical path of the 16 x 16 factor: hardware estimate plus two
// Newton steps (about 1 ulp) instead of the long IEEE division sequence.
// a <= 0 or NaN gives a negative, infinite or NaN result, never a trap.
__device__ __forceinline__ double pivot_rcp(double a) {
  double x = __builtin_amdgcn_rcp(a);
  double e = fma(-a, x, 1.0);
  x = fma(x, e, x);
  e = fma(-a, x, 1.0);
  return fma(x, e, x);
}
__device__ __forceinline__ float pivot_rcp(float a) { return 1.0f / a; }

// One wave, no barrier, no LDS traffic inside the loops: Cholesky of the
// 16 x 16 diagonal block at (c0, c0) of L. Lane l holds ROW i = l & 15 of the
// block in 16 registers (the four 16-lane groups hold copies), so U[i][p] is
// the lane's own and U[j][p] is a readlane of the constant lane j.
//
// LDL^T-style elimination on unscaled columns
//   U[i][j] -= (U[i][p] / U[p][p]) conj(U[j][p])   (p < j)
// then L[:,j] = U[:,j] / sqrt(U[j][j]); rdiag[c0+j] = 1 / sqrt(U[j][j]) is
// kept for the panel solve. A non-positive pivot only shows in that last
// step, as a NaN column j: the columns before it stay exact. Entries above
// the diagonal are carried along and never feed one on or below it.
template <typename S>
__device__ inline void factor16_wave(Img<S> L,
                                     typename ScalarTraits<S>::real_t* rdiag,
                                     int c0, int lane) {
  using TR = ScalarTraits<S>;
  using RT = typename TR::real_t;
  const int i = lane & 15;
  S u[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) u[j] = L[c0 + i][c0 + j];
#pragma unroll
  for (int p = 0; p < 15; ++p) {
    const RT s = pivot_rcp(TR::real(read_lane(u[p], p)));
    const S w = u[p] * s;
#pragma unroll
    for (int j = p + 1; j < 16; ++j)
      u[j] -= w * TR::conj(read_lane(u[p], j));
  }
  RT dv = RT(0);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (i == j) dv = TR::real(u[j]);
  const RT sc = RT(1) / sqrt(dv);
#pragma unroll
  for (int j = 0; j < 16; ++j) u[j] = u[j] * read_lane(sc, j);
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j <= i) L[c0 + i][c0 + j] = u[j];
    rdiag[c0 + i] = sc;
  }
}

// One wave: inverse of the lower-triangular 16 x 16 block at (c0, c0) of L
// into the same place of T (strict upper part zero). Same lane layout;
// row-oriented forward substitution, so the rows above a NaN row stay clean.
template <typename S>
__device__ inline void invert16_wave(Img<S> L, Img<S> T, int c0, int lane) {
  using TR = ScalarTraits<S>;
  const int i = lane & 15;
  S l[16], t[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) l[j] = L[c0 + i][c0 + j];
  S dv = TR::from_real(1);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (i == j) dv = l[j];
  const S rd = TR::recip(dv);
#pragma unroll
  for (int c = 0; c < 16; ++c) t[c] = (c == i) ? rd : TR::zero();
  // row p of T is final when step p starts: T[p][c] = rd_p (delta_pc - sum);
  // rows i > p then take  t_i -= rd_i L[i][p] T[p][:]
#pragma unroll
  for (int p = 0; p < 15; ++p) {
    const S f = rd * l[p];
#pragma unroll
    for (int c = 0; c <= p; ++c) {
      const S tp = read_lane(t[c], p);
      if (i > p) t[c] -= f * tp;
    }
  }
  if (lane < 16) {
#pragma unroll
    for (int c = 0; c < 16; ++c)
      T[c0 + i][c0 + c] = (c <= i) ? t[c] : TR::zero();
  }
}

// Whole workgroup (256 threads). L holds the block: lower triangle live,
// identity on and zero below the diagonal outside the live n x n part, strict
// upper triangle never feeding a result. On return L holds the factor (if
// do_factor) and T its full inverse (zero strict upper triangle, identity
// outside the live part). Sc is a 32 x 33 scratch, rdiag holds 64 reals. T
// needs no initialisation. The caller puts a barrier between its writes of L
// and this call; the call ends on one.
template <typename S>
__device__ void factor_invert_core(Img<S> L, Img<S> T, S (*Sc)[33],
                                   typename ScalarTraits<S>::real_t* rdiag,
                                   int tid, int do_factor) {
  using TR = ScalarTraits<S>;
  for (int e = tid; e < kB * kImgLd; e += 256) (&T[0][0])[e] = TR::zero();
  if (do_factor) {
    for (int cb = 0; cb < 4; ++cb) {
      const int c0 = cb * 16;
      if (tid < 64) factor16_wave<S>(L, rdiag, c0, tid);
      __syncthreads();
      if (cb == 3) break;
      // panel below the 16-block, X L_cc^H = A: one row per thread, in
      // registers and in place (a thread reads and writes its own row only);
      // right-looking, so the 15 - j updates of a step are independent
      {
        const int r = c0 + 16 + tid;
        if (r < kB) {
          S a[16];
#pragma unroll
          for (int p = 0; p < 16; ++p) a[p] = L[r][c0 + p];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            a[j] = a[j] * rdiag[c0 + j];
#pragma unroll
            for (int q = j + 1; q < 16; ++q)
              a[q] -= a[j] * TR::conj(L[c0 + q][c0 + j]);
          }
#pragma unroll
          for (int p = 0; p < 16; ++p) L[r][c0 + p] = a[p];
        }
        __syncthreads();
      }
      // trailing update of the lower triangle, 16 x 16 sub-blocks, one
      // element per thread per sub-block
      {
        const int t0 = c0 + 16, m = 3 - cb;
        const int ti = tid >> 4, tj = tid & 15;
        for (int bi = 0; bi < m; ++bi) {
          S xi[16];
#pragma unroll
          for (int p = 0; p < 16; ++p) xi[p] = L[t0 + 16 * bi + ti][c0 + p];
          for (int bj = 0; bj <= bi; ++bj) {
            if (bj == bi && tj > ti) continue;
            const int rj = t0 + 16 * bj + tj;
            S acc = TR::zero();
#pragma unroll
            for (int p = 0; p < 16; ++p) acc += xi[p] * TR::conj(L[rj][c0 + p]);
            L[t0 + 16 * bi + ti][rj] -= acc;
          }
        }
        __syncthreads();
      }
    }
  } else {
    __syncthreads();  // T is zero before the diagonal blocks are written
  }
  // the four diagonal 16-blocks of the inverse are independent: one wave each
  invert16_wave<S>(L, T, (tid >> 6) * 16, tid & 63);
  __syncthreads();
  // off-diagonal 16-blocks of the inverse by distance from the diagonal:
  //   W = sum_P L_IP T_PJ (J <= P < I),  T_IJ = -T_II W
  for (int dist = 1; dist < 4; ++dist) {
    const int nblk = 4 - dist;
    for (int e = tid; e < nblk * 256; e += 256) {
      const int b = e >> 8, r = (e & 255) >> 4, c = e & 15;
      const int I = (b + dist) * 16, J = b * 16;
      S acc = TR::zero();
      for (int p = J; p < I; ++p) acc += L[I + r][p] * T[p][J + c];
      Sc[(b >> 1) * 16 + r][(b & 1) * 16 + c] = acc;
    }
    __syncthreads();
    for (int e = tid; e < nblk * 256; e += 256) {
      const int b = e >> 8, r = (e & 255) >> 4, c = e & 15;
      const int I = (b + dist) * 16, J = b * 16;
      S acc = TR::zero();
      for (int p = 0; p <= r; ++p)
        acc += T[I + r][I + p] * Sc[(b >> 1) * 16 + p][(b & 1) * 16 + c];
      T[I + r][J + c] = -acc;
    }
    __syncthreads();
  }
}

// store the live lower triangle of the factor and the whole inverse block
template <typename S>
__device__ inline void store_factor_and_inverse(Img<S> L, Img<S> T, S* A,
                                                int n, int ld, S* Tout,
                                                int tid, int store_factor) {
  for (int e = tid; e < kB * kB; e += 256) {
    const int i = e >> 6, j = e & 63;
    if (store_factor && i < n && j <= i) A[(int64_t)i * ld + j] = L[i][j];
    Tout[e] = T[i][j];
  }
}

// Stand-alone entry: [factor +] invert the leading n x n (n <= 64) of A into
// the 64 x 64 block Tout. Launch 0 of the tile factorization is this kernel.
// do_factor=0 inverts an already-factored block (a tile received after a
// broadcast); its strict upper triangle is not read.
template <typename S>
__launch_bounds__(256) __global__ void potrf_invert_block_k(S* A, int n,
                                                            int ld, S* Tout,
                                                            int do_factor) {
  using TR = ScalarTraits<S>;
  __shared__ S Li[kB][kImgLd];
  __shared__ S Ti[kB][kImgLd];
  __shared__ S Sc[32][33];
  __shared__ typename TR::real_t Rd[kB];
  const int tid = threadIdx.x;
  for (int e = tid; e < kB * kB; e += 256) {
    const int i = e >> 6, j = e & 63;
    Li[i][j] = (i < n && j <= i) ? A[(int64_t)i * ld + j]
                                 : (i == j ? TR::from_real(1) : TR::zero());
  }
  __syncthreads();
  factor_invert_core<S>(Li, Ti, Sc, Rd, tid, do_factor);
  store_factor_and_inverse<S>(Li, Ti, A, n, ld, Tout, tid, do_factor);
}

// Launch d >= 1 of the tile factorization: see potrf_plan.h for the
// decomposition and for which workgroup owns which write.
template <typename S>
__launch_bounds__(256) __global__ void potrf_step_k(S* A, int n, int ld,
                                                    S* dinv, S* side, int d,
                                                    int nbk) {
  using TR = ScalarTraits<S>;
  namespace plan = dlaf::potrf_plan;
  __shared__ S P0[kB][kImgLd];
  __shared__ S P1[kB][kImgLd];
  __shared__ S Sc[32][33];
  __shared__ typename TR::real_t Rd[kB];
  const int tid = threadIdx.x;
  int I, J;
  plan::block_of((int)blockIdx.x, nbk, d, &I, &J);
  const int c = d - 1;
  const int r0 = I * kB, s0 = J * kB, q0 = c * kB;  // tile rows / cols / panel col

  // column d-2 of the tile <- side half (d-2)&1 (written by launch d-1)
  for (int R = d - 1; R < nbk; ++R) {
    if (!plan::copies_row(I, J, nbk, d, R)) continue;
    const S* src = side + plan::side_offset((d - 2) & 1, R, nbk, kB);
    for (int e = tid; e < kB * kB; e += 256) {
      const int i = e >> 6, j = e & 63;
      if (R * kB + i < n)
        A[(int64_t)(R * kB + i) * ld + (q0 - kB) + j] = src[e];
    }
  }

  // P0 <- A[I,c], P1 <- dinv[c]; block column c is full (c < nbk-1)
  const S* Dc = dinv + (int64_t)c * kB * kB;
  for (int e = tid; e < kB * kB; e += 256) {
    const int i = e >> 6, j = e & 63;
    P0[i][j] = (r0 + i < n) ? A[(int64_t)(r0 + i) * ld + q0 + j] : TR::zero();
    P1[i][j] = Dc[e];
  }
  __syncthreads();

  // 4 x 4 outputs per thread: rows ty + 16a, columns tx + 16b
  const int ty = tid >> 4, tx = tid & 15;
  // X = P0 * dinv[c]^H; dinv[c] is lower triangular, so column block b of X
  // needs p < 16 (b+1) only
  auto panel_product = [&](S (&x)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) x[a][b] = TR::zero();
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
      for (int pp = 0; pp < 16; ++pp) {
        const int p = pb * 16 + pp;
        S av[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = P0[ty + 16 * a][p];
#pragma unroll
        for (int b = pb; b < 4; ++b) {
          const S dv = TR::conj(P1[tx + 16 * b][p]);
#pragma unroll
          for (int a = 0; a < 4; ++a) x[a][b] += av[a] * dv;
        }
      }
    }
  };

  S xi[4][4], xj[4][4];
  panel_product(xi);
  __syncthreads();
  if (I != J) {
    for (int e = tid; e < kB * kB; e += 256) {
      const int i = e >> 6, j = e & 63;
      P0[i][j] = (s0 + i < n) ? A[(int64_t)(s0 + i) * ld + q0 + j] : TR::zero();
    }
    __syncthreads();
    panel_product(xj);
    __syncthreads();
  }
  // every read of A[I,c], A[J,c] and dinv[c] is done: P0 <- X_I, P1 <- X_J
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      P0[ty + 16 * a][tx + 16 * b] = xi[a][b];
      P1[ty + 16 * a][tx + 16 * b] = (I != J) ? xj[a][b] : xi[a][b];
    }
  // X_I = L[I,c]: to the side half c&1, or in place in the last launch
  if (plan::writes_side(I, J, nbk, d)) {
    S* dst = side + plan::side_offset(c & 1, I, nbk, kB);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        dst[(ty + 16 * a) * kB + tx + 16 * b] = xi[a][b];
  } else if (plan::writes_panel_in_place(I, J, nbk, d)) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (r0 + ty + 16 * a < n)
          A[(int64_t)(r0 + ty + 16 * a) * ld + q0 + tx + 16 * b] = xi[a][b];
  }
  __syncthreads();

  // C = A[I,J] - X_I X_J^H
  S cv[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int gr = r0 + ty + 16 * a, gc = s0 + tx + 16 * b;
      const bool live = gr < n && gc < n && (I != J || gc <= gr);
      cv[a][b] = live ? A[(int64_t)gr * ld + gc] : TR::zero();
    }
  for (int q = 0; q < kB; ++q) {
    S av[4], bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) av[a] = P0[ty + 16 * a][q];
#pragma unroll
    for (int b = 0; b < 4; ++b) bv[b] = TR::conj(P1[tx + 16 * b][q]);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) cv[a][b] -= av[a] * bv[b];
  }

  if (!plan::factors(I, J, d)) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int gr = r0 + ty + 16 * a, gc = s0 + tx + 16 * b;
        if (gr < n && gc < n && (I != J || gc <= gr))
          A[(int64_t)gr * ld + gc] = cv[a][b];
      }
    return;
  }

  // workgroup (d,d): factor the updated block and write dinv[d]
  __syncthreads();  // all reads of X from P0 / P1 are done
  const int nl = min(kB, n - r0);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = ty + 16 * a, j = tx + 16 * b;
      P0[i][j] = (i < nl && j <= i) ? cv[a][b]
                                    : (i == j ? TR::from_real(1) : TR::zero());
    }
  __syncthreads();
  factor_invert_core<S>(P0, P1, Sc, Rd, tid, 1);
  store_factor_and_inverse<S>(P0, P1, A + (int64_t)r0 * ld + r0, nl, ld,
                              dinv + (int64_t)d * kB * kB, tid, 1);
}

template <typename S>
__global__ void trtri_lower_k(const S* L, S* T, int n, int ldl, int ldt,
                              int unit_diag) {
  using TR = ScalarTraits<S>;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  // zero the upper part of column j (full tiles feed fused GEMMs)
  for (int i = 0; i < j; ++i) T[(int64_t)i * ldt + j] = TR::zero();
  const S djj = unit_diag ? TR::from_real(1) : TR::recip(L[(int64_t)j * ldl + j]);
  T[(int64_t)j * ldt + j] = djj;
  for (int i = j + 1; i < n; ++i) {
    S acc = TR::zero();
    for (int p = j; p < i; ++p)
      acc += L[(int64_t)i * ldl + p] * T[(int64_t)p * ldt + j];
    const S dii = unit_diag ? TR::from_real(1) : TR::recip(L[(int64_t)i * ldl + i]);
    T[(int64_t)i * ldt + j] = -(dii * acc);
  }
}

}  // namespace

// Tout is the kPotrfBsz x kPotrfBsz dinv block (see kernels.h for the size).
template <typename S>
void dlaf::potrf_invert_block(S* A, int n, int ld, S* Tout, int do_factor,
                              hipStream_t stream) {
  potrf_invert_block_k<S><<<1, 256, 0, stream>>>(A, n, ld, Tout, do_factor);
}

// One launch per block column (potrf_plan.h); nothing but the stream orders
// them, and nothing is allocated or copied from the host.
template <typename S>
void dlaf::potrf_tile_fused(S* A, int n, int ld, S* dinv, S* side,
                            hipStream_t stream) {
  namespace plan = dlaf::potrf_plan;
  if (n <= 0) return;
  const int nbk = plan::nblocks(n, kPotrfBsz);
  potrf_invert_block_k<S>
      <<<1, 256, 0, stream>>>(A, std::min(n, kPotrfBsz), ld, dinv, 1);
  for (int d = 1; d < nbk; ++d)
    potrf_step_k<S>
        <<<plan::grid(nbk, d), 256, 0, stream>>>(A, n, ld, dinv, side, d, nbk);
}

template <typename S>
void dlaf::trtri_lower(const S* L, S* T, int n, int ldl, int ldt,
                       int unit_diag, hipStream_t stream) {
  // largest block whose [BSZ][BSZ+1] LDS image fits: 64 for c128, else 128
  constexpr int BSZ = sizeof(S) == 16 ? 64 : 128;
  if (n <= BSZ)
    trtri_block_lds_k<S, BSZ>
        <<<1, 256, 0, stream>>>(L, T, n, ldl, ldt, unit_diag);
  else
    trtri_lower_k<S>
        <<<(n + 255) / 256, 256, 0, stream>>>(L, T, n, ldl, ldt, unit_diag);
}

#define INSTANTIATE(S)                                                       \
  template void dlaf::potrf_invert_block(S*, int, int, S*, int, hipStream_t); \
  template void dlaf::potrf_tile_fused(S*, int, int, S*, S*, hipStream_t);    \
  template void dlaf::trtri_lower(const S*, S*, int, int, int, int, hipStream_t);
INSTANTIATE(double)
INSTANTIATE(float)
INSTANTIATE(cplx<double>)
INSTANTIATE(cplx<float>)
#undef INSTANTIATE
