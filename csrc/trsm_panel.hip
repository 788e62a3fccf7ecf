// Single-launch panel TRSM of the right-looking Cholesky (gfx950, real types):
// every panel tile X (mb x nb) becomes X * tril(L)^-T in ONE kernel.
//
// The right-side solve is independent per row of X, so a workgroup that owns
// a strip of STRIP rows of one tile runs the whole blocked recurrence itself,
//     for d:  X[:, d] = (X[:, d] - sum_{e<d} X[:, e] * L[d, e]^T) * dinv[d]^T
// over the kPotrfBsz-wide column blocks d. No workgroup reads what another
// writes: no grid barrier, no flags, one wait for compute units per step of
// the factorization instead of one per gemm_fused launch (2 * nb/64 - 1).
//
// Work of one workgroup (256 threads, 4 waves; wave w owns columns
// [16w, 16w+16) of the current 64-column block, STRIP/16 MFMA fragments):
//   * the K dimension runs in "chunks" of one 64-column block. The chunks of
//     block d are (X[:, d-1], L[d, d-1]) first, then (X[:, e], L[d, e]) for
//     e = 0 .. d-2, then the apply chunk (T, dinv[d]) with T = X[:, d] - sum;
//   * the B operand of every chunk (L and dinv are constant during the
//     kernel) and the A operand of the e <= d-2 chunks (solved blocks this
//     workgroup wrote to the tile at least one whole block step earlier) are
//     loaded to registers one chunk ahead, so a global-memory latency is
//     covered by the 4 x BK = 16 LDS sub-steps of the chunk before;
//   * the block solved last (e = d-1) and T never take that round trip: they
//     sit in the LDS strip buffer Xs, which serves directly as the A operand;
//   * solved blocks go to their place in the tile; the later re-reads by other
//     threads of the same workgroup are ordered by the __syncthreads() of the
//     sub-steps in between (workgroup-scope release/acquire).
//
// L is read strictly below its block diagonal only (dinv supplies the
// diagonal), so stale values in its strict upper triangle never arrive here.
// Rows >= mb, columns >= nb stage zeros and are not stored; dinv is staged
// through the same guard, so only its live bs x bs part is read.
//
// Static LDS (double / float): STRIP = 16: 18.8 / 9.4 KiB, 32: 29.0 / 14.5 KiB.
// A 64-row strip (49.5 KiB, 403 registers in double) was measured and lost to
// 32 rows at every tile count (docs/DESIGN.md).
#include "gemm_common.h"

namespace {

constexpr int kBsz = dlaf::kPotrfBsz;  // 64: column block of the recurrence
constexpr int kBK = 16;                // K extent of one LDS sub-step
constexpr int kSub = kBsz / kBK;       // sub-steps per chunk

// One 64-deep K chunk of the recurrence. e == -1: the apply chunk of block d.
struct Chunk {
  int d, e;
  __device__ bool a_from_lds() const { return e < 0 || e == d - 1; }
  __device__ Chunk next() const {
    if (e < 0) return {d + 1, d};
    if (e == d - 1) return {d, d >= 2 ? 0 : -1};
    return {d, e + 1 <= d - 2 ? e + 1 : -1};
  }
};

template <typename T, int STRIP>
__launch_bounds__(256) __global__ void trsm_panel_k(
    T* base, const int64_t* __restrict__ tile_offs, const T* __restrict__ L,
    int ldl, const T* __restrict__ dinv, int mb, int nb, int ld, int strips) {
  static_assert(kBsz == 64 && STRIP % 16 == 0, "geometry");
  constexpr int NF = STRIP / 16;            // row fragments per wave
  constexpr int LA = STRIP * kBK / 256;     // A elements per thread, sub-step
  constexpr int LB = kBsz * kBK / 256;      // B elements per thread, sub-step
  static_assert(LA >= 1, "strip too short for 256 threads");
  using acc_t = typename Mfma<T>::acc_t;

  __shared__ T As[STRIP][kBK + 1];
  __shared__ T Bs[kBsz][kBK + 1];   // Bs[c][k] = B(k, c): rows of L / dinv
  __shared__ T Xs[STRIP][kBsz + 1];

  const int tile = blockIdx.x / strips;
  const int r0 = (blockIdx.x % strips) * STRIP;
  T* X = base + tile_offs[tile];

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int nblk = (nb + kBsz - 1) / kBsz;

  // staging coordinates of this thread inside one sub-step
  int arow[LA], acol[LA], brow[LB], bcol[LB];
#pragma unroll
  for (int j = 0; j < LA; ++j) {
    const int idx = j * 256 + tid;
    arow[j] = idx / kBK;
    acol[j] = idx % kBK;
  }
#pragma unroll
  for (int j = 0; j < LB; ++j) {
    const int idx = j * 256 + tid;
    brow[j] = idx / kBK;
    bcol[j] = idx % kBK;
  }

  // global -> registers for one whole chunk
  auto load_chunk = [&](Chunk c, T (&va)[kSub][LA], T (&vb)[kSub][LB]) {
    const int bs = min(kBsz, nb - c.d * kBsz);  // live rows of block d
    const T* Bsrc;
    int ldb, klim;
    if (c.e < 0) {
      Bsrc = dinv + (int64_t)c.d * kBsz * kBsz;
      ldb = kBsz;
      klim = bs;
    } else {
      Bsrc = L + (int64_t)c.d * kBsz * ldl + c.e * kBsz;
      ldb = ldl;
      klim = kBsz;
    }
#pragma unroll
    for (int s = 0; s < kSub; ++s)
#pragma unroll
      for (int j = 0; j < LB; ++j) {
        const int k = s * kBK + bcol[j];
        T v = T(0);
        if (brow[j] < bs && k < klim) v = Bsrc[(int64_t)brow[j] * ldb + k];
        vb[s][j] = v;
      }
    if (!c.a_from_lds()) {
      const T* Asrc = X + c.e * kBsz;
#pragma unroll
      for (int s = 0; s < kSub; ++s)
#pragma unroll
        for (int j = 0; j < LA; ++j) {
          const int gr = r0 + arow[j];
          T v = T(0);
          if (gr < mb) v = Asrc[(int64_t)gr * ld + s * kBK + acol[j]];
          va[s][j] = v;
        }
    }
  };

  acc_t acc[NF];
  auto clear_acc = [&]() {
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = {0, 0, 0, 0};
  };

  // the 4 sub-steps of one chunk: stage -> barrier -> MFMA -> barrier
  auto run_chunk = [&](Chunk c, T (&va)[kSub][LA], T (&vb)[kSub][LB]) {
    const bool alds = c.a_from_lds();
#pragma unroll
    for (int s = 0; s < kSub; ++s) {
#pragma unroll
      for (int j = 0; j < LB; ++j) Bs[brow[j]][bcol[j]] = vb[s][j];
      if (!alds) {
#pragma unroll
        for (int j = 0; j < LA; ++j) As[arow[j]][acol[j]] = va[s][j];
      }
      __syncthreads();
#pragma unroll
      for (int kq = 0; kq < kBK / 4; ++kq) {
        const T b = Bs[w * 16 + li][kq * 4 + lk];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const T a = alds ? Xs[f * 16 + li][s * kBK + kq * 4 + lk]
                           : As[f * 16 + li][kq * 4 + lk];
          acc[f] = Mfma<T>::mma(a, b, acc[f]);
        }
      }
      __syncthreads();
    }
  };

  T ra[kSub][LA], rb[kSub][LB];    // chunk in flight to LDS
  T na[kSub][LA], nbr[kSub][LB];   // chunk in flight from global memory
#pragma unroll
  for (int s = 0; s < kSub; ++s)
#pragma unroll
    for (int j = 0; j < LA; ++j) ra[s][j] = na[s][j] = T(0);

  // original X[:, d] in the accumulator layout, loaded one chunk ahead too
  T xo[NF][4];
  auto load_xo = [&](int d) {
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + f * 16 + Mfma<T>::acc_row(lk, r);
        const int col = d * kBsz + w * 16 + li;
        T x = T(0);
        if (row < mb && col < nb) x = X[(int64_t)row * ld + col];
        xo[f][r] = x;
      }
  };

  Chunk cur{0, -1};
  load_chunk(cur, ra, rb);
  load_xo(0);
  clear_acc();

  while (cur.d < nblk) {
    const Chunk nxt = cur.next();
    const bool more = nxt.d < nblk;
    if (more) {
      load_chunk(nxt, na, nbr);
      if (nxt.e < 0) load_xo(nxt.d);
    }

    const int c0 = cur.d * kBsz;
    if (cur.e < 0) {
      // T = X[:, d] - sum, into Xs as the A operand of the apply chunk. The
      // barrier that ended the previous sub-step lets Xs be overwritten.
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = f * 16 + Mfma<T>::acc_row(lk, r);
          Xs[row][w * 16 + li] = xo[f][r] - (T)acc[f][r];
        }
      clear_acc();
    }

    run_chunk(cur, ra, rb);

    if (cur.e < 0) {
      // solved block: to its place in the tile and into Xs for chunk (d+1, d)
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = f * 16 + Mfma<T>::acc_row(lk, r);
          const int col = w * 16 + li;
          const T v = (T)acc[f][r];
          Xs[row][col] = v;
          if (r0 + row < mb && c0 + col < nb)
            X[(int64_t)(r0 + row) * ld + c0 + col] = v;
        }
      clear_acc();
    }

    if (more) {
#pragma unroll
      for (int s = 0; s < kSub; ++s) {
#pragma unroll
        for (int j = 0; j < LA; ++j) ra[s][j] = na[s][j];
#pragma unroll
        for (int j = 0; j < LB; ++j) rb[s][j] = nbr[s][j];
      }
    }
    cur = nxt;
  }
}

template <typename T, int STRIP>
void launch(T* base, const int64_t* tile_offs, int ntiles, const T* L, int ldl,
            const T* dinv, int mb, int nb, int ld, hipStream_t stream) {
  const int strips = (mb + STRIP - 1) / STRIP;
  hipLaunchKernelGGL((trsm_panel_k<T, STRIP>), dim3(ntiles * strips), dim3(256),
                     0, stream, base, tile_offs, L, ldl, dinv, mb, nb, ld,
                     strips);
}

}  // namespace

int dlaf::trsm_panel_strip(int ntiles, int mb) {
  // The solve of one strip is a serial chain of nblk * (nblk + 1) / 2 chunks,
  // so as long as 16-row strips leave every CU at most one workgroup they
  // finish first (77 against 101 us for one 512 tile in double); beyond that
  // the A reuse of 32 rows wins (293 against 399 us for 63 tiles).
  return (int64_t)ntiles * ((mb + 15) / 16) <= 256 ? 16 : 32;
}

template <typename S>
void dlaf::trsm_panel_fused(S* base, const int64_t* tile_offs, int ntiles,
                            const S* L, int ldl, const S* dinv, int mb, int nb,
                            int ld, hipStream_t stream) {
  trsm_panel_fused_strip(base, tile_offs, ntiles, L, ldl, dinv, mb, nb, ld,
                         trsm_panel_strip(ntiles, mb), stream);
}

template <typename S>
void dlaf::trsm_panel_fused_strip(S* base, const int64_t* tile_offs,
                                  int ntiles, const S* L, int ldl,
                                  const S* dinv, int mb, int nb, int ld,
                                  int strip, hipStream_t stream) {
  if (ntiles <= 0 || mb <= 0 || nb <= 0) return;
  switch (strip) {
    case 16:
      launch<S, 16>(base, tile_offs, ntiles, L, ldl, dinv, mb, nb, ld, stream);
      break;
    default:
      launch<S, 32>(base, tile_offs, ntiles, L, ldl, dinv, mb, nb, ld, stream);
  }
}

#define INSTANTIATE(S)                                                       \
  template void dlaf::trsm_panel_fused<S>(S*, const int64_t*, int, const S*, \
                                          int, const S*, int, int, int,      \
                                          hipStream_t);                      \
  template void dlaf::trsm_panel_fused_strip<S>(S*, const int64_t*, int,     \
                                                const S*, int, const S*, int, \
                                                int, int, int, hipStream_t);
INSTANTIATE(double)
INSTANTIATE(float)
#undef INSTANTIATE
