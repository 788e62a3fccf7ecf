// Triangular solve for ONE vector over a local tile storage: op(T) x = b, in
// place on x (length nt * nb), T the `uplo` triangle of a [nt, nt, nb, nb]
// storage of row-major tiles (the layout norms.hip walks).
//
// The solve is memory-bound (every element of the triangle is read once), so
// it is built from two streaming matrix-vector kernels and a host loop over
// the nt tile steps. Step k (k ascending when op(T) is lower triangular, i.e.
// Lower/N and Upper/T,C; descending for Lower/T,C and Upper/N) issues two
// plain launches on the stream:
//   1. y    = op(Dinv_k) x_k            one tile, Dinv_k = inverse of T_kk
//   2. x_i -= op(T)_ik y  for every remaining i, and x_k = y
// The diagonal tiles are applied as products with their inverses, which the
// caller computes once and reuses for every solve with the same matrix; that
// is also where Unit / NonUnit is decided, so the kernels never look at a
// stored diagonal. y is a separate nb-vector: launch 1 may not overwrite x_k
// while other workgroups still read it.
//
// Which kernel runs depends on op alone:
//   op = N   the tiles of tile column k, (i, k): out[r] = sum_c T[r, c] v[c],
//            row-contiguous dot products reduced inside a wave (trsv_rowdot);
//   op = T/C the tiles of tile row k, (k, i): out[c] = sum_r op(T[r, c]) v[r],
//            column sums with the lanes along the contiguous dimension, the
//            rows split over the waves (and quarter waves) and combined
//            through LDS (trsv_colsum).
// Every output element is written by exactly one workgroup of a launch, in a
// fixed summation order; no workgroup waits on another, there are no atomics:
// two calls on the same data return the same bits.
//
// The identity padding of a partial last tile is not part of the matrix:
// rows and columns at or beyond n are never read into a sum and never
// written, so a zero tail of x stays zero whatever the padding holds.
// float and cplx<float> accumulate in double.

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vec_acc.h"

namespace {

constexpr int kRdThreads = 256;
constexpr int kRdWaves = kRdThreads / 64;
constexpr int kRdRowsPerWave = 2;
constexpr int kRdSegs = 4;  // row segments of 64 vectors loaded together
constexpr int kRdRows = kRdWaves * kRdRowsPerWave;  // rows per workgroup

constexpr int kCsThreads = 1024;
constexpr int kCsWaves = kCsThreads / 64;
constexpr int kCsSplit = 4;               // rows one wave load covers
constexpr int kCsLanes = 64 / kCsSplit;   // lanes along a row
constexpr int kCsSlots = kCsWaves * kCsSplit;  // rows a workgroup load covers
constexpr int kCsBatch = 8;  // loads in flight per lane

using namespace dlaf::vecacc;

// One launch: out (+)= op(tile_t) v over ntiles tiles, tile t at
// tiles + t * tile_stride, its outputs at out[t * nb ...]. Indices at or
// beyond vvalid (of v) / ovalid (of out) are outside the matrix. The first
// cblocks workgroups instead copy v[0 : vvalid) to xk.
struct Step {
  long long tile_stride;
  long long ovalid;
  int ntiles, nb, vvalid;
  int assign;  // out = sum (else out -= sum)
  int conj;
  int cblocks;
};

template <typename S>
__device__ inline void copy_block(const S* v, S* xk, const Step& p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.vvalid) xk[i] = v[i];
}

template <typename S>
__device__ inline void put(S* out, long long i, typename Acc<S>::type s,
                           int assign) {
  out[i] = narrow<S>(assign ? s : widen(out[i]) - s);
}

// out[r] = sum_c T[r, c] v[c]: a workgroup owns kRdRows rows of one tile, the
// four waves four adjacent rows; a wave issues the loads of kRdSegs segments
// of 64 vectors of each of its rows before the first is consumed (one round
// trip to memory for a 512-wide f64 row, so that a step of the solve is not a
// chain of load latencies).
template <typename S, int V, bool ALIGNED>
__global__ __launch_bounds__(kRdThreads) void trsv_rowdot(
    const S* __restrict__ tiles, const S* v, S* out, S* xk, Step p) {
  using A = typename Acc<S>::type;
  if ((int)blockIdx.x < p.cblocks) {
    copy_block(v, xk, p);
    return;
  }
  const int b = blockIdx.x - p.cblocks;
  const int strips = (p.nb + kRdRows - 1) / kRdRows;
  const int t = b / strips, s = b % strips;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const S* tile = tiles + (long long)t * p.tile_stride;
  const long long obase = (long long)t * p.nb;

  A acc[kRdRowsPerWave];
#pragma unroll
  for (int j = 0; j < kRdRowsPerWave; ++j) acc[j] = ScalarTraits<A>::zero();

  for (int c0 = 0; c0 < p.vvalid; c0 += 64 * V * kRdSegs) {
    // ALIGNED: c and nb are multiples of V, so c < vvalid <= nb keeps the
    // whole vector inside the tile row
    Vec<S, V> xs[kRdRowsPerWave][kRdSegs];
#pragma unroll
    for (int j = 0; j < kRdRowsPerWave; ++j) {
      const int r = s * kRdRows + wave + kRdWaves * j;
      const bool rowok = r < p.nb && obase + r < p.ovalid;  // wave-uniform
#pragma unroll
      for (int g = 0; g < kRdSegs; ++g) {
        const int c = c0 + (g * 64 + lane) * V;
        if (rowok && c < p.vvalid)
          load_vec<S, V, ALIGNED>(xs[j][g], tile + (long long)r * p.nb + c, c,
                                  p.vvalid);
      }
    }
#pragma unroll
    for (int g = 0; g < kRdSegs; ++g) {
      const int c = c0 + (g * 64 + lane) * V;
      A vv[V];
#pragma unroll
      for (int k = 0; k < V; ++k)
        vv[k] = c + k < p.vvalid ? widen(v[c + k]) : ScalarTraits<A>::zero();
#pragma unroll
      for (int j = 0; j < kRdRowsPerWave; ++j) {
        const int r = s * kRdRows + wave + kRdWaves * j;
        const bool rowok = r < p.nb && obase + r < p.ovalid;
        if (!rowok) continue;
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (c + k < p.vvalid) acc[j] += widen(xs[j][g].v[k]) * vv[k];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kRdRowsPerWave; ++j) {
    const int r = s * kRdRows + wave + kRdWaves * j;
    const bool rowok = r < p.nb && obase + r < p.ovalid;
    const A sum = wave_sum(acc[j]);
    if (lane == 0 && rowok) put(out, obase + r, sum, p.assign);
  }
}

// out[c] = sum_r op(T[r, c]) v[r]: a workgroup owns a block of kCsLanes * V
// columns of one tile (narrow, so that a tile row of the matrix gives enough
// workgroups to fill the chip: only columns can be split without two writers
// per output). A wave load covers kCsSplit rows, kCsLanes lanes along each;
// the workgroup's kCsSlots row slots take rows slot, slot + kCsSlots, ...,
// and their partial column sums are added through LDS in slot order.
template <typename S, int V, bool ALIGNED>
__global__ __launch_bounds__(kCsThreads) void trsv_colsum(
    const S* __restrict__ tiles, const S* v, S* out, S* xk, Step p) {
  using A = typename Acc<S>::type;
  constexpr int kBlockCols = kCsLanes * V;
  __shared__ A part[kCsSlots][kBlockCols];
  if ((int)blockIdx.x < p.cblocks) {
    copy_block(v, xk, p);
    return;
  }
  const int b = blockIdx.x - p.cblocks;
  const int cbs = (p.nb + kBlockCols - 1) / kBlockCols;
  const int t = b / cbs, cb = b % cbs;
  const int lane = threadIdx.x & 63;
  const int slot = (threadIdx.x >> 6) * kCsSplit + lane / kCsLanes;
  const int l = lane % kCsLanes;
  const S* tile = tiles + (long long)t * p.tile_stride;
  const long long obase = (long long)t * p.nb;
  const int c = cb * kBlockCols + l * V;
  const bool has = c < p.nb;  // ALIGNED: nb % V == 0, the vector fits

  A acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = ScalarTraits<A>::zero();

  for (int r0 = 0; r0 < p.vvalid; r0 += kCsSlots * kCsBatch) {
    Vec<S, V> xs[kCsBatch];
#pragma unroll
    for (int j = 0; j < kCsBatch; ++j) {
      const int r = r0 + slot + kCsSlots * j;
      if (r < p.vvalid && has)
        load_vec<S, V, ALIGNED>(xs[j], tile + (long long)r * p.nb + c, c,
                                p.nb);
    }
#pragma unroll
    for (int j = 0; j < kCsBatch; ++j) {
      const int r = r0 + slot + kCsSlots * j;
      if (!(r < p.vvalid && has)) continue;
      const A vr = widen(v[r]);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (!ALIGNED && c + k >= p.nb) continue;
        A a = widen(xs[j].v[k]);
        if (p.conj) a = ScalarTraits<A>::conj(a);
        acc[k] += a * vr;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) part[slot][l * V + k] = acc[k];
  __syncthreads();
  const int i = threadIdx.x;
  const int col = cb * kBlockCols + i;
  if (i < kBlockCols && col < p.nb && obase + col < p.ovalid) {
    A sum = part[0][i];
#pragma unroll 8
    for (int w = 1; w < kCsSlots; ++w) sum += part[w][i];
    put(out, obase + col, sum, p.assign);
  }
}

template <typename S>
void launch(bool trans, bool vec, const S* tiles, const S* v, S* out, S* xk,
            const Step& p, hipStream_t stream) {
  constexpr int V = 16 / sizeof(S) > 1 ? 16 / sizeof(S) : 1;
  const int per_tile = trans ? (p.nb + kCsLanes * V - 1) / (kCsLanes * V)
                             : (p.nb + kRdRows - 1) / kRdRows;
  const unsigned grid = p.cblocks + p.ntiles * per_tile;
  if (trans) {
    if (vec)
      trsv_colsum<S, V, true>
          <<<grid, kCsThreads, 0, stream>>>(tiles, v, out, xk, p);
    else
      trsv_colsum<S, V, false>
          <<<grid, kCsThreads, 0, stream>>>(tiles, v, out, xk, p);
  } else {
    if (vec)
      trsv_rowdot<S, V, true>
          <<<grid, kRdThreads, 0, stream>>>(tiles, v, out, xk, p);
    else
      trsv_rowdot<S, V, false>
          <<<grid, kRdThreads, 0, stream>>>(tiles, v, out, xk, p);
  }
}

}  // namespace

template <typename S>
void dlaf::trsv_tiles(const S* a, const S* dinv, S* x, S* work, int nt, int nb,
                      int64_t n, int uplo, int op, hipStream_t stream) {
  if (nt <= 0 || n <= 0) return;
  const bool trans = op != OP_N;
  const bool lower = uplo == 0;
  const bool forward = lower != trans;  // op(T) is lower triangular
  const long long tile = (long long)nb * nb;
  // 16-byte loads when every row of every tile starts on a 16-byte boundary
  constexpr int V = 16 / sizeof(S) > 1 ? 16 / sizeof(S) : 1;
  const bool vec = nb % V == 0 &&
                   reinterpret_cast<uintptr_t>(a) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(dinv) % 16 == 0;
  for (int s = 0; s < nt; ++s) {
    const int k = forward ? s : nt - 1 - s;
    const long long left = n - (long long)k * nb;  // rows from tile k on
    if (left <= 0) continue;
    Step p;
    p.nb = nb;
    p.vvalid = (int)(left < nb ? left : nb);
    p.conj = op == OP_C;
    // y = op(Dinv_k) x_k
    p.tile_stride = 0;
    p.ntiles = 1;
    p.ovalid = p.vvalid;
    p.assign = 1;
    p.cblocks = 0;
    launch(trans, vec, dinv + k * tile, x + (long long)k * nb, work,
           (S*)nullptr, p, stream);
    // x_i -= op(T)_ik y for the remaining i; x_k = y
    const int i0 = forward ? k + 1 : 0;
    p.ntiles = forward ? nt - 1 - k : k;
    p.ovalid = n - (long long)i0 * nb;
    if (p.ovalid <= 0) p.ntiles = 0;
    p.assign = 0;
    const int cthreads = trans ? kCsThreads : kRdThreads;
    p.cblocks = (p.vvalid + cthreads - 1) / cthreads;
    // op = N walks tile column k, (i, k); op = T/C tile row k, (k, i)
    p.tile_stride = trans ? tile : (long long)nt * tile;
    const S* first = a;
    S* out = x;
    if (p.ntiles > 0) {
      first += (trans ? (long long)k * nt + i0 : (long long)i0 * nt + k) * tile;
      out += (long long)i0 * nb;
    }
    launch(trans, vec, first, work, out, x + (long long)k * nb, p, stream);
  }
}

#define DLAF_INSTANTIATE_TRSV(S)                                              \
  template void dlaf::trsv_tiles<S>(const S*, const S*, S*, S*, int, int,     \
                                    int64_t, int, int, hipStream_t);
DLAF_INSTANTIATE_TRSV(float)
DLAF_INSTANTIATE_TRSV(double)
DLAF_INSTANTIATE_TRSV(cplx<float>)
DLAF_INSTANTIATE_TRSV(cplx<double>)
