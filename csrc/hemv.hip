// Hermitian matrix-vector product over a local tile storage: y = A x and,
// from the same pass, yabs = |A| |x|, A the Hermitian matrix whose `uplo`
// triangle is stored in a [nt, nt, nb, nb] storage of row-major tiles (the
// layout norms.hip and trsv.hip walk). |.| is LAPACK's CABS1, |re| + |im|, so
// that yabs is the vector ?porfs builds for its backward error.
//
// The product is memory-bound and the triangle is read ONCE: a stored element
// a_rc off the diagonal serves y_r += a_rc x_c and y_c += conj(a_rc) x_r from
// the same registers; a diagonal element counts once, with its imaginary part
// taken as zero (as zhemv). The layout is the one of norms_partial, whose row
// sums and column sums are this kernel's two contributions with weights:
//
// Pass 1 (hemv_partial): one 256-thread workgroup per (stored tile, strip of
// kRows rows); tiles of the other triangle get no workgroup. A wave reads one
// row segment of 64 vectors (1 KiB with 16-byte loads), the four waves four
// adjacent rows; the workgroup walks the strip's column blocks left to right.
// A lane keeps its V column sums for the current column block and one row sum
// per row it owns (kRows / 4, in registers across the column blocks). The
// loads of kBatch rows are issued before the first is consumed. Column sums
// are combined across the four waves through LDS in wave order, row sums
// across the lanes by a xor-butterfly: every order is fixed. Each workgroup
// STORES its partials, zeros included, so the workspace needs no clearing:
//   part [nt + nt * strips] [nt * nb]
//     part lj                    rows of tile row li at [li * nb ...]
//     part nt + li * strips + rb columns of tile column lj at [lj * nb ...]
// as accumulator values (double or cplx<double>), followed by the same
// layout in double for |A| |x|.
// Pass 2 (hemv_combine): one thread per output element sums the partials that
// pass 1 wrote for it (those of the stored tiles of its tile row and tile
// column), in index order, and rounds once.
// No atomics, one writer per element, no workgroup waits on another: two
// calls on the same data return the same bits.
//
// The identity padding of a partial last tile is not part of the matrix: rows
// and columns at or beyond n are never read into a sum, and y / yabs are
// never written there. float and cplx<float> accumulate in double.
//
// 16-byte loads need nb % V == 0 and a 16-byte aligned base; otherwise the
// same lanes take the same elements by guarded scalar loads, so both paths
// sum in the same order and return the same bits.

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "vec_acc.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = dlaf::kHemvStripRows;  // rows per workgroup strip
constexpr int kRowsPerLane = kRows / kWaves;
constexpr int kBatch = 8;  // rows whose loads are in flight together

using namespace dlaf::vecacc;

__device__ inline double cabs1(double x) { return fabs(x); }
__device__ inline double cabs1(cplx<double> x) {
  return fabs(x.re) + fabs(x.im);
}
// a stored diagonal element: its real part
__device__ inline double real_only(double x) { return x; }
__device__ inline cplx<double> real_only(cplx<double> x) {
  return {x.re, 0.0};
}

struct Geom {
  int nt, nb, upper, strips;
  int n;  // nt * nb < 2^31
};

template <typename S, int V, bool ALIGNED, bool ABS>
__global__ __launch_bounds__(kThreads) void hemv_partial(
    const S* __restrict__ a, const S* __restrict__ x, Geom g,
    typename Acc<S>::type* __restrict__ part, double* __restrict__ apart) {
  using A = typename Acc<S>::type;
  constexpr int kBlockCols = 64 * V;  // columns per column block
  __shared__ A scol[kWaves][kBlockCols];
  __shared__ double sabs[ABS ? kWaves : 1][kBlockCols];

  const int lane = threadIdx.x & 63;
  // through readfirstlane, so that rows, their masks and addresses are scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rb = blockIdx.x % g.strips;
  // stored tile t of the triangle: (hi, lo), lo <= hi, row by row
  const int t = blockIdx.x / g.strips;
  int hi = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((hi + 1) * (hi + 2) / 2 <= t) ++hi;
  while (hi * (hi + 1) / 2 > t) --hi;
  const int lo = t - hi * (hi + 1) / 2;
  const int li = g.upper ? lo : hi, lj = g.upper ? hi : lo;
  const int grow0 = li * g.nb, gcol0 = lj * g.nb;
  const S* tile = a + ((long long)li * g.nt + lj) * g.nb * g.nb;
  const long long len = (long long)g.nt * g.nb;
  const long long rowoff = (long long)lj * len + grow0;
  const long long coloff =
      (long long)(g.nt + li * g.strips + rb) * len + gcol0;

  A rowp[kRowsPerLane];
  double rowa[kRowsPerLane];
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) {
    rowp[i] = ScalarTraits<A>::zero();
    rowa[i] = 0;
  }

  for (int c0 = 0; c0 < g.nb; c0 += kBlockCols) {
    const int c = c0 + lane * V;
    A colacc[V], xc[V];
    double cola[V], axc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      colacc[k] = ScalarTraits<A>::zero();
      cola[k] = 0;
      // x of this lane's columns; the tail beyond n is loaded but never used
      xc[k] = c + k < g.nb ? widen(x[gcol0 + c + k]) : ScalarTraits<A>::zero();
      axc[k] = cabs1(xc[k]);
    }
    const int gcf = gcol0 + c0;             // first column
    const int gcl = gcf + kBlockCols - 1;   // last column
#pragma unroll
    for (int h = 0; h < kRowsPerLane; h += kBatch) {
      Vec<S, V> xs[kBatch];
      unsigned loaded = 0;
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int r = rb * kRows + wave + kWaves * (h + j);
        const int gr = grow0 + r;
        // wave-uniform: nothing of this row segment is in the stored triangle
        const bool skip = r >= g.nb || gr >= g.n || gcf >= g.n ||
                          (g.upper ? gcl < gr : gcf > gr);
        if (skip || c >= g.nb) continue;
        load_vec<S, V, ALIGNED>(xs[j], tile + (long long)r * g.nb + c, c,
                                g.nb);
        loaded |= 1u << j;
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        if (!(loaded >> j & 1)) continue;
        const int i = h + j;
        const int gr = grow0 + rb * kRows + wave + kWaves * i;
        const A xr = widen(x[gr]);  // gr < n: the row was not skipped
        const double axr = cabs1(xr);
        // wave-uniform: the whole segment is inside the matrix and strictly
        // inside the triangle
        const bool interior = gcl < g.n && c0 + kBlockCols <= g.nb &&
                              (g.upper ? gcf > gr : gcl < gr);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const int gc = gcol0 + c + k;
          if (!interior) {
            const bool in = gc < g.n && c + k < g.nb &&
                            (g.upper ? gc >= gr : gc <= gr);
            if (!in) continue;
            if (gc == gr) {
              const A d = real_only(widen(xs[j].v[k]));
              rowp[i] += d * xc[k];
              if constexpr (ABS) rowa[i] += cabs1(d) * axc[k];
              continue;
            }
          }
          const A v = widen(xs[j].v[k]);
          rowp[i] += v * xc[k];
          colacc[k] += ScalarTraits<A>::conj(v) * xr;
          if constexpr (ABS) {
            const double av = cabs1(v);
            rowa[i] += av * axc[k];
            cola[k] += av * axr;
          }
        }
      }
    }
    // column sums of this block: the four waves in wave order
    __syncthreads();  // previous block's scol fully read
#pragma unroll
    for (int k = 0; k < V; ++k) {
      scol[wave][lane * V + k] = colacc[k];
      if constexpr (ABS) sabs[wave][lane * V + k] = cola[k];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < kBlockCols; q += kThreads) {
      if (c0 + q < g.nb) {
        A s = scol[0][q];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += scol[w][q];
        part[coloff + c0 + q] = s;
        if constexpr (ABS) {
          double sa = sabs[0][q];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) sa += sabs[w][q];
          apart[coloff + c0 + q] = sa;
        }
      }
    }
  }

  // row sums: across the lanes of the wave that owns the row
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) {
    const int r = rb * kRows + wave + kWaves * i;
    const A s = wave_sum(rowp[i]);
    double sa = 0;
    if constexpr (ABS) sa = wave_sum(rowa[i]);
    if (lane == 0 && r < g.nb) {
      part[rowoff + r] = s;
      if constexpr (ABS) apart[rowoff + r] = sa;
    }
  }
}

// y[k] (and yabs[k]), k < n: the partials of the stored tiles of tile row
// k / nb, then those of tile column k / nb, in index order.
template <typename S, bool ABS>
__global__ __launch_bounds__(kThreads) void hemv_combine(
    Geom g, const typename Acc<S>::type* __restrict__ part,
    const double* __restrict__ apart, S* __restrict__ y,
    typename ScalarTraits<S>::real_t* __restrict__ yabs) {
  using A = typename Acc<S>::type;
  using R = typename ScalarTraits<S>::real_t;
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= g.n) return;
  const int b = (int)(k / g.nb);
  const long long len = (long long)g.nt * g.nb;
  A s = ScalarTraits<A>::zero();
  double sa = 0;
  // tile row b holds the stored tiles (b, lj): lj <= b (Lower), lj >= b
  const int j0 = g.upper ? b : 0, j1 = g.upper ? g.nt - 1 : b;
  for (int lj = j0; lj <= j1; ++lj) {
    s += part[lj * len + k];
    if constexpr (ABS) sa += apart[lj * len + k];
  }
  // tile column b the stored tiles (li, b): li >= b (Lower), li <= b
  const int i0 = g.upper ? 0 : b, i1 = g.upper ? b : g.nt - 1;
  for (long long p = (long long)i0 * g.strips;
       p < (long long)(i1 + 1) * g.strips; ++p) {
    s += part[(g.nt + p) * len + k];
    if constexpr (ABS) sa += apart[(g.nt + p) * len + k];
  }
  y[k] = narrow<S>(s);
  if constexpr (ABS) yabs[k] = (R)sa;
}

template <typename S, int V, bool ALIGNED>
void launch(const S* a, const S* x, S* y,
            typename ScalarTraits<S>::real_t* yabs, const Geom& g,
            double* work, hipStream_t stream) {
  using A = typename Acc<S>::type;
  const long long parts = (long long)g.nt + (long long)g.nt * g.strips;
  const long long len = (long long)g.nt * g.nb;
  A* part = reinterpret_cast<A*>(work);
  double* apart = work + parts * len * (long long)(sizeof(A) / sizeof(double));
  const unsigned nwg = (unsigned)((long long)g.nt * (g.nt + 1) / 2 * g.strips);
  const unsigned cblocks = (unsigned)((g.n + kThreads - 1) / kThreads);
  if (yabs) {
    hemv_partial<S, V, ALIGNED, true>
        <<<nwg, kThreads, 0, stream>>>(a, x, g, part, apart);
    hemv_combine<S, true>
        <<<cblocks, kThreads, 0, stream>>>(g, part, apart, y, yabs);
  } else {
    hemv_partial<S, V, ALIGNED, false>
        <<<nwg, kThreads, 0, stream>>>(a, x, g, part, apart);
    hemv_combine<S, false>
        <<<cblocks, kThreads, 0, stream>>>(g, part, apart, y, yabs);
  }
}

}  // namespace

int64_t dlaf::hemv_work_size(int nt, int nb) {
  const int64_t strips = (nb + kRows - 1) / kRows;
  // y partials as (re, im) and |A| |x| partials, for any dtype
  return 3 * (nt + nt * strips) * ((int64_t)nt * nb);
}

template <typename S>
void dlaf::hemv_tiles(const S* a, const S* x, S* y,
                      typename ScalarTraits<S>::real_t* yabs, int nt, int nb,
                      int64_t n, int uplo, double* work, hipStream_t stream) {
  if (nt <= 0 || n <= 0) return;
  Geom g;
  g.nt = nt;
  g.nb = nb;
  g.upper = uplo != 0;
  g.strips = (nb + kRows - 1) / kRows;
  g.n = (int)n;
  constexpr int V = 16 / sizeof(S) > 1 ? 16 / sizeof(S) : 1;
  if constexpr (V > 1) {
    // 16-byte loads when every row of every tile starts on a 16-byte boundary
    if (nb % V == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0)
      launch<S, V, true>(a, x, y, yabs, g, work, stream);
    else
      launch<S, V, false>(a, x, y, yabs, g, work, stream);
  } else {
    launch<S, 1, true>(a, x, y, yabs, g, work, stream);
  }
}

#define DLAF_INSTANTIATE_HEMV(S)                                             \
  template void dlaf::hemv_tiles<S>(const S*, const S*, S*,                  \
                                    typename ScalarTraits<S>::real_t*, int,  \
                                    int, int64_t, int, double*, hipStream_t);
DLAF_INSTANTIATE_HEMV(float)
DLAF_INSTANTIATE_HEMV(double)
DLAF_INSTANTIATE_HEMV(cplx<float>)
DLAF_INSTANTIATE_HEMV(cplx<double>)
