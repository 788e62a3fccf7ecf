// Matrix norms of a rank's local tile storage: max |a|, per-row and per-column
// absolute sums and the sum of squares, all from ONE memory-bound pass.
//
// Storage is [tiles_r, tiles_c, mb, nb], contiguous row-major tiles. Partial
// edge tiles are padded with the identity extension, which is not part of the
// matrix: every element is masked by its GLOBAL (row, col) against (m, n), and
// by the structure (general / hermitian / triangular, Lower / Upper).
//
// Pass 1 (norms_partial): one 256-thread workgroup per (tile, strip of kRows
// rows). A wave reads one row segment of 64 vectors (1 KiB with 16-byte
// loads), the four waves four adjacent rows; the workgroup walks the strip's
// column blocks left to right. A lane keeps its VEC column sums for the
// current column block and one row sum per row it owns (kRows / 4, in
// registers across the column blocks), plus max and the sum-of-squares
// accumulators. The loads of kBatch rows are issued before the first is
// consumed (8 KiB in flight per wave); a row segment that lies wholly inside
// the matrix and strictly inside the triangle takes a path without masks.
// Column sums are combined across the four waves through LDS,
// row sums and scalars across the lanes by xor-butterflies: every order is
// fixed. Each workgroup STORES its partials (zeros included, so the workspace
// needs no clearing):
//   rowpart  [tiles_c]            [tiles_r * mb]
//   colpart  [tiles_r * strips]   [tiles_c * nb]
//   scalpart [workgroups]         [4]   (max, small, medium, big)
// Pass 2 (norms_combine) sums the partials per destination in index order.
// No floating-point atomics anywhere: two calls on the same data return the
// same bits.
//
// Sum of squares: Blue's three accumulators with LAPACK 3.10's constants for
// double (values above 2^486 are scaled by 2^-538, values below 2^-511 by
// 2^537, before squaring). float inputs are squared in double, where neither
// overflow nor underflow can happen, and use the medium accumulator alone.
// NaN propagates through every sum; max, taken with fmax (which drops NaN),
// gets it back from the sums in norms_combine.

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = dlaf::kNormStripRows;  // rows per workgroup strip
constexpr int kRowsPerLane = kRows / kWaves;
constexpr int kBatch = 8;  // rows whose loads are in flight together

constexpr int kGeneral = 0, kHermitian = 1, kTriangular = 2;
constexpr int kLower = 0;

// LAPACK la_constants (double): thresholds and scalings of Blue's algorithm
constexpr double kTsml = 0x1p-511, kTbig = 0x1p486;
constexpr double kSsml = 0x1p537, kSbig = 0x1p-538;

template <typename S, int V>
struct alignas(V > 1 ? sizeof(S) * V : alignof(S)) Vec {
  S v[V];
};

struct Geom {
  int tiles_r, tiles_c, mb, nb;
  long long m, n;
  int gr0, grs, gc0, gcs;  // global tile index of local tile l: g0 + l * gs
  int structure, uplo, unit_diag;
  int strips;  // row strips per tile
};

template <typename R>
struct SumSq {
  double sml = 0, med = 0, big = 0;
  // add w * ax^2, ax >= 0 (or NaN), w = 1 or 2. Values outside Blue's medium
  // range are rare: one test sends them to the scaled accumulators, zero and
  // NaN stay on the medium one.
  __device__ inline void add(double ax, double w) {
    if constexpr (sizeof(R) == 4) {
      med += w * (ax * ax);
    } else {
      if (__builtin_expect((ax > kTbig) | ((ax < kTsml) & (ax > 0.0)), 0)) {
        const double t = ax * (ax > kTbig ? kSbig : kSsml);
        (ax > kTbig ? big : sml) += w * (t * t);
      } else {
        med += w * (ax * ax);
      }
    }
  }
};

// |x| and the real parts whose squares make |x|^2
template <typename T>
__device__ inline double abs_of(T x) {
  return fabs((double)x);
}
__device__ inline double abs_of(cplx<float> x) {
  const double re = x.re, im = x.im;
  return sqrt(re * re + im * im);  // float squares are safe in double
}
__device__ inline double abs_of(cplx<double> x) {
  // the plain formula where the squares can neither overflow nor lose bits
  const double s = x.re * x.re + x.im * x.im;
  return (s > 0x1p-900 && s < 0x1p900) ? sqrt(s) : hypot(x.re, x.im);
}

template <typename T>
__device__ inline double re_of(T x) {
  return fabs((double)x);
}
template <typename T>
__device__ inline double re_of(cplx<T> x) {
  return fabs((double)x.re);
}
template <typename R, typename T>
__device__ inline void add_sq(SumSq<R>& s, T x, double w) {
  s.add(fabs((double)x), w);
}
template <typename R, typename T>
__device__ inline void add_sq(SumSq<R>& s, cplx<T> x, double w) {
  s.add(fabs((double)x.re), w);
  s.add(fabs((double)x.im), w);
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// fmax drops a NaN: the sums keep it, and norms_combine puts it back
__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename S, int V>
__global__ __launch_bounds__(kThreads) void norms_partial(
    const S* __restrict__ a, Geom g, long long wg0,
    double* __restrict__ rowpart, double* __restrict__ colpart,
    double* __restrict__ scalpart) {
  using R = typename ScalarTraits<S>::real_t;
  constexpr int kBlockCols = 64 * V;  // columns per column block
  __shared__ double scol[kWaves][kBlockCols];
  __shared__ double sscal[kWaves][4];

  const int lane = threadIdx.x & 63;
  // the wave index through readfirstlane, so that everything derived from it
  // (rows, their masks, tile addresses) is scalar and branches are uniform
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long wg = wg0 + blockIdx.x;  // wg0: first workgroup of this launch
  const int rb = (int)(wg % g.strips);
  const int lj = (int)((wg / g.strips) % g.tiles_c);
  const int li = (int)(wg / ((long long)g.strips * g.tiles_c));
  const long long grow0 = (long long)(g.gr0 + li * g.grs) * g.mb;
  const long long gcol0 = (long long)(g.gc0 + lj * g.gcs) * g.nb;
  const S* tile = a + ((long long)li * g.tiles_c + lj) * g.mb * g.nb;

  const long long lrows = (long long)g.tiles_r * g.mb;
  const long long lcols = (long long)g.tiles_c * g.nb;
  double* colout = colpart + ((long long)li * g.strips + rb) * lcols +
                   (long long)lj * g.nb;

  double rowp[kRowsPerLane];
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) rowp[i] = 0;
  double vmax = 0;
  SumSq<R> ss;

  for (int c0 = 0; c0 < g.nb; c0 += kBlockCols) {
    const int c = c0 + lane * V;
    double colacc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) colacc[k] = 0;
    const long long gcf = gcol0 + c0;                  // first column
    const long long gcl = gcf + kBlockCols - 1;        // last column
    // issue the loads of kBatch of the lane's rows before any is consumed:
    // one 16-byte load in flight per wave would leave the pass latency-bound
#pragma unroll
    for (int h = 0; h < kRowsPerLane; h += kBatch) {
      Vec<S, V> xs[kBatch];
      unsigned loaded = 0;
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int r = rb * kRows + wave + kWaves * (h + j);
        const long long gr = grow0 + r;
        // wave-uniform: nothing of this row segment is part of the matrix
        bool skip = r >= g.mb || gr >= g.m || gcf >= g.n;
        if (g.structure != kGeneral)
          skip = skip || (g.uplo == kLower ? gcf > gr : gcl < gr);
        if (skip || c >= g.nb) continue;
        xs[j] =
            *reinterpret_cast<const Vec<S, V>*>(tile + (long long)r * g.nb + c);
        loaded |= 1u << j;
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        if (!(loaded >> j & 1)) continue;
        const int i = h + j;
        const long long gr = grow0 + rb * kRows + wave + kWaves * i;
        const Vec<S, V>& x = xs[j];
        // wave-uniform: the whole segment is inside the matrix and strictly
        // inside the triangle, so no element needs a mask or is on the diagonal
        bool interior = gcl < g.n && c0 + kBlockCols <= g.nb;
        if (g.structure != kGeneral)
          interior = interior && (g.uplo == kLower ? gcl < gr : gcf > gr);
        if (interior) {
          const double w = g.structure == kHermitian ? 2.0 : 1.0;
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const double v = abs_of(x.v[k]);
            vmax = fmax(vmax, v);
            colacc[k] += v;
            rowp[i] += v;
            add_sq(ss, x.v[k], w);
          }
          continue;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const long long gc = gcol0 + c + k;
          bool in = gc < g.n && c + k < g.nb;
          if (g.structure != kGeneral)
            in = in && (g.uplo == kLower ? gc <= gr : gc >= gr);
          if (!in) continue;
          const bool diag = gc == gr;
          if (diag && g.structure == kTriangular && g.unit_diag) {
            vmax = fmax(vmax, 1.0);
            colacc[k] += 1.0;
            rowp[i] += 1.0;
            ss.add(1.0, 1.0);
          } else if (diag && g.structure == kHermitian) {
            // |Re a_ii|; counted once, in the column sum
            const double v = re_of(x.v[k]);
            vmax = fmax(vmax, v);
            colacc[k] += v;
            ss.add(v, 1.0);
          } else {
            const double v = abs_of(x.v[k]);
            vmax = fmax(vmax, v);
            colacc[k] += v;
            rowp[i] += v;
            add_sq(ss, x.v[k], g.structure == kHermitian ? 2.0 : 1.0);
          }
        }
      }
    }
    // column sums of this block: the four waves in wave order
    __syncthreads();  // previous block's scol fully read
#pragma unroll
    for (int k = 0; k < V; ++k) scol[wave][lane * V + k] = colacc[k];
    __syncthreads();
    for (int t = threadIdx.x; t < kBlockCols; t += kThreads) {
      if (c0 + t < g.nb) {
        double s = scol[0][t];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += scol[w][t];
        colout[c0 + t] = s;
      }
    }
  }

  // row sums: across the lanes of the wave that owns the row
  double* rowout = rowpart + (long long)lj * lrows + (long long)li * g.mb;
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) {
    const int r = rb * kRows + wave + kWaves * i;
    const double s = wave_sum(rowp[i]);
    if (lane == 0 && r < g.mb) rowout[r] = s;
  }

  // scalars: lanes, then the four waves in wave order
  vmax = wave_max(vmax);
  const double sml = wave_sum(ss.sml), med = wave_sum(ss.med),
               big = wave_sum(ss.big);
  if (lane == 0) {
    sscal[wave][0] = vmax;
    sscal[wave][1] = sml;
    sscal[wave][2] = med;
    sscal[wave][3] = big;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double o0 = sscal[0][0], o1 = sscal[0][1], o2 = sscal[0][2],
           o3 = sscal[0][3];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      o0 = fmax(o0, sscal[w][0]);
      o1 += sscal[w][1];
      o2 += sscal[w][2];
      o3 += sscal[w][3];
    }
    double* o = scalpart + wg * 4;
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
    o[3] = o3;
  }
}

// Sum the stored partials per destination, in index order. Blocks
// [0, rblocks) take local rows, [rblocks, rblocks + cblocks) local columns,
// the last block the four scalars.
__global__ __launch_bounds__(kThreads) void norms_combine(
    Geom g, long long nwg, int rblocks, int cblocks,
    const double* __restrict__ rowpart, const double* __restrict__ colpart,
    const double* __restrict__ scalpart, double* __restrict__ rows,
    double* __restrict__ cols, double* __restrict__ scal) {
  const long long lrows = (long long)g.tiles_r * g.mb;
  const long long lcols = (long long)g.tiles_c * g.nb;
  const int b = blockIdx.x;
  if (b < rblocks) {
    const long long r = (long long)b * kThreads + threadIdx.x;
    if (r >= lrows) return;
    double s = 0;
    for (int k = 0; k < g.tiles_c; ++k) s += rowpart[k * lrows + r];
    rows[r] = s;
    return;
  }
  if (b < rblocks + cblocks) {
    const long long c = (long long)(b - rblocks) * kThreads + threadIdx.x;
    if (c >= lcols) return;
    double s = 0;
    const long long parts = (long long)g.tiles_r * g.strips;
    for (long long k = 0; k < parts; ++k) s += colpart[k * lcols + c];
    cols[c] = s;
    return;
  }
  __shared__ double sh[kThreads][4];
  double o0 = 0, o1 = 0, o2 = 0, o3 = 0;
  for (long long k = threadIdx.x; k < nwg; k += kThreads) {
    o0 = fmax(o0, scalpart[k * 4 + 0]);
    o1 += scalpart[k * 4 + 1];
    o2 += scalpart[k * 4 + 2];
    o3 += scalpart[k * 4 + 3];
  }
  sh[threadIdx.x][0] = o0;
  sh[threadIdx.x][1] = o1;
  sh[threadIdx.x][2] = o2;
  sh[threadIdx.x][3] = o3;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[threadIdx.x][0] = fmax(sh[threadIdx.x][0], sh[threadIdx.x + s][0]);
      sh[threadIdx.x][1] += sh[threadIdx.x + s][1];
      sh[threadIdx.x][2] += sh[threadIdx.x + s][2];
      sh[threadIdx.x][3] += sh[threadIdx.x + s][3];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // a NaN element is in the medium sum (and in no max): put it back
    const double sums = sh[0][1] + sh[0][2] + sh[0][3];
    scal[0] = sums != sums ? sums : sh[0][0];
    scal[1] = sh[0][1];
    scal[2] = sh[0][2];
    scal[3] = sh[0][3];
  }
}

}  // namespace

int64_t dlaf::matrix_norms_work_size(int tiles_r, int tiles_c, int mb, int nb) {
  const int64_t strips = (mb + kRows - 1) / kRows;
  const int64_t lrows = (int64_t)tiles_r * mb, lcols = (int64_t)tiles_c * nb;
  return tiles_c * lrows + tiles_r * strips * lcols +
         4 * (int64_t)tiles_r * tiles_c * strips;
}

template <typename S>
void dlaf::matrix_norms(const S* a, int tiles_r, int tiles_c, int mb, int nb,
                        int64_t m, int64_t n, int gr0, int grs, int gc0,
                        int gcs, int structure, int uplo, int unit_diag,
                        double* rows, double* cols, double* scal, double* work,
                        hipStream_t stream) {
  if (tiles_r <= 0 || tiles_c <= 0) return;
  Geom g;
  g.tiles_r = tiles_r;
  g.tiles_c = tiles_c;
  g.mb = mb;
  g.nb = nb;
  g.m = m;
  g.n = n;
  g.gr0 = gr0;
  g.grs = grs;
  g.gc0 = gc0;
  g.gcs = gcs;
  g.structure = structure;
  g.uplo = uplo;
  g.unit_diag = unit_diag;
  g.strips = (mb + kRows - 1) / kRows;
  const long long lrows = (long long)tiles_r * mb;
  const long long lcols = (long long)tiles_c * nb;
  const long long nwg = (long long)tiles_r * tiles_c * g.strips;
  double* rowpart = work;
  double* colpart = rowpart + tiles_c * lrows;
  double* scalpart = colpart + (long long)tiles_r * g.strips * lcols;

  // 16-byte loads when every row of every tile starts on a 16-byte boundary
  constexpr int V = 16 / sizeof(S) > 1 ? 16 / sizeof(S) : 1;
  const bool vec =
      V > 1 && nb % V == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0;
  // a launch is limited to 2^32 threads: at most kMaxLaunch workgroups each
  constexpr long long kMaxLaunch = 1LL << 23;
  for (long long wg0 = 0; wg0 < nwg; wg0 += kMaxLaunch) {
    const unsigned nblk = (unsigned)(nwg - wg0 < kMaxLaunch ? nwg - wg0
                                                             : kMaxLaunch);
    if (vec)
      norms_partial<S, V><<<nblk, kThreads, 0, stream>>>(
          a, g, wg0, rowpart, colpart, scalpart);
    else
      norms_partial<S, 1><<<nblk, kThreads, 0, stream>>>(
          a, g, wg0, rowpart, colpart, scalpart);
  }
  const int rblocks = (int)((lrows + kThreads - 1) / kThreads);
  const int cblocks = (int)((lcols + kThreads - 1) / kThreads);
  norms_combine<<<rblocks + cblocks + 1, kThreads, 0, stream>>>(
      g, nwg, rblocks, cblocks, rowpart, colpart, scalpart, rows, cols, scal);
}

#define DLAF_INSTANTIATE_NORMS(S)                                            \
  template void dlaf::matrix_norms<S>(const S*, int, int, int, int, int64_t, \
                                      int64_t, int, int, int, int, int, int, \
                                      int, double*, double*, double*,        \
                                      double*, hipStream_t);
DLAF_INSTANTIATE_NORMS(float)
DLAF_INSTANTIATE_NORMS(double)
DLAF_INSTANTIATE_NORMS(cplx<float>)
DLAF_INSTANTIATE_NORMS(cplx<double>)
