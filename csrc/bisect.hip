// Tridiagonal eigenvalues by Sturm-sequence bisection, one kernel launch.
//
// One THREAD per eigenvalue (tridiag_bisect) or per query point
// (sturm_count). One evaluation of the count is a serial chain of n
// dependent divisions, so the parallelism is across eigenvalues; 64-thread
// workgroups (one wave) spread n = 20000 over ~313 workgroups on 256 CUs.
// Every lane reads the same d[i], e2[i-1] at the same step: the workgroup
// stages them through LDS in kChunk-sized pieces with coalesced loads and the
// chain reads them back as LDS broadcasts. All lanes of a workgroup stay in
// the (uniform) bisection loop until the last lane has converged, so no
// barrier sits in divergent control flow; converged lanes and lanes past
// k_end keep staging and only skip their state update / final store.
// The recurrence and the bisection rule are the ones of sturm.h, shared with
// the host twins.

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "sturm.h"

namespace {

constexpr int kThreads = 64;
constexpr int kChunk = dlaf::kBisectChunk;
constexpr int kBatch = 8;  // recurrence steps per group of LDS reads

// Stage d[base .. base+len) and the shifted e2 (e2[i-1], 0 for i = 0).
__device__ inline void stage(const double* __restrict__ d,
                             const double* __restrict__ e2, int base, int len,
                             double* sd, double* se) {
  for (int j = threadIdx.x; j < len; j += kThreads) {
    const int i = base + j;
    sd[j] = d[i];
    se[j] = i ? e2[i - 1] : 0.0;
  }
}

// count(x) for this lane's x; uniform control flow (n is uniform).
// `resident` means the whole matrix (n <= kChunk) is already staged.
__device__ inline long long count_staged(const double* __restrict__ d,
                                         const double* __restrict__ e2, int n,
                                         double pivmin, double x, double* sd,
                                         double* se, bool resident) {
  long long cnt = 0;
  double q = 1.0;
  for (int base = 0; base < n; base += kChunk) {
    const int len = min(kChunk, n - base);
    if (!resident) {
      __syncthreads();  // previous chunk fully consumed
      stage(d, e2, base, len, sd, se);
      __syncthreads();
    }
    // the chain is serial, the LDS reads are not: fetch kBatch steps' worth
    // of operands ahead of the divisions that consume them
    int j = 0;
    for (; j + kBatch <= len; j += kBatch) {
      double dv[kBatch], ev[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        dv[u] = sd[j + u];
        ev[u] = se[j + u];
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        q = dlaf::sturm::step(q, dv[u], ev[u], x, pivmin, cnt);
    }
    for (; j < len; ++j)
      q = dlaf::sturm::step(q, sd[j], se[j], x, pivmin, cnt);
  }
  return cnt;
}

__global__ __launch_bounds__(kThreads) void bisect_kernel(
    const double* __restrict__ d, const double* __restrict__ e2, int n,
    int k_begin, int k_end, double gl, double gu, double pivmin,
    double* __restrict__ w) {
  __shared__ double sd[kChunk];
  __shared__ double se[kChunk];
  // k can pass k_end (and n) in the last workgroup: such a lane bisects
  // towards gu like any other and skips the store
  // (the bindings keep n < 2^30, so k does not overflow)
  const int k = k_begin + blockIdx.x * kThreads + threadIdx.x;
  const bool resident = n <= kChunk;
  if (resident) {
    stage(d, e2, 0, n, sd, se);
    __syncthreads();
  }
  dlaf::sturm::Bisect s;
  dlaf::sturm::bisect_begin(s, gl, gu, pivmin);
  while (__syncthreads_or(!s.done)) {
    const long long cnt =
        count_staged(d, e2, n, pivmin, s.mid, sd, se, resident);
    if (!s.done) dlaf::sturm::bisect_update(s, cnt, k, pivmin);
  }
  if (k < k_end) w[k - k_begin] = s.mid;
}

__global__ __launch_bounds__(kThreads) void count_kernel(
    const double* __restrict__ d, const double* __restrict__ e2, int n,
    double pivmin, const double* __restrict__ x, int nx,
    long long* __restrict__ count) {
  __shared__ double sd[kChunk];
  __shared__ double se[kChunk];
  const int j = blockIdx.x * kThreads + threadIdx.x;
  const double xj = j < nx ? x[j] : 0.0;
  const long long cnt = count_staged(d, e2, n, pivmin, xj, sd, se, false);
  if (j < nx) count[j] = cnt;
}

}  // namespace

void dlaf::tridiag_bisect(const double* d, const double* e2, int n,
                          int k_begin, int k_end, double gl, double gu,
                          double pivmin, double* w, hipStream_t stream) {
  if (n <= 0 || k_begin >= k_end) return;
  const int blocks = (k_end - k_begin + kThreads - 1) / kThreads;
  bisect_kernel<<<blocks, kThreads, 0, stream>>>(d, e2, n, k_begin, k_end, gl,
                                                 gu, pivmin, w);
}

void dlaf::sturm_count(const double* d, const double* e2, int n, double pivmin,
                       const double* x, int nx, long long* count,
                       hipStream_t stream) {
  if (nx <= 0) return;
  if (n <= 0) {
    (void)hipMemsetAsync(count, 0, sizeof(long long) * nx, stream);
    return;
  }
  const int blocks = (nx + kThreads - 1) / kThreads;
  count_kernel<<<blocks, kThreads, 0, stream>>>(d, e2, n, pivmin, x, nx,
                                                count);
}
