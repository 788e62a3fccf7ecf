// Shifted tridiagonal solves for inverse iteration, one kernel launch:
// (T - lam[j] I) y_j = x_j for k columns at once, in place on X.
//
// One THREAD per column. One solve is a serial chain of n dependent
// divisions forward and n backward (tridiag_lu.h), so the parallelism is
// across columns; 64-thread workgroups (one wave). X is [n, k] row-major, so
// lane j of step i touches X[i*ldx + j]: every load and store of a wave is
// one contiguous 512-byte row piece. The U rows go to a [3, n, cols]
// workspace with the same interleaving: the forward sweep writes them, the
// back substitution reads them (and needs nothing else, so only the forward
// sweep stages d/e). Every lane reads the same d[i+1], e[i], e[i+1] at the
// same step: the workgroup stages them through LDS in kBisectChunk pieces
// with coalesced loads and the chain reads them back as LDS broadcasts. The
// loops over i are uniform, so no barrier sits in divergent control flow;
// lanes past k keep staging and computing and only skip their loads and
// stores. The chain is latency-bound, the memory operations are not: both
// sweeps fetch kBatch steps' worth of operands ahead of the divisions that
// consume them.

#include <hip/hip_runtime.h>

#include "kernels.h"
#include "tridiag_lu.h"

namespace {

constexpr int kThreads = 64;
constexpr int kChunk = dlaf::kBisectChunk;
constexpr int kBatch = 8;  // chain steps per group of loads

__global__ __launch_bounds__(kThreads) void shifted_solve_kernel(
    const double* __restrict__ d, const double* __restrict__ e, int n,
    const double* __restrict__ lam, int k, double tol, double* __restrict__ X,
    long long ldx, double* __restrict__ U, long long cols) {
  // step i uses d[i+1], e[i], e[i+1]; entries past the end are 0 (the last
  // step pairs the working row with a zero row)
  __shared__ double sd[kChunk];      // sd[j] = d[base + j + 1]
  __shared__ double se[kChunk + 1];  // se[j] = e[base + j]
  const long long col = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool live = col < k;
  const double shift = live ? lam[col] : 0.0;
  double* __restrict__ xc = X + col;
  const long long plane = (long long)n * cols;
  double* __restrict__ uc = U + col;

  double a = d[0] - shift;
  double b = n > 1 ? e[0] : 0.0;
  double xcur = live ? xc[0] : 0.0;
  for (int base = 0; base < n; base += kChunk) {
    const int len = min(kChunk, n - base);
    __syncthreads();  // previous chunk fully consumed
    for (int j = threadIdx.x; j <= len; j += kThreads) {
      const int i = base + j;
      if (j < len) sd[j] = i + 1 < n ? d[i + 1] : 0.0;
      se[j] = i < n - 1 ? e[i] : 0.0;
    }
    __syncthreads();
    for (int j0 = 0; j0 < len; j0 += kBatch) {
      const int nb = min(kBatch, len - j0);
      double xn[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const long long r = (long long)base + j0 + u + 1;  // row of xj
        xn[u] = (live && u < nb && r < n) ? xc[r * ldx] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        if (u < nb) {  // uniform
          const int j = j0 + u;
          const long long i = (long long)base + j;
          double u0, u1, u2, xi = xcur, xj = xn[u];
          dlaf::trilu::forward(a, b, se[j], sd[j] - shift, se[j + 1], tol, xi,
                               xj, u0, u1, u2);
          xcur = xj;
          if (live) {
            xc[i * ldx] = xi;
            uc[i * cols] = u0;
            uc[plane + i * cols] = u1;
            uc[2 * plane + i * cols] = u2;
          }
        }
      }
    }
  }

  // back substitution, rows n-1 .. 0
  double y1 = 0.0, y2 = 0.0;
  for (long long top = n; top > 0; top -= kBatch) {
    const int nb = (int)min((long long)kBatch, top);
    double xv[kBatch], v0[kBatch], v1[kBatch], v2[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const bool on = live && u < nb;
      const long long i = top - 1 - u;
      xv[u] = on ? xc[i * ldx] : 0.0;
      v0[u] = on ? uc[i * cols] : 1.0;
      v1[u] = on ? uc[plane + i * cols] : 0.0;
      v2[u] = on ? uc[2 * plane + i * cols] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      if (u < nb) {  // uniform
        const double y = dlaf::trilu::back(xv[u], v0[u], v1[u], v2[u], y1, y2);
        y2 = y1;
        y1 = y;
        if (live) xc[(top - 1 - u) * ldx] = y;
      }
    }
  }
}

}  // namespace

void dlaf::tridiag_shifted_solve(const double* d, const double* e, int n,
                                 const double* lam, int k, double tol,
                                 double* X, long long ldx, double* work,
                                 long long cols, hipStream_t stream) {
  if (n <= 0 || k <= 0) return;
  const int blocks = (k + kThreads - 1) / kThreads;
  shifted_solve_kernel<<<blocks, kThreads, 0, stream>>>(d, e, n, lam, k, tol,
                                                        X, ldx, work, cols);
}
