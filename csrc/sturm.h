// Sturm-sequence eigenvalue count and bisection for a real symmetric
// tridiagonal matrix (diagonal d[0..n), off-diagonal e[0..n-1)), double
// precision only. One definition for the host twins (ext.cpp) and the device
// kernels (bisect.hip): both sides run exactly these operations in this
// order, with the IEEE division.
//
//   e2[i]  = e[i]^2
//   pivmin = DBL_MIN * max(1, max_i e2[i])
//   count(x) = #{eigenvalues < x}: q_0 = d_0 - x, q_i = (d_i - x) - e2[i-1]/q_{i-1};
//     after every step |q| < pivmin -> q = -pivmin (the dstebz safeguard, which
//     makes zero off-diagonals and exact hits well defined), then count q < 0.
//     With IEEE division the count is monotone in x, so bisection on it
//     returns the eigenvalues in ascending order.
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define STURM_HD __host__ __device__ inline
#else
#define STURM_HD inline
#endif

namespace dlaf {
namespace sturm {

constexpr int kMaxBisect = 128;  // cap; ~60 halvings reach the stop width

// One step of the recurrence. `q` is the previous pivot (1 before the first
// step), `e2prev` is e2[i-1] (0 before the first step, so the first pivot is
// exactly d[0] - x). Returns the new pivot and bumps `cnt` when it is
// negative.
template <typename Count>
STURM_HD double step(double q, double di, double e2prev, double x,
                     double pivmin, Count& cnt) {
  q = (di - x) - e2prev / q;
  if (fabs(q) < pivmin) q = -pivmin;
  if (q < 0.0) ++cnt;
  return q;
}

// Number of eigenvalues strictly below x. e2 has n-1 entries.
STURM_HD long long count(const double* d, const double* e2, int n,
                         double pivmin, double x) {
  long long cnt = 0;
  double q = 1.0;
  for (int i = 0; i < n; ++i)
    q = step(q, d[i], i ? e2[i - 1] : 0.0, x, pivmin, cnt);
  return cnt;
}

// Bisection state for one eigenvalue. `mid` is the next point to evaluate
// while !done, and the result once done.
struct Bisect {
  double lo, hi, mid;
  int it;
  bool done;
};

STURM_HD void bisect_prepare(Bisect& s, double pivmin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double width = s.hi - s.lo;
  const double half = 0.5 * width;
  s.mid = s.lo + half;
  const double amax = fmax(fabs(s.lo), fabs(s.hi));
  const double t1 = 2.0 * DBL_EPSILON * amax;
  const double tol = t1 + 2.0 * pivmin;
  s.done = !(s.lo < s.mid && s.mid < s.hi) || width <= tol ||
           s.it >= kMaxBisect;
}

STURM_HD void bisect_begin(Bisect& s, double gl, double gu, double pivmin) {
  s.lo = gl;
  s.hi = gu;
  s.it = 0;
  bisect_prepare(s, pivmin);
}

// Feed count(s.mid) for eigenvalue k (0-based, ascending).
STURM_HD void bisect_update(Bisect& s, long long cnt, int k, double pivmin) {
  if (cnt <= k)
    s.lo = s.mid;
  else
    s.hi = s.mid;
  ++s.it;
  bisect_prepare(s, pivmin);
}

// Host-side setup: pivmin and the widened Gershgorin interval [gl, gu] that
// contains every eigenvalue. e has n-1 entries.
inline void interval(const double* d, const double* e, int n, double* gl_out,
                     double* gu_out, double* pivmin_out) {
  double e2max = 0.0;
  for (int i = 0; i + 1 < n; ++i) e2max = fmax(e2max, e[i] * e[i]);
  const double pivmin = DBL_MIN * fmax(1.0, e2max);
  double gl = 0.0, gu = 0.0;
  for (int i = 0; i < n; ++i) {
    const double r = (i > 0 ? fabs(e[i - 1]) : 0.0) +
                     (i + 1 < n ? fabs(e[i]) : 0.0);
    const double a = d[i] - r, b = d[i] + r;
    if (i == 0 || a < gl) gl = a;
    if (i == 0 || b > gu) gu = b;
  }
  const double tnorm = fmax(fabs(gl), fabs(gu));
  const double widen = 2.0 * tnorm * DBL_EPSILON * n + 2.0 * pivmin;
  *gl_out = gl - widen;
  *gu_out = gu + widen;
  *pivmin_out = pivmin;
}

}  // namespace sturm
}  // namespace dlaf
