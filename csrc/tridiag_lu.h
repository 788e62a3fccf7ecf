// Partially pivoted LU solve of (T - lam I) y = x for ONE column of a real
// symmetric tridiagonal T (diagonal d[0..n), off-diagonal e[0..n-1)), double
// precision only: LAPACK dlagtf + dlagts folded into one forward sweep and
// one back substitution. One definition for the host twin (ext.cpp) and the
// device kernel (invit.hip): both sides run exactly these operations in this
// order, with the IEEE division and no contraction.
//
// Forward step i eliminates between the working row (a, b) = what is left of
// row i in columns (i, i+1) and row i+1 = (sub, nd, ne) = (e[i], d[i+1]-lam,
// e[i+1]) in columns (i, i+1, i+2). The row with the larger leading entry
// becomes row i of U = (u0, u1, u2); the multiplier goes to the right-hand
// side at once, so neither L nor the pivot flags are kept. A pivot below
// `tol` in magnitude is replaced by copysign(tol, u0) (dlagts job = -1: the
// perturbation that keeps inverse iteration alive on an exact eigenvalue).
// The last row is the same step with row n = (0, 0, 0) and x[n] = 0: it never
// swaps and leaves u0 = floored a, u1 = +-0, u2 = 0, so the sweep is n
// uniform steps and the back substitution n uniform steps with y[n] =
// y[n+1] = 0.
//
// Selects only, no data-dependent branch: the pivot choice differs per lane.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define TRILU_HD __host__ __device__ inline
#else
#define TRILU_HD inline
#endif

namespace dlaf {
namespace trilu {

// In: working row (a, b), next row (sub, nd, ne), right-hand sides xi (row i)
// and xj (row i+1). Out: U row (u0, u1, u2), xi = right-hand side of U row i,
// xj = updated right-hand side of the new working row, (a, b) = new working
// row.
TRILU_HD void forward(double& a, double& b, double sub, double nd, double ne,
                      double tol, double& xi, double& xj, double& u0,
                      double& u1, double& u2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool swap = fabs(sub) > fabs(a);
  const double p = swap ? sub : a;  // pivot
  const double o = swap ? a : sub;  // the entry it eliminates
  u0 = fabs(p) < tol ? copysign(tol, p) : p;
  u1 = swap ? nd : b;
  u2 = swap ? ne : 0.0;
  const double m = o / u0;
  const double xp = swap ? xj : xi;
  const double xo = swap ? xi : xj;
  // eliminated row, columns (i+1, i+2)
  const double ra = swap ? b : nd;
  const double rb = swap ? 0.0 : ne;
  a = ra - m * u1;
  b = rb - m * u2;
  xi = xp;
  xj = xo - m * xp;
}

// y[i] from U row i, its right-hand side and y[i+1], y[i+2].
TRILU_HD double back(double x, double u0, double u1, double u2, double y1,
                     double y2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((x - u1 * y1) - u2 * y2) / u0;
}

}  // namespace trilu
}  // namespace dlaf
