"""Tridiagonal test families and the independent extended-precision
reference shared by the bisection tests (CPU and GPU).

The reference is a Sturm-count bisection written here in ``numpy.longdouble``
(vectorised over the eigenvalues, 90 fixed halvings of the Gershgorin
interval); it imports nothing from the code under test. Without an 80-bit
long double the dense LAPACK eigenvalues stand in, with the looser bound.
"""

from functools import lru_cache

import numpy as np

EPS = 2.0 ** -52
HAVE_LONGDOUBLE = np.finfo(np.longdouble).eps < 1e-18
# |w - w_ref| <= TOL_FACTOR * eps * G: 4 against the longdouble bisection
# (a float64 prototype of the recurrence measured 0.74), 64 against dense
# LAPACK (itself up to 17.5 eps*G from the longdouble values)
TOL_FACTOR = 4.0 if HAVE_LONGDOUBLE else 64.0

FAMILIES = ["random", "wilkinson", "toeplitz", "glued_wilkinson",
            "random_split", "graded", "constant_diag"]


def make_case(family: str, n: int):
    """(d [n], e [n-1]) float64 numpy arrays."""
    rng = np.random.default_rng(1234 + n)
    m = max(n - 1, 0)
    i = np.arange(n, dtype=np.float64)
    if family == "random":
        d, e = rng.standard_normal(n), rng.standard_normal(m)
    elif family == "wilkinson":
        d, e = np.abs(i - (n - 1) / 2.0), np.ones(m)
    elif family == "toeplitz":
        d, e = np.full(n, 2.0), np.full(m, -1.0)
    elif family == "glued_wilkinson":
        # Wilkinson-21 blocks glued with 1e-8 (twelve of them at n = 252)
        d = np.abs((np.arange(n) % 21) - 10.0)
        e = np.ones(m)
        e[(np.arange(m) % 21) == 20] = 1e-8
    elif family == "random_split":
        d, e = rng.standard_normal(n), rng.standard_normal(m)
        for p in (m // 4, m // 2, (3 * m) // 4):
            if m:
                e[p] = 0.0
    elif family == "graded":
        d = 10.0 ** (-i / 16.0)
        e = 0.5 * 10.0 ** (-(i[:m] + 0.5) / 16.0)
    elif family == "constant_diag":
        d, e = np.full(n, 3.0), np.zeros(m)
    else:
        raise ValueError(family)
    return d.astype(np.float64), e.astype(np.float64)


def gershgorin(d, e):
    """(gl, gu, G = max(|gl|, |gu|)), not widened."""
    n = len(d)
    r = np.zeros(n)
    if n > 1:
        r[:-1] += np.abs(e)
        r[1:] += np.abs(e)
    gl, gu = float((d - r).min()), float((d + r).max())
    return gl, gu, max(abs(gl), abs(gu))


def _count_ld(d, e2, pivmin, x):
    """#eigenvalues < x[j], vectorised over x, in long double."""
    q = d[0] - x
    q = np.where(np.abs(q) < pivmin, -pivmin, q)
    cnt = (q < 0).astype(np.int64)
    for i in range(1, len(d)):
        q = (d[i] - x) - e2[i - 1] / q
        q = np.where(np.abs(q) < pivmin, -pivmin, q)
        cnt += q < 0
    return cnt


def _reference_uncached(d, e):
    n = len(d)
    if n == 1:
        return d.astype(np.longdouble)  # exact (also covers the zero matrix)
    if not HAVE_LONGDOUBLE:
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        return np.linalg.eigvalsh(T)
    ld = np.longdouble
    dl, el = d.astype(ld), e.astype(ld)
    e2 = el * el
    pivmin = ld(np.finfo(np.float64).tiny) * max(ld(1), e2.max() if n > 1 else ld(1))
    gl, gu, G = gershgorin(d, e)
    pad = ld(G) * ld(1e-10) + ld(1e-300)
    lo = np.full(n, ld(gl) - pad, dtype=ld)
    hi = np.full(n, ld(gu) + pad, dtype=ld)
    k = np.arange(n)
    for _ in range(90):
        mid = lo + (hi - lo) / 2
        below = _count_ld(dl, e2, pivmin, mid) <= k
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    return lo + (hi - lo) / 2


@lru_cache(maxsize=None)
def reference(family: str, n: int):
    """Reference eigenvalues (long double where available), computed once per
    case and shared; callers must not modify the returned array."""
    d, e = make_case(family, n)
    w = _reference_uncached(d, e)
    w.setflags(write=False)
    return w


def max_err_units(w, family: str, n: int) -> float:
    """max |w - w_ref| in units of eps*G."""
    d, e = make_case(family, n)
    G = gershgorin(d, e)[2]
    ref = reference(family, n)
    err = np.abs(np.asarray(w, dtype=ref.dtype) - ref).max()
    if err == 0:
        return 0.0  # also the G == 0 case (zero matrix)
    return float(err / (EPS * G)) if G > 0 else float("inf")
