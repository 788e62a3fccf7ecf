"""Matrices, truths and bounds shared by the refinement tests (CPU and GPU):
the Hermitian vector product of csrc/hemv.hip, cholesky_refine,
cholesky_solve_expert and cholesky_solve_mixed. SPD kinds, shapes and dtypes
are those of cond_cases.py.

Vector product, against the float64 / complex128 product on the host of the
numbers as stored (``|.|`` is CABS1, ``|re| + |im|``), componentwise:

    |y - A x|_i          <= (n + 2) eps (|A| |x|)_i
    |yabs - |A| |x||_i   <= (n + 4) eps (|A| |x|)_i

the standard dot-product bound plus the final rounding; nothing measured.

cholesky_refine: berr <= 4 eps(dtype) (numpy eps; LAPACK's ?posvx reaches at
most 1.29 eps over the table, the factor is the margin for another summation
order); the true relative forward error is at most ferr.

The ferr band. ferr depends on |r| at rounding level, so it is not bitwise
LAPACK's. The ``"blocked"`` method was run on the CPU over the whole table
(SOLVE_SHAPES x SPD kinds x dtypes x uplos, three right-hand sides) before
the kernel ran: ferr / ferr_ref against ``scipy.linalg.lapack.?posvx``
(fact='N') stayed within FERR_RATIO_BLOCKED. The band is that range widened
by 2 on each side; the device result is held to the same band against the
CPU result.

cholesky_solve_mixed converges when, for every column,

    ||b - A x||_inf <= ||x||_inf ||A||_inf eps sqrt(n),  eps = 2^-53,

with CABS1 inside the vector norms (dsposv / zcposv). The tests evaluate it
for the returned x with the residual formed in extended precision.
"""

from functools import lru_cache

import numpy as np
import torch

import cond_cases as cc
from cond_cases import make_spd, to_matrix, DTYPES, UPLOS, eps_of  # noqa: F401

from dlaf_amd import UpLo

NRHS = 3
REFINE_SHAPES = [(7, 16), (100, 32), (330, 160)]
MIXED_DTYPES = ("float64", "complex128")

# smallest and largest ferr / ferr_ref of the "blocked" method on the CPU
FERR_RATIO_BLOCKED = (0.8596, 1.1183)
FERR_BAND = (FERR_RATIO_BLOCKED[0] / 2, FERR_RATIO_BLOCKED[1] * 2)


def np_eps(dtype: str) -> float:
    return float(np.finfo(dtype).eps)


def cabs1(a):
    a = np.asarray(a)
    return np.abs(a.real) + np.abs(a.imag) if np.iscomplexobj(a) else np.abs(a)


def stored_hermitian(a, uplo):
    """What a caller may hold for the Hermitian matrix ``a``: 1e30 in the
    other triangle and, for complex, 1e30 i added to the stored diagonal."""
    s = np.array(a)
    n = s.shape[0]
    i, j = np.indices((n, n))
    s[(j > i) if uplo == UpLo.Lower else (j < i)] = 1e30
    if np.iscomplexobj(s):
        s[i == j] += 1e30j
    return s


@lru_cache(maxsize=None)
def vector(n, dtype, salt=57):
    return cc._frozen(cc._random(cc._rng(n, dtype, salt), (n,), dtype), dtype)


@lru_cache(maxsize=None)
def rhs_block(n, dtype):
    return cc._frozen(cc._random(cc._rng(n, dtype, 41), (n, NRHS), dtype),
                      dtype)


@lru_cache(maxsize=None)
def product_truth(kind, n, dtype):
    """(A x, |A| |x|) in float64 / complex128 of the stored numbers."""
    w = cc.wide(dtype)
    a, x = make_spd(kind, n, dtype).astype(w), vector(n, dtype).astype(w)
    return a @ x, cabs1(a) @ cabs1(x)


def check_product(y, yabs, kind, n, dtype):
    want, wabs = product_truth(kind, n, dtype)
    eps = eps_of(dtype)
    err = np.abs(np.asarray(y).astype(cc.wide(dtype)) - want)
    assert (err <= (n + 2) * eps * wabs).all(), (err / (eps * wabs)).max()
    aerr = np.abs(np.asarray(yabs).astype(np.float64) - wabs)
    assert (aerr <= (n + 4) * eps * wabs).all(), (aerr / (eps * wabs)).max()


@lru_cache(maxsize=None)
def solve_truth(kind, n, dtype):
    w = cc.wide(dtype)
    x = np.linalg.solve(make_spd(kind, n, dtype).astype(w),
                        rhs_block(n, dtype).astype(w))
    x.setflags(write=False)
    return x


def forward_error(x, kind, n, dtype):
    xt = solve_truth(kind, n, dtype)
    return (np.abs(np.asarray(x) - xt).max(axis=0) / np.abs(xt).max(axis=0))


def check_bounds(x, ferr, berr, kind, n, dtype):
    """Items (a) and (b): berr <= 4 eps, true forward error <= ferr."""
    ferr, berr = ferr.numpy(), berr.numpy()
    assert ferr.dtype == np.float64 and berr.dtype == np.float64
    assert ferr.shape == (NRHS,) and berr.shape == (NRHS,)
    true = forward_error(x, kind, n, dtype)
    print(f"{kind} n={n} {dtype} berr/eps={berr / np_eps(dtype)} "
          f"true/ferr={true / ferr}")
    assert (berr <= 4 * np_eps(dtype)).all(), berr / np_eps(dtype)
    assert (true <= ferr).all(), (true, ferr)


def check_band(ferr, ferr_ref):
    q = np.asarray(ferr) / np.asarray(ferr_ref)
    assert (FERR_BAND[0] <= q).all() and (q <= FERR_BAND[1]).all(), q


def run_refine(kind, n, nb, dtype, uplo, device, method, grid=None,
               perturb=False):
    """cholesky_refine on X from cholesky_solve (one entry pushed off by
    1e3 eps ||x|| with ``perturb``); returns (x, ferr, berr)."""
    from dlaf_amd import (cholesky_factorization, cholesky_solve,
                          cholesky_refine)
    A = to_matrix(make_spd(kind, n, dtype), nb, device, grid)
    B = to_matrix(rhs_block(n, dtype), nb, device, grid)
    L = A.clone()
    cholesky_factorization(uplo, L, grid)
    X = B.clone()
    cholesky_solve(uplo, L, X, grid)
    if perturb:
        xg = X.to_global()
        xg[n // 2, 1] += 1e3 * np_eps(dtype) * float(xg[:, 1].abs().max())
        X.set_from_global(xg)
    keep = [A.storage.clone(), L.storage.clone(), B.storage.clone()]
    ferr, berr = cholesky_refine(uplo, A, L, B, X, grid, method)
    for m, k in zip((A, L, B), keep):
        assert torch.equal(m.storage, k)
    return X.to_global().cpu().numpy(), ferr, berr


@lru_cache(maxsize=None)
def blocked_ferr(kind, n, nb, dtype, uplo):
    """ferr of the "blocked" method on the CPU (the device's reference)."""
    _, ferr, _ = run_refine(kind, n, nb, dtype, uplo, "cpu", "blocked")
    return ferr.numpy()


def mixed_criterion(a, b, x) -> bool:
    """The convergence test of cholesky_solve_mixed, on the host. The
    threshold is a few units of the last place of ||A|| ||x||, which is also
    the size of the rounding error of a float64 ``b - a @ x``: the residual
    is formed in extended precision, so that the test sees the returned x
    and not the host's own rounding."""
    n = a.shape[0]
    ext = np.clongdouble if np.iscomplexobj(a) else np.longdouble
    r = b.astype(ext) - a.astype(ext) @ x.astype(ext)
    cte = np.abs(a).sum(axis=1).max() * 2.0 ** -53 * np.sqrt(n)
    return bool((cabs1(r).max(axis=0) <= cabs1(x).max(axis=0) * cte).all())


def potrs_residual_ok(a, b, x) -> bool:
    """||A x - b||_inf <= 100 n eps (||A||_inf ||x||_inf + ||b||_inf), the
    p?potrs bound of tests/c/test_dlaf_c_cond.c."""
    n = a.shape[0]
    res = np.abs(a @ x - b).max()
    scale = np.abs(a).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return bool(res <= 100 * n * np_eps(a.dtype.name) * scale)


@lru_cache(maxsize=None)
def ill_conditioned(n, dtype):
    """Q diag(logspace(0, -10)) Q^H: beyond single precision."""
    g = cc._random(cc._rng(n, dtype, 71), (n, n), dtype)
    q, _ = np.linalg.qr(g)
    a = (q * np.logspace(0.0, -10.0, n)) @ q.conj().T
    return cc._frozen((a + a.conj().T) / 2, dtype)


def run_mixed(a, b, nb, uplo, device, grid=None):
    """cholesky_solve_mixed; checks that A and B are bit-unchanged. Returns
    (x or None, iters, info)."""
    from dlaf_amd import cholesky_solve_mixed
    A, B = to_matrix(a, nb, device, grid), to_matrix(b, nb, device, grid)
    ka, kb = A.storage.clone(), B.storage.clone()
    X, iters, info = cholesky_solve_mixed(uplo, A, B, grid)
    assert torch.equal(A.storage, ka) and torch.equal(B.storage, kb)
    return (None if X is None else X.to_global().cpu().numpy()), iters, info


def check_mixed_spd(kind, n, nb, dtype, uplo, device):
    a, b = make_spd(kind, n, dtype), rhs_block(n, dtype)
    x, iters, info = run_mixed(a, b, nb, uplo, device)
    print(f"mixed {kind} n={n} {dtype} {uplo.value} iters={iters}")
    assert 0 <= iters <= 8 and info == 0, (iters, info)
    assert x.dtype == a.dtype
    assert mixed_criterion(a, b, x)


def check_mixed_fallback(dtype, uplo, device):
    n, nb = 100, 32
    a, b = ill_conditioned(n, dtype), rhs_block(n, dtype)
    x, iters, info = run_mixed(a, b, nb, uplo, device)
    print(f"mixed kappa=1e10 {dtype} {uplo.value} iters={iters}")
    assert iters in (-3, -31) and info == 0, (iters, info)
    # the double precision fallback is cholesky_solve: held to the residual
    # bound the C-ABI test sets for p?potrs (the absolute-error bound of
    # cond_cases.solve_tol presumes ||A^-1|| ~ 1; it is 1e10 here)
    assert potrs_residual_ok(a, b, x)


def check_mixed_overflow(dtype, uplo, device):
    n, nb = 100, 32
    a = np.array(make_spd("diagdom", n, dtype))
    a[n - 1, n - 1] = 1e39
    x, iters, info = run_mixed(a, rhs_block(n, dtype), nb, uplo, device)
    assert iters == -2 and info == 0, (iters, info)
    assert potrs_residual_ok(a, rhs_block(n, dtype), x)


def check_expert(device, method):
    from dlaf_amd import (matrix_norm, cholesky_factorization, cholesky_rcond,
                          cholesky_solve, cholesky_refine,
                          cholesky_solve_expert)
    n, nb, dtype, uplo = 100, 32, "float64", UpLo.Lower
    A = to_matrix(make_spd("wishart", n, dtype), nb, device)
    B = to_matrix(rhs_block(n, dtype), nb, device)
    ka, kb = A.storage.clone(), B.storage.clone()
    X, L, rcond, ferr, berr, info = cholesky_solve_expert(uplo, A, B,
                                                          method=method)
    assert torch.equal(A.storage, ka) and torch.equal(B.storage, kb)
    anorm = matrix_norm("one", A, structure="hermitian", uplo=uplo)
    L2 = A.clone()
    cholesky_factorization(uplo, L2)
    X2 = B.clone()
    cholesky_solve(uplo, L2, X2)
    ferr2, berr2 = cholesky_refine(uplo, A, L2, B, X2, method=method)
    assert info == 0
    assert torch.equal(L.storage, L2.storage)
    assert torch.equal(X.storage, X2.storage)
    assert rcond == cholesky_rcond(uplo, L2, anorm, method=method)
    assert torch.equal(ferr, ferr2) and torch.equal(berr, berr2)
    # not positive definite: the pivot that fails
    bad = np.array(make_spd("wishart", n, dtype))
    bad[40, 40] = -1.0
    out = cholesky_solve_expert(uplo, to_matrix(bad, nb, device), B,
                                method=method)
    assert out[0] is None and out[5] == 41, out[5]
