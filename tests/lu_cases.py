"""Matrices, references and checks shared by the LU tests (CPU twin and HIP
kernel). The independent reference is ``torch.linalg.lu_factor`` on the CPU,
which the library itself never calls.

Matrices, frozen numpy arrays from fixed seeds:

    planted    P0^T L0 U0. L0 unit lower, off-diagonals uniform in +-0.4
               (complex: both parts, divided by sqrt 2); U0 upper, diagonal
               magnitudes in [0.5, 1.5]. The pivot order is forced: at step j
               the rivals of the planted pivot u_jj are l_ij u_jj, smaller by
               1 / 0.4 in modulus, which is still > 1 after the sqrt 2 between
               CABS1 and the modulus. Badly conditioned for large n, so only
               pivots, multipliers and residuals are checked on it, n <= 200.
    scrambled  (G + 0.75 n I)[perm], G uniform in +-0.5: well conditioned,
               non-trivial pivots.
    random     uniform in +-0.5; residual only.

Every ``planted`` and ``scrambled`` fixture is asserted, in a float64 /
complex128 elimination, to have its pivot beat the second candidate by a
factor of at least 1.4 at every step: a condition on the fixtures that makes
"the pivots equal the reference's" a fair demand in single precision too.

Residual: rho = ||P A - L U||_1 / ||A||_1, in float64 / complex128, must be at
most 10 max(rho_ref, eps), rho_ref the same figure for the reference's factor
of the same array in the same dtype. The factor 10 covers a different
summation order (blocked, MFMA) and the row solve through an explicit
unit-lower tile inverse.
"""

from functools import lru_cache

import numpy as np
import torch

import cond_cases as cc
from dlaf_amd import Matrix, Op

DTYPES = cc.DTYPES
OPS = cc.OPS
KINDS = ("planted", "scrambled", "random")
# (n, nb): one tile, a full tile, several tiles, a partial last tile with a
# misaligned tile base (17), nb = kLuW, nb not a multiple of kLuW (40), nb
# above kLuW (64), and a tile of several inner blocks over several row chunks
SHAPES = [(1, 16), (16, 16), (40, 16), (70, 17), (100, 32), (165, 40),
          (200, 64)]
BIG = (300, 160)  # scrambled only
MIN_PIVOT_RATIO = 1.4


def _frozen(a, dtype):
    a = np.ascontiguousarray(a.astype(dtype))
    a.setflags(write=False)
    return a


def _rng(n, dtype, salt):
    return np.random.default_rng(104729 * n + 37 * len(dtype) + salt)


def _uniform(rng, shape, dtype, half):
    if cc.is_complex(dtype):
        s = half / np.sqrt(2.0)
        return rng.uniform(-s, s, shape) + 1j * rng.uniform(-s, s, shape)
    return rng.uniform(-half, half, shape)


def cabs1(a):
    return np.abs(a.real) + np.abs(a.imag)


def pivot_ratio(a) -> float:
    """Smallest (largest candidate / second candidate) over the steps of a
    float64 / complex128 elimination with LAPACK's pivot rule."""
    w = np.array(a, dtype=cc.wide(a.dtype.name))
    n = w.shape[0]
    worst = np.inf
    for j in range(n - 1):
        cand = cabs1(w[j:, j])
        order = np.argsort(-cand, kind="stable")
        p = j + int(order[0])
        if cand[order[1]] > 0:
            worst = min(worst, cand[order[0]] / cand[order[1]])
        if p != j:
            w[[j, p]] = w[[p, j]]
        w[j + 1:, j] /= w[j, j]
        w[j + 1:, j + 1:] -= np.outer(w[j + 1:, j], w[j, j + 1:])
    return float(worst)


@lru_cache(maxsize=None)
def make(kind, n, dtype):
    rng = _rng(n, dtype, KINDS.index(kind))
    if kind == "planted":
        assert n <= 200
        l0 = np.tril(_uniform(rng, (n, n), dtype, 0.4), -1) + np.eye(n)
        u0 = np.triu(_uniform(rng, (n, n), dtype, 0.5), 1)
        mag = rng.uniform(0.5, 1.5, n)
        if cc.is_complex(dtype):
            diag = mag * np.exp(2j * np.pi * rng.uniform(0, 1, n))
        else:
            diag = mag * rng.choice([-1.0, 1.0], n)
        u0 = u0 + np.diag(diag)
        a = np.empty((n, n), dtype=u0.dtype)
        a[rng.permutation(n)] = l0 @ u0
    elif kind == "scrambled":
        g = _uniform(rng, (n, n), dtype, 0.5)
        a = (g + 0.75 * n * np.eye(n))[rng.permutation(n)]
    else:
        a = _uniform(rng, (n, n), dtype, 0.5)
    a = _frozen(a, dtype)
    if kind != "random" and n > 1:
        ratio = pivot_ratio(a)
        assert ratio >= MIN_PIVOT_RATIO, (kind, n, dtype, ratio)
    return a


@lru_cache(maxsize=None)
def singular(n, dtype, cols):
    """``scrambled`` with the columns ``cols`` zeroed."""
    a = np.array(make("scrambled", n, dtype))
    a[:, list(cols)] = 0
    return _frozen(a, dtype)


def residual(a, lu, piv0) -> float:
    """||P A - L U||_1 / ||A||_1 in float64 / complex128; ``piv0`` 0-based."""
    w = cc.wide(a.dtype.name)
    pa = np.array(a, dtype=w)
    for j, p in enumerate(np.asarray(piv0).tolist()):
        if p != j:
            pa[[j, p]] = pa[[p, j]]
    f = np.asarray(lu).astype(w)
    n = f.shape[0]
    r = pa - (np.tril(f, -1) + np.eye(n)) @ np.triu(f)
    return cc.norm1(r) / cc.norm1(pa)


@lru_cache(maxsize=None)
def reference(a_key):
    """(0-based pivots, info, rho_ref) of torch.linalg.lu_factor_ex on the
    CPU, in the array's own dtype. ``a_key``: ("kind", kind, n, dtype) or
    ("singular", n, dtype, cols)."""
    a = array_of(a_key)
    lu, piv, info = torch.linalg.lu_factor_ex(torch.from_numpy(np.array(a)))
    piv0 = (piv - 1).numpy().astype(np.int64)
    piv0.setflags(write=False)
    return piv0, int(info), residual(a, lu.numpy(), piv0)


def array_of(a_key):
    if a_key[0] == "kind":
        return make(*a_key[1:])
    return singular(*a_key[1:])


def factor(a, nb, device):
    from dlaf_amd import lu_factorization
    A = cc.to_matrix(a, nb, device)
    ipiv, info = lu_factorization(A)
    return A, ipiv, info


def check_padding(A: Matrix) -> None:
    """The identity extension of a partial last tile."""
    d = A.dist
    n, nb, nt = d.m, d.nb, d.nr_tiles[0]
    pad = nt * nb - n
    if nt == 0 or pad == 0:
        return
    st = A.storage
    v = nb - pad
    assert not bool(st[nt - 1, : nt - 1, v:, :].any())
    assert not bool(st[: nt - 1, nt - 1, :, v:].any())
    last = st[nt - 1, nt - 1]
    assert not bool(last[v:, :v].any()) and not bool(last[:v, v:].any())
    assert torch.equal(last[v:, v:], torch.eye(pad, dtype=A.dtype,
                                               device=A.device))


def check_factor(a_key, nb, device, pivots_must_match=True):
    """Checks 1-3 (and the info of check 4) for one array; returns
    (A, ipiv, info, rho / max(rho_ref, eps))."""
    a = array_of(a_key)
    dtype = a.dtype.name
    n = a.shape[0]
    eps = cc.eps_of(dtype)
    piv_ref, info_ref, rho_ref = reference(a_key)
    A, ipiv, info = factor(a, nb, device)
    assert ipiv.dtype == torch.int32 and ipiv.shape == (n,)
    assert ipiv.device == A.device
    piv = ipiv.cpu().numpy().astype(np.int64)
    assert (piv >= np.arange(n)).all() and (piv < n).all()
    assert info == info_ref, (info, info_ref)
    if pivots_must_match:
        assert np.array_equal(piv, piv_ref), np.nonzero(piv != piv_ref)[0][:8]
    f = A.to_global().cpu().numpy()
    assert np.isfinite(f).all()
    low = np.abs(np.tril(f.astype(cc.wide(dtype)), -1))
    bound = (np.sqrt(2.0) if cc.is_complex(dtype) else 1.0) * (1 + 4 * eps)
    assert low.max(initial=0.0) <= bound, low.max()
    rho = residual(a, f, piv)
    ratio = rho / max(rho_ref, eps)
    print(f"{a_key} nb={nb} {device}: rho={rho:.3e} rho_ref={rho_ref:.3e} "
          f"ratio={ratio:.3f}")
    assert rho <= 10 * max(rho_ref, eps), (rho, rho_ref)
    check_padding(A)
    return A, ipiv, info, ratio


def zero_cols(n):
    """(c,) and (c, c2): a column inside the first tile and a later one."""
    c = n // 3
    return (c,), (c, min(n - 1, c + n // 2))


def check_singular(n, nb, dtype, device):
    """Check 4."""
    from dlaf_amd import lu_rcond, general_solve
    for cols in zero_cols(n):
        key = ("singular", n, dtype, cols)
        A, ipiv, info, _ = check_factor(key, nb, device,
                                        pivots_must_match=False)
        c = cols[0]
        assert info == c + 1
        f = A.to_global().cpu().numpy()
        assert f[c, c] == 0
        assert int(ipiv[c]) == c
        a = array_of(key)
        assert lu_rcond("one", A, cc.norm1(a)) == 0.0
        assert lu_rcond("inf", A, cc.norm1(a.T)) == 0.0
        b = rhs(n, 3, dtype)
        A2, B = cc.to_matrix(a, nb, device), cc.to_matrix(b, nb, device)
        before = B.storage.clone()
        ipiv2, info2 = general_solve(A2, B)
        assert info2 == c + 1
        assert torch.equal(B.storage, before)
        assert torch.equal(ipiv2, ipiv)
        assert torch.equal(A2.storage, A.storage)


@lru_cache(maxsize=None)
def rhs(n, nrhs, dtype):
    return _frozen(_uniform(_rng(n, dtype, 51 + nrhs), (n, nrhs), dtype, 0.5),
                   dtype)


def check_solve(n, nb, dtype, device, nrhs_list=(1, 3)):
    """Check 5 on ``scrambled``."""
    from dlaf_amd import lu_solve, general_solve
    a = make("scrambled", n, dtype)
    w = cc.wide(dtype)
    LU, ipiv, info = factor(a, nb, device)
    assert info == 0
    for nrhs in nrhs_list:
        b = rhs(n, nrhs, dtype)
        for op in OPS:
            B = cc.to_matrix(b, nb, device)
            lu_solve(op, LU, ipiv, B)
            want = np.linalg.solve(cc.apply_op(a.astype(w), op), b.astype(w))
            err = np.abs(B.to_global().cpu().numpy() - want).max()
            print(f"getrs n={n} nb={nb} {dtype} {op.value} nrhs={nrhs} "
                  f"err={err:.3e}")
            assert err < cc.solve_tol(dtype, n + nrhs), (op, nrhs, err)
            if op == Op.NoTrans:
                A2, B2 = cc.to_matrix(a, nb, device), cc.to_matrix(b, nb,
                                                                   device)
                ipiv2, info2 = general_solve(A2, B2)
                assert info2 == 0 and torch.equal(ipiv2, ipiv)
                assert torch.equal(A2.storage, LU.storage)
                assert torch.equal(B2.storage, B.storage)


def check_rcond(kind, n, nb, dtype, device, method="auto"):
    """Check 6: the estimator band against the exact inverse norm."""
    from dlaf_amd import lu_rcond, matrix_norm
    a = make(kind, n, dtype)
    A = cc.to_matrix(a, nb, device)
    norms = {nm: matrix_norm(nm, A) for nm in ("one", "inf")}
    from dlaf_amd import lu_factorization
    _, info = lu_factorization(A)
    assert info == 0
    out = {}
    for nm in ("one", "inf"):
        t = a if nm == "one" else a.T
        an, ai = cc.norm1(t.astype(cc.wide(dtype))), cc.inv_norm1(t)
        assert abs(norms[nm] - an) <= 4 * (n + 2) * cc.eps_of(dtype) * an
        est = lu_rcond(nm, A, norms[nm], method=method)
        print(f"gecon {kind} n={n} {dtype} {nm} est/true={est * an * ai:.6f}")
        cc.check_band(est, an, ai, n, dtype)
        out[nm] = est
    return A, norms, out


def reversed_toeplitz(n):
    """The (2, -1) Toeplitz matrix with its rows reversed: ||A||_1 = 4,
    ||A^-1||_1 = n (n + 2) / 8 for even n (a row permutation of A permutes
    the columns of the inverse), ipiv[j] = n - 1 - j for the first rows, and
    A x = e_1 + e_n has x = 1."""
    return np.ascontiguousarray(cc.toeplitz(n)[::-1])


def check_toeplitz(device, method="auto"):
    from dlaf_amd import lu_rcond, lu_solve, matrix_norm
    n, nb = 96, 32
    a = reversed_toeplitz(n)
    A = cc.to_matrix(a, nb, device)
    anorm = matrix_norm("one", A)
    assert anorm == 4.0
    from dlaf_amd import lu_factorization
    ipiv, info = lu_factorization(A)
    assert info == 0
    piv = ipiv.cpu().numpy()
    half = n // 2
    assert np.array_equal(piv[:half], n - 1 - np.arange(half))
    est = lu_rcond("one", A, anorm, method=method)
    assert abs(est * 4704.0 - 1.0) <= 1e-12, est
    b = np.zeros((n, 1))
    b[0] = b[n - 1] = 1.0
    B = cc.to_matrix(b, nb, device)
    lu_solve(Op.NoTrans, A, ipiv, B)
    assert np.abs(B.to_global().cpu().numpy() - 1.0).max() <= 1e-12
