"""Matrices, exact inverse norms and the bounds shared by the condition
estimate and triangular-vector-solve tests (CPU and GPU).

Random entries G are uniform with |g| <= 0.5 (real) or real and imaginary
parts in [-0.35, 0.35] (complex), seeded by shape and dtype.

    SPD  wishart   G G^H + 1e-3 n I
         diagdom   G G^H / n + n I
         graded    Q diag(logspace(0, -log10 k)) Q^H, Q orthogonal / unitary,
                   k = 1e6 (float64, complex128) or 1e3 (float32, complex64)
    triangular     tril(G) + 3 I, its transpose for Upper;
                   Diag.Unit: 0.5 tril(G, -1) / sqrt(n) under a unit diagonal

The truth is ``numpy.linalg.inv`` of the matrix in float64 / complex128 (the
matrix as rounded to the tested dtype). The estimator band is

    rcond_true (1 - delta) <= rcond_est <= 3 rcond_true,
    delta = 100 n eps(dtype) kappa_1

3 is the known worst practical underestimate of ``?lacn2``; delta covers the
rounding of the solves, which can only matter through kappa_1.

Vector solve: the normwise residual

    ||op(T) x - b||_inf <= SOLVE_C n eps (||T||_inf ||x||_inf + ||b||_inf)

computed in float64 / complex128 on the host. SOLVE_C was fixed before the
kernel ran: the ``"blocked"`` method (``triangular_solver`` on an n x 1 matrix,
the same error model through inverses of the diagonal tiles) was run on the
CPU over the whole SOLVE_SHAPES x uplo x op x diag x dtype table; the largest
ratio residual / (n eps (||T|| ||x|| + ||b||)) it reached was
SOLVE_RATIO_BLOCKED, and SOLVE_C is 4 times that, the margin being for the
kernel's different summation order.
"""

from functools import lru_cache

import numpy as np
import torch

from dlaf_amd import Matrix, UpLo, Op, Diag

DTYPES = ("float32", "float64", "complex64", "complex128")
UPLOS = (UpLo.Lower, UpLo.Upper)
OPS = (Op.NoTrans, Op.Trans, Op.ConjTrans)
DIAGS = (Diag.NonUnit, Diag.Unit)

# (n, nb) of the vector-solve table
SOLVE_SHAPES = [(1, 16), (7, 16), (40, 17), (64, 16), (100, 32), (200, 64),
                (330, 160)]
# largest ratio of the "blocked" method on the CPU over the whole table
SOLVE_RATIO_BLOCKED = 0.4342  # at n = 1, complex128; 0.17 in float32
SOLVE_C = 4 * SOLVE_RATIO_BLOCKED  # 1.7368

# (n, nb) of the estimator table
RCOND_SHAPES = [(1, 16), (2, 16), (3, 16), (17, 16), (64, 16), (100, 32),
                (257, 32)]
SPD_KINDS = ("wishart", "diagdom", "graded")


def eps_of(dtype: str) -> float:
    return 2.0 ** -23 if dtype in ("float32", "complex64") else 2.0 ** -52


def is_complex(dtype: str) -> bool:
    return dtype.startswith("complex")


def wide(dtype: str) -> str:
    return "complex128" if is_complex(dtype) else "float64"


def _random(rng, shape, dtype):
    if is_complex(dtype):
        return (rng.uniform(-0.35, 0.35, shape)
                + 1j * rng.uniform(-0.35, 0.35, shape))
    return rng.uniform(-0.5, 0.5, shape)


def _rng(n, dtype, salt):
    return np.random.default_rng(7919 * n + 31 * len(dtype) + salt)


def _frozen(a, dtype):
    a = np.ascontiguousarray(a.astype(dtype))
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def make_spd(kind, n, dtype):
    """Hermitian positive definite n x n numpy array of ``dtype``."""
    rng = _rng(n, dtype, SPD_KINDS.index(kind))
    g = _random(rng, (n, n), dtype)
    if kind == "wishart":
        a = g @ g.conj().T + 1e-3 * n * np.eye(n)
    elif kind == "diagdom":
        a = g @ g.conj().T / n + n * np.eye(n)
    else:
        cap = 1e3 if eps_of(dtype) > 1e-10 else 1e6
        q, _ = np.linalg.qr(g)
        lam = np.logspace(0.0, -np.log10(cap), n) if n > 1 else np.ones(1)
        a = (q * lam) @ q.conj().T
    a = (a + a.conj().T) / 2
    return _frozen(a, dtype)


@lru_cache(maxsize=None)
def make_triangular(n, dtype, uplo, diag):
    """The triangular matrix itself (zeros in the other triangle, ones on a
    unit diagonal)."""
    g = _random(_rng(n, dtype, 11), (n, n), dtype)
    if diag == Diag.Unit:
        t = 0.5 * np.tril(g, -1) / np.sqrt(n) + np.eye(n)
    else:
        t = np.tril(g) + 3.0 * np.eye(n)
    if uplo == UpLo.Upper:
        t = t.T
    return _frozen(t, dtype)


def stored_with_garbage(t, uplo, diag):
    """What a caller may hold for the triangular matrix ``t``: 1e30 in the
    other triangle and, for Diag.Unit, on the diagonal."""
    a = np.array(t)
    n = a.shape[0]
    i, j = np.indices((n, n))
    a[(j > i) if uplo == UpLo.Lower else (j < i)] = 1e30
    if diag == Diag.Unit:
        a[i == j] = 1e30
    return a


def to_matrix(a, nb, device="cpu", grid=None):
    m, n = a.shape
    mat = Matrix.create(m, n, nb, nb, dtype=getattr(torch, a.dtype.name),
                        device=device, grid=grid)
    if a.size:
        mat.set_from_global(torch.from_numpy(np.array(a)))
    return mat


def norm1(a) -> float:
    return float(np.abs(a).sum(axis=0).max()) if a.size else 0.0


def inv_norm1(a) -> float:
    """Exact ||a^-1||_1 of the stored numbers, in float64 / complex128."""
    return norm1(np.linalg.inv(a.astype(wide(a.dtype.name))))


def check_band(est: float, anorm: float, ainvnm: float, n: int, dtype: str):
    true = 1.0 / (anorm * ainvnm)
    delta = 100 * n * eps_of(dtype) * anorm * ainvnm
    assert true * (1 - delta) <= est <= 3 * true, (est, true, delta)


def apply_op(t, op):
    if op == Op.NoTrans:
        return t
    return t.T if op == Op.Trans else t.conj().T


@lru_cache(maxsize=None)
def rhs(n, dtype):
    return _frozen(_random(_rng(n, dtype, 23), (n,), dtype), dtype)


def solve_ratio(t, op, b, x, dtype: str) -> float:
    """residual / (n eps (||T||_inf ||x||_inf + ||b||_inf)), everything in
    float64 / complex128; SOLVE_C bounds it."""
    w = wide(dtype)
    tw = apply_op(t.astype(w), op)
    xw, bw = np.asarray(x).astype(w), np.asarray(b).astype(w)
    n = t.shape[0]
    res = np.abs(tw @ xw - bw).max()
    scale = np.abs(tw).sum(axis=1).max() * np.abs(xw).max() + np.abs(bw).max()
    return float(res / (n * eps_of(dtype) * scale))


def toeplitz(n):
    """The (2, -1) Toeplitz matrix: ||A||_1 = 4 and, the inverse having the
    entries min(i, j) (n + 1 - max(i, j)) / (n + 1) (1-based), column j of it
    sums to j (n + 1 - j) / 2: ||A^-1||_1 = 300 for n = 48 (j = 24)."""
    return (2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1))


# ---- checks shared by the CPU and the GPU tests ---------------------------

def check_solver_table(n, nb, dtype, device, method):
    """Every uplo x op x diag of one (n, nb, dtype): the residual bound, and
    that x beyond the call is untouched in shape and dtype."""
    from dlaf_amd import TriangularVectorSolver
    b = rhs(n, dtype)
    for uplo in UPLOS:
        for diag in DIAGS:
            t = make_triangular(n, dtype, uplo, diag)
            A = to_matrix(stored_with_garbage(t, uplo, diag), nb, device)
            sv = TriangularVectorSolver(uplo, diag, A, method=method)
            assert sv.method == method
            for op in OPS:
                x = torch.from_numpy(np.array(b)).to(device)
                assert sv.solve(op, x) is x
                ratio = solve_ratio(t, op, b, x.cpu().numpy(), dtype)
                print(f"n={n} nb={nb} {dtype} {uplo.value}{op.value}"
                      f"{diag.value} ratio={ratio:.4f}")
                assert ratio <= SOLVE_C, (uplo, op, diag, ratio)


def spd_truth(kind, n, dtype):
    """(||A||_1, ||A^-1||_1) of the stored numbers."""
    a = make_spd(kind, n, dtype)
    return norm1(a.astype(wide(dtype))), inv_norm1(a)


def cholesky_rcond_of(a, nb, uplo, device="cpu", grid=None, method="auto"):
    """(rcond estimate, the factor's Matrix, anorm) by the library's route:
    norm, factorization, estimate."""
    from dlaf_amd import (matrix_norm, cholesky_factorization,
                          cholesky_rcond)
    mat = to_matrix(a, nb, device, grid)
    anorm = matrix_norm("one", mat, structure="hermitian", uplo=uplo,
                        grid=grid)
    cholesky_factorization(uplo, mat, grid)
    return cholesky_rcond(uplo, mat, anorm, grid, method), mat, anorm


def check_rcond_table(n, nb, dtype, device, method):
    """The band for every SPD kind x uplo and every triangular uplo x diag x
    norm of one (n, nb, dtype)."""
    from dlaf_amd import triangular_rcond
    for kind in SPD_KINDS:
        an, ai = spd_truth(kind, n, dtype)
        for uplo in UPLOS:
            est, _, anorm = cholesky_rcond_of(make_spd(kind, n, dtype), nb,
                                              uplo, device, method=method)
            assert abs(anorm - an) <= 4 * (n + 2) * eps_of(dtype) * an
            print(f"{kind} n={n} {dtype} {uplo.value} est/true="
                  f"{est * an * ai:.6f}")
            check_band(est, an, ai, n, dtype)
    for uplo in UPLOS:
        for diag in DIAGS:
            t = make_triangular(n, dtype, uplo, diag)
            A = to_matrix(stored_with_garbage(t, uplo, diag), nb, device)
            for norm in ("one", "inf"):
                tt = t if norm == "one" else t.T
                an, ai = norm1(tt.astype(wide(dtype))), inv_norm1(tt)
                est = triangular_rcond(norm, uplo, diag, A, method=method)
                print(f"tri n={n} {dtype} {uplo.value}{diag.value} {norm} "
                      f"est/true={est * an * ai:.6f}")
                check_band(est, an, ai, n, dtype)


def solve_tol(dtype: str, n: int) -> float:
    """The bound style of tests/test_triangular.py: absolute error against
    the dense solve of a well-conditioned system."""
    base = 2e-4 if eps_of(dtype) > 1e-10 else 5e-10
    return base * max(1, n)


def check_cholesky_solve(n, nb, nrhs, dtype, uplo, device="cpu", grid=None):
    from dlaf_amd import cholesky_factorization, cholesky_solve
    a = make_spd("diagdom", n, dtype)
    b = _frozen(_random(_rng(n, dtype, 41), (n, nrhs), dtype), dtype)
    L = to_matrix(a, nb, device, grid)
    B = to_matrix(b, nb, device, grid)
    cholesky_factorization(uplo, L, grid)
    cholesky_solve(uplo, L, B, grid)
    want = np.linalg.solve(a.astype(wide(dtype)), b.astype(wide(dtype)))
    err = np.abs(B.to_global().cpu().numpy() - want).max()
    print(f"potrs n={n} {dtype} {uplo.value} err={err:.3e}")
    assert err < solve_tol(dtype, n + nrhs), err
    return err
