"""Condition estimates (triangular_rcond, cholesky_rcond), the vector solver's
"blocked" method, cholesky_solve and the warn_b_rcond keyword on the CPU.
Matrices, truths and bounds: cond_cases.py."""

import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

from dlaf_amd import (  # noqa: E402
    Matrix, CommGrid, UpLo, Op, Diag, matrix_norm, cholesky_factorization,
    TriangularVectorSolver, inverse_norm_estimate, triangular_rcond,
    cholesky_rcond, cholesky_solve, hermitian_generalized_eigensolver,
    hermitian_generalized_eigenvalues,
)
from dlaf_amd.core.asserts import DlafAssertError  # noqa: E402


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_blocked_vector_solve_residual(shape, dtype):
    cc.check_solver_table(shape[0], shape[1], dtype, "cpu", "blocked")


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.RCOND_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_rcond_band(shape, dtype):
    cc.check_rcond_table(shape[0], shape[1], dtype, "cpu", "auto")


@pytest.mark.parametrize("shape", cc.RCOND_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_rcond_equals_lapack(shape):
    """float64, kappa_1 <= 1e4: the same number as dpocon / dtrcon."""
    lapack = pytest.importorskip("scipy").linalg.lapack
    n, nb = shape
    compared = 0
    for kind in cc.SPD_KINDS:
        an, ai = cc.spd_truth(kind, n, "float64")
        if an * ai > 1e4:
            continue
        for uplo in cc.UPLOS:
            est, fac, anorm = cc.cholesky_rcond_of(
                cc.make_spd(kind, n, "float64"), nb, uplo)
            ref, info = lapack.dpocon(fac.to_global().numpy(), anorm,
                                      uplo=uplo.value)
            assert info == 0
            assert abs(est - ref) <= 1e-8 * ref, (kind, uplo, est, ref)
            compared += 1
    for uplo in cc.UPLOS:
        for diag in cc.DIAGS:
            t = cc.make_triangular(n, "float64", uplo, diag)
            A = cc.to_matrix(cc.stored_with_garbage(t, uplo, diag), nb)
            for norm, ch in (("one", "1"), ("inf", "I")):
                tt = t if norm == "one" else t.T
                if cc.norm1(tt) * cc.inv_norm1(tt) > 1e4:
                    continue
                est = triangular_rcond(norm, uplo, diag, A)
                ref, info = lapack.dtrcon(np.asfortranarray(t), norm=ch,
                                          uplo=uplo.value, diag=diag.value)
                assert info == 0
                assert abs(est - ref) <= 1e-8 * ref, (uplo, diag, norm, est,
                                                      ref)
                compared += 1
    assert compared > 0


def test_toeplitz_closed_form():
    """||A||_1 = 4, ||A^-1||_1 = 300: rcond = 1 / 1200."""
    a = cc.toeplitz(48)
    assert abs(cc.inv_norm1(a) - 300.0) < 1e-9
    est, _, anorm = cc.cholesky_rcond_of(a, 16, UpLo.Lower)
    assert anorm == 4.0
    assert abs(est * 1200.0 - 1.0) <= 1e-12


def test_singular_triangular_gives_zero():
    t = np.array(cc.make_triangular(40, "float64", UpLo.Lower, Diag.NonUnit))
    t[23, 23] = 0.0
    A = cc.to_matrix(t, 16)
    assert triangular_rcond("one", UpLo.Lower, Diag.NonUnit, A) == 0.0
    assert triangular_rcond("inf", UpLo.Lower, Diag.NonUnit, A) == 0.0
    # the stored diagonal does not count under Diag.Unit
    assert triangular_rcond("one", UpLo.Lower, Diag.Unit, A) > 0.0


def test_empty_matrix():
    A = Matrix.create(0, 0, 16, 16)
    assert triangular_rcond("one", UpLo.Lower, Diag.NonUnit, A) == 1.0
    assert cholesky_rcond(UpLo.Lower, A, 0.0) == 1.0
    x = torch.zeros(0, dtype=torch.float64)
    TriangularVectorSolver(UpLo.Lower, Diag.NonUnit, A).solve(Op.NoTrans, x)


def test_zero_anorm_gives_zero():
    _, fac, _ = cc.cholesky_rcond_of(cc.make_spd("diagdom", 17, "float64"), 16,
                                     UpLo.Lower)
    assert cholesky_rcond(UpLo.Lower, fac, 0.0) == 0.0


def test_inverse_norm_estimate_with_plain_callables():
    """The estimator alone, on a dense inverse: n = 1 and a general n."""
    for n in (1, 2, 33):
        a = cc.make_spd("wishart", n, "complex128")
        inv = torch.from_numpy(np.linalg.inv(a))

        def solve(x):
            x.copy_(inv @ x)

        def solve_h(x):
            x.copy_(inv.mH @ x)

        est = inverse_norm_estimate(n, solve, solve_h, torch.complex128,
                                    "cpu")
        true = cc.inv_norm1(a)
        assert true / 3 <= est <= true * (1 + 1e-10), (n, est, true)


def test_kernel_method_on_cpu_raises():
    A = cc.to_matrix(cc.make_triangular(17, "float64", UpLo.Lower,
                                        Diag.NonUnit), 16)
    with pytest.raises(DlafAssertError):
        TriangularVectorSolver(UpLo.Lower, Diag.NonUnit, A, method="kernel")
    with pytest.raises(DlafAssertError):
        triangular_rcond("one", UpLo.Lower, Diag.NonUnit, A, method="kernel")
    assert TriangularVectorSolver(UpLo.Lower, Diag.NonUnit, A).method == "blocked"


def _worker_rcond(rank, ws):
    grid = CommGrid(1, 2)
    a = cc.make_spd("wishart", 96, "float64")
    est, _, _ = cc.cholesky_rcond_of(a, 32, UpLo.Lower, grid=grid)
    t = cc.make_triangular(96, "float64", UpLo.Upper, Diag.NonUnit)
    A = cc.to_matrix(cc.stored_with_garbage(t, UpLo.Upper, Diag.NonUnit), 32,
                     grid=grid)
    return est, triangular_rcond("inf", UpLo.Upper, Diag.NonUnit, A, grid)


@pytest.mark.timeout(300)
def test_rcond_two_ranks():
    outs = run_distributed(_worker_rcond, 2)
    assert outs[0] == outs[1]
    an, ai = cc.spd_truth("wishart", 96, "float64")
    cc.check_band(outs[0][0], an, ai, 96, "float64")
    t = cc.make_triangular(96, "float64", UpLo.Upper, Diag.NonUnit).T
    cc.check_band(outs[0][1], cc.norm1(t), cc.inv_norm1(t), 96, "float64")


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, ids=lambda u: u.value)
def test_cholesky_solve(uplo, dtype):
    cc.check_cholesky_solve(100, 32, 3, dtype, uplo)


def _worker_potrs(rank, ws):
    grid = CommGrid(1, 2)
    return cc.check_cholesky_solve(100, 32, 3, "float64", UpLo.Lower,
                                   grid=grid)


@pytest.mark.timeout(300)
def test_cholesky_solve_two_ranks():
    run_distributed(_worker_potrs, 2)


# ---- warn_b_rcond ----------------------------------------------------------

def _gen_problem(n, nb, b_global):
    a = cc.make_spd("wishart", n, "float64")
    return cc.to_matrix(a, nb), cc.to_matrix(b_global, nb)


def _ill_b(n):
    """Diagonal B with kappa = 1e17: its Cholesky factor exists exactly."""
    return np.diag(np.logspace(0.0, -17.0, n))


@pytest.mark.parametrize("driver", ["eigensolver", "eigenvalues"])
def test_warn_b_rcond(driver):
    n, nb = 24, 8

    def run(b_global, **kw):
        A, B = _gen_problem(n, nb, b_global)
        if driver == "eigensolver":
            w, ev = hermitian_generalized_eigensolver(UpLo.Lower, A, B, **kw)
            return w, ev.to_global(), B.to_global()
        w = hermitian_generalized_eigenvalues(UpLo.Lower, A, B, **kw)
        return w, B.to_global()

    with pytest.warns(RuntimeWarning, match="rcond") as rec:
        run(_ill_b(n), warn_b_rcond=True)
    assert any("B is ill-conditioned" in str(r.message) for r in rec)

    good = cc.make_spd("diagdom", n, "float64")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        on = run(good, warn_b_rcond=True)
        off = run(good, warn_b_rcond=False)
        default = run(good)
        run(_ill_b(n))  # keyword off: silent whatever B is
    # the estimate only reads the factor: identical bits with, without and
    # by default
    for x, y, z in zip(on, off, default):
        assert torch.equal(x, y) and torch.equal(y, z)
