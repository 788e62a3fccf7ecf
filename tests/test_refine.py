"""cholesky_refine, cholesky_solve_expert and cholesky_solve_mixed on the CPU
(method "blocked"), against LAPACK's ?posvx (fact='N') through scipy, and on a
2-rank gloo grid. Matrices and bounds: refine_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch
from scipy.linalg import lapack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
import refine_cases as rc  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

from dlaf_amd import (  # noqa: E402
    Matrix, UpLo, HermitianVectorProduct, cholesky_refine,
    cholesky_solve_expert, cholesky_solve_mixed,
)

_ids = dict(ids=lambda s: f"{s[0]}-{s[1]}")
_uids = dict(ids=lambda u: u.value)
_POSVX = {"float32": lapack.sposvx, "float64": lapack.dposvx,
          "complex64": lapack.cposvx, "complex128": lapack.zposvx}


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, **_ids)
def test_blocked_product(shape, dtype):
    """The fallback product and its CABS1 copy, on clean storage (the other
    triangle still holds garbage)."""
    n, nb = shape
    for uplo in cc.UPLOS:
        a = np.array(cc.make_spd("wishart", n, dtype))
        i, j = np.indices((n, n))
        a[(j > i) if uplo == UpLo.Lower else (j < i)] = 1e30
        hv = HermitianVectorProduct(uplo, cc.to_matrix(a, nb))
        assert hv.method == "blocked"
        x = torch.from_numpy(np.array(rc.vector(n, dtype)))
        y, yabs = hv.apply(x, want_abs=True)
        assert y.dtype == x.dtype and not yabs.is_complex()
        rc.check_product(y.numpy(), yabs.numpy(), "wishart", n, dtype)
        assert torch.equal(hv.apply(x), y)


def test_kernel_needs_the_device():
    A = cc.to_matrix(cc.make_spd("wishart", 7, "float64"), 16)
    with pytest.raises(Exception):
        HermitianVectorProduct(UpLo.Lower, A, method="kernel")


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("kind", cc.SPD_KINDS)
@pytest.mark.parametrize("shape", rc.REFINE_SHAPES, **_ids)
def test_refine_against_posvx(shape, kind, dtype):
    n, nb = shape
    a, b = cc.make_spd(kind, n, dtype), rc.rhs_block(n, dtype)
    for uplo in cc.UPLOS:
        x, ferr, berr = rc.run_refine(kind, n, nb, dtype, uplo, "cpu",
                                      "blocked")
        rc.check_bounds(x, ferr, berr, kind, n, dtype)
        ref = _POSVX[dtype](a, b, fact="N", lower=int(uplo == UpLo.Lower))
        ferr_ref, berr_ref, info = ref[7], ref[8], ref[9]
        assert info == 0
        assert (berr.numpy() <= np.maximum(4 * berr_ref,
                                           rc.np_eps(dtype))).all()
        rc.check_band(ferr.numpy(), ferr_ref)
        # (d): one entry pushed off by 1e3 eps ||x|| is refined away
        x, ferr, berr = rc.run_refine(kind, n, nb, dtype, uplo, "cpu",
                                      "blocked", perturb=True)
        rc.check_bounds(x, ferr, berr, kind, n, dtype)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, **_ids)
def test_expert_against_posvx(shape, dtype):
    """The whole table of refine_cases.FERR_RATIO_BLOCKED: rcond as dpocon
    has it, berr and the ferr band."""
    n, nb = shape
    for kind in cc.SPD_KINDS:
        a, b = cc.make_spd(kind, n, dtype), rc.rhs_block(n, dtype)
        for uplo in cc.UPLOS:
            X, L, rcond, ferr, berr, info = cholesky_solve_expert(
                uplo, cc.to_matrix(a, nb), cc.to_matrix(b, nb))
            ref = _POSVX[dtype](a, b, fact="N", lower=int(uplo == UpLo.Lower))
            rcond_ref, ferr_ref, berr_ref = ref[6], ref[7], ref[8]
            assert info == 0 and ref[9] == 0
            if dtype == "float64":
                # as test_condition.py holds cholesky_rcond to dpocon
                assert abs(rcond - rcond_ref) <= 1e-10 * rcond_ref
            assert (berr.numpy() <= np.maximum(4 * berr_ref,
                                               rc.np_eps(dtype))).all()
            rc.check_band(ferr.numpy(), ferr_ref)
            rc.check_bounds(X.to_global().numpy(), ferr, berr, kind, n, dtype)


def test_expert_is_its_parts():
    rc.check_expert("cpu", "blocked")


def test_expert_flags_a_singular_matrix():
    n, nb = 40, 16
    a = np.diag(np.logspace(0.0, -18.0, n))
    out = cholesky_solve_expert(UpLo.Lower, cc.to_matrix(a, nb),
                                cc.to_matrix(np.ones((n, 1)), nb))
    assert out[5] == n + 1 and out[2] < 2.0 ** -53 and out[0] is not None


def test_empty():
    A = Matrix.create(0, 0, 16, 16)
    B = Matrix.create(0, 3, 16, 16)
    ferr, berr = cholesky_refine(UpLo.Lower, A, A.clone(), B, B.clone())
    assert ferr.tolist() == [0.0] * 3 and berr.tolist() == [0.0] * 3
    A = cc.to_matrix(cc.make_spd("wishart", 7, "float64"), 16)
    B = Matrix.create(7, 0, 16, 16)
    ferr, berr = cholesky_refine(UpLo.Lower, A, A.clone(), B, B.clone())
    assert ferr.numel() == 0 and berr.numel() == 0
    assert cholesky_solve_mixed(UpLo.Lower, A, B)[1:] == (0, 0)


@pytest.mark.parametrize("dtype", rc.MIXED_DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, **_uids)
@pytest.mark.parametrize("kind", cc.SPD_KINDS)
@pytest.mark.parametrize("shape", rc.REFINE_SHAPES, **_ids)
def test_mixed_converges(shape, kind, uplo, dtype):
    rc.check_mixed_spd(kind, shape[0], shape[1], dtype, uplo, "cpu")


@pytest.mark.parametrize("dtype", rc.MIXED_DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, **_uids)
def test_mixed_falls_back(uplo, dtype):
    rc.check_mixed_fallback(dtype, uplo, "cpu")
    rc.check_mixed_overflow(dtype, uplo, "cpu")


def test_mixed_rejects_single_precision():
    A = cc.to_matrix(cc.make_spd("wishart", 7, "float32"), 16)
    with pytest.raises(Exception):
        cholesky_solve_mixed(UpLo.Lower, A, A.clone())


def test_mixed_reports_a_failed_pivot():
    n, nb = 40, 16
    a = np.array(cc.make_spd("wishart", n, "float64"))
    a[10, 10] = -1.0
    X, iters, info = cholesky_solve_mixed(
        UpLo.Lower, cc.to_matrix(a, nb), cc.to_matrix(np.ones((n, 2)), nb))
    assert X is None and iters == -3 and info == 11


def test_astype_keeps_distribution_and_padding():
    A = cc.to_matrix(cc.make_spd("wishart", 40, "float64"), 17)
    S = A.astype(torch.float32)
    assert S.dtype == torch.float32 and S.dist is A.dist
    assert torch.equal(S.storage, A.storage.to(torch.float32))
    assert torch.equal(S.astype(torch.float64).storage[-1, -1, 6:, 6:],
                       A.storage[-1, -1, 6:, 6:])  # the identity padding
    S.storage.zero_()
    assert bool(A.storage.any())  # a copy


def _worker_two_ranks(rank, ws):
    from dlaf_amd import CommGrid
    grid = CommGrid(1, 2)
    n, nb, dtype = 100, 32, "float64"
    x, ferr, berr = rc.run_refine("wishart", n, nb, dtype, UpLo.Lower, "cpu",
                                  "auto", grid=grid)
    rc.check_bounds(x, ferr, berr, "wishart", n, dtype)
    a, b = cc.make_spd("graded", n, dtype), rc.rhs_block(n, dtype)
    xm, iters, info = rc.run_mixed(a, b, nb, UpLo.Lower, "cpu", grid=grid)
    assert info == 0 and 0 <= iters <= 8 and rc.mixed_criterion(a, b, xm)
    return ferr.tolist(), berr.tolist(), iters


@pytest.mark.timeout(300)
def test_two_ranks_agree():
    outs = run_distributed(_worker_two_ranks, 2)
    assert outs[0] == outs[1]
    rc.check_band(outs[0][0],
                  rc.blocked_ferr("wishart", 100, 32, "float64", UpLo.Lower))
