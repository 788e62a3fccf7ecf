"""The triangular-vector-solve kernel (csrc/trsv.hip) and, on top of it, the
condition estimates on the device. The (n, nb) of cond_cases.SOLVE_SHAPES are
the smallest that reach one tile, a partial last tile, misaligned tile bases
(nb=17 in float32 / complex64: the scalar path), two and three tile steps in
both sweep directions, and a tile of several workgroup strips and column
blocks with a ragged last one (nb=160). Bounds and matrices: cond_cases.py."""

import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402

from dlaf_amd import (  # noqa: E402
    Matrix, UpLo, Op, Diag, TriangularVectorSolver, triangular_rcond,
    hermitian_generalized_eigenvalues,
)
from dlaf_amd.ops._ext import get_ext  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_OPC = {Op.NoTrans: 0, Op.Trans: 1, Op.ConjTrans: 2}
_ids = dict(ids=lambda s: f"{s[0]}-{s[1]}")


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, **_ids)
def test_kernel_solve_residual(shape, dtype):
    cc.check_solver_table(shape[0], shape[1], dtype, DEV, "kernel")


def _raw_solve(sv, storage, dinv, b, op):
    """The kernel on a padded copy of b; returns the whole padded vector."""
    d = sv.A.dist
    xp = torch.zeros(d.nr_tiles[0] * d.nb, dtype=sv.A.dtype, device=DEV)
    xp[: sv.n] = torch.from_numpy(np.array(b)).to(DEV)
    get_ext().trsv_tiles(storage, dinv, xp, sv.n, int(sv.uplo == UpLo.Upper),
                         _OPC[op])
    return xp


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, **_ids)
def test_kernel_repeatable_and_padding(shape, dtype):
    """Two calls on the same data give the same bits; the padded tail of x
    stays zero and nothing stored in the padding of the tiles (or of the
    diagonal inverses) reaches the logical part."""
    n, nb = shape
    b = cc.rhs(n, dtype)
    for uplo in cc.UPLOS:
        for diag in cc.DIAGS:
            t = cc.make_triangular(n, dtype, uplo, diag)
            A = cc.to_matrix(cc.stored_with_garbage(t, uplo, diag), nb, DEV)
            sv = TriangularVectorSolver(uplo, diag, A, method="kernel")
            nt = A.dist.nr_tiles[0]
            pad = nt * nb - n
            # the same tiles with NaN all over the padding
            dirty, dinv = sv._storage.clone(), sv._dinv.clone()
            if pad:
                dirty[nt - 1, :, nb - pad:, :] = float("nan")
                dirty[:, nt - 1, :, nb - pad:] = float("nan")
                dinv[nt - 1, nb - pad:, :] = float("nan")
                dinv[nt - 1, :, nb - pad:] = float("nan")
            for op in cc.OPS:
                x1 = _raw_solve(sv, sv._storage, sv._dinv, b, op)
                x2 = _raw_solve(sv, sv._storage, sv._dinv, b, op)
                x3 = _raw_solve(sv, dirty, dinv, b, op)
                assert torch.equal(x1, x2), (uplo, op, diag)
                assert torch.equal(x1, x3), (uplo, op, diag)
                assert not bool(x1[n:].any()), (uplo, op, diag)
                via = torch.from_numpy(np.array(b)).to(DEV)
                sv.solve(op, via)
                assert torch.equal(via, x1[:n])


@pytest.mark.parametrize("dtype", ["float32", "float64", "complex64"])
def test_unaligned_storage_takes_scalar_path(dtype):
    """A storage (and inverses) starting 4 or 8 bytes into the allocation
    cannot use 16-byte loads; the result is the one of the aligned storage."""
    n, nb = 100, 32
    b = cc.rhs(n, dtype)
    for uplo in cc.UPLOS:
        t = cc.make_triangular(n, dtype, uplo, Diag.NonUnit)
        A = cc.to_matrix(cc.stored_with_garbage(t, uplo, Diag.NonUnit), nb,
                         DEV)
        sv = TriangularVectorSolver(uplo, Diag.NonUnit, A, method="kernel")

        def shifted(src):
            flat = torch.zeros(src.numel() + 1, dtype=src.dtype, device=DEV)
            flat[1:] = src.reshape(-1)
            out = flat[1:].view(src.shape)
            assert out.data_ptr() % 16 != 0
            return out

        st, dv = shifted(sv._storage), shifted(sv._dinv)
        for op in cc.OPS:
            want = _raw_solve(sv, sv._storage, sv._dinv, b, op)
            assert torch.equal(_raw_solve(sv, st, sv._dinv, b, op), want)
            assert torch.equal(_raw_solve(sv, sv._storage, dv, b, op), want)


def test_empty_storage_launches_nothing():
    st = torch.zeros((0, 0, 16, 16), dtype=torch.float64, device=DEV)
    dinv = torch.zeros((0, 16, 16), dtype=torch.float64, device=DEV)
    x = torch.zeros(0, dtype=torch.float64, device=DEV)
    get_ext().trsv_tiles(st, dinv, x, 0, 0, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.RCOND_SHAPES, **_ids)
def test_rcond_band_kernel(shape, dtype):
    cc.check_rcond_table(shape[0], shape[1], dtype, DEV, "kernel")


def test_auto_picks_the_kernel_on_the_device():
    t = cc.make_triangular(40, "float64", UpLo.Lower, Diag.NonUnit)
    A = cc.to_matrix(t, 16, DEV)
    assert TriangularVectorSolver(UpLo.Lower, Diag.NonUnit, A).method == "kernel"
    est = triangular_rcond("one", UpLo.Lower, Diag.NonUnit, A)
    cc.check_band(est, cc.norm1(t), cc.inv_norm1(t), 40, "float64")


def test_toeplitz_closed_form_kernel():
    est, _, anorm = cc.cholesky_rcond_of(cc.toeplitz(48), 16, UpLo.Lower, DEV,
                                         method="kernel")
    assert anorm == 4.0
    assert abs(est * 1200.0 - 1.0) <= 1e-12


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, ids=lambda u: u.value)
def test_cholesky_solve_device(uplo, dtype):
    cc.check_cholesky_solve(100, 32, 3, dtype, uplo, DEV)


def test_warn_b_rcond_device():
    n, nb = 96, 32
    a = cc.make_spd("wishart", n, "float64")

    def run(b, **kw):
        A, B = cc.to_matrix(a, nb, DEV), cc.to_matrix(b, nb, DEV)
        return hermitian_generalized_eigenvalues(UpLo.Lower, A, B, **kw)

    with pytest.warns(RuntimeWarning, match="B is ill-conditioned"):
        run(np.diag(np.logspace(0.0, -17.0, n)), warn_b_rcond=True)
    good = cc.make_spd("diagdom", n, "float64")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert torch.equal(run(good, warn_b_rcond=True), run(good))
