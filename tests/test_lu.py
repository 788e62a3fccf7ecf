"""LU with partial pivoting, its solves and its condition estimate on the CPU
twin of the panel kernel. Matrices, references and bounds: lu_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
import lu_cases as lc  # noqa: E402

from dlaf_amd import (  # noqa: E402
    CommGrid, Matrix, Op, lu_factorization, lu_solve, general_solve, lu_rcond,
    matrix_norm,
)
from dlaf_amd.core.asserts import DlafAssertError  # noqa: E402
from dlaf_amd.ops import tile_ops as ops  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

_ids = dict(ids=lambda s: f"{s[0]}-{s[1]}")


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES, **_ids)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_factor(kind, shape, dtype):
    n, nb = shape
    lc.check_factor(("kind", kind, n, dtype), nb, "cpu",
                    pivots_must_match=kind != "random")


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_factor_big_tile(dtype):
    lc.check_factor(("kind", "scrambled", lc.BIG[0], dtype), lc.BIG[1], "cpu")


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", [(40, 16), (70, 17), (165, 40)], **_ids)
def test_singular(shape, dtype):
    lc.check_singular(shape[0], shape[1], dtype, "cpu")


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES + [lc.BIG], **_ids)
def test_solve(shape, dtype):
    lc.check_solve(shape[0], shape[1], dtype, "cpu")


def test_solve_wide_rhs_takes_interchanges():
    """70 right-hand sides: the row interchanges run column-parallel."""
    lc.check_solve(100, 32, "float64", "cpu", nrhs_list=(70,))


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES + [lc.BIG], **_ids)
def test_rcond_band(shape, dtype):
    for kind in ("scrambled", "random"):
        lc.check_rcond(kind, shape[0], shape[1], dtype, "cpu")


@pytest.mark.parametrize("shape", [(40, 16), (100, 32), (165, 40), lc.BIG],
                         **_ids)
def test_rcond_equals_lapack(shape):
    lapack = pytest.importorskip("scipy").linalg.lapack
    n, nb = shape
    for dtype, gecon in (("float64", lapack.dgecon),
                         ("complex128", lapack.zgecon)):
        A, norms, est = lc.check_rcond("scrambled", n, nb, dtype, "cpu")
        f = A.to_global().numpy()
        for nm, key in (("one", "1"), ("inf", "I")):
            ref, info = gecon(f, norms[nm], norm=key)
            assert info == 0
            assert abs(est[nm] - ref) <= 1e-8 * ref, (dtype, nm, est[nm], ref)


def test_toeplitz_closed_form():
    lc.check_toeplitz("cpu")


def test_empty_and_one():
    A = Matrix.create(0, 0, 16, 16)
    ipiv, info = lu_factorization(A)
    assert ipiv.shape == (0,) and ipiv.dtype == torch.int32 and info == 0
    assert lu_rcond("one", A, 0.0) == 1.0
    B = Matrix.create(0, 3, 16, 16)
    lu_solve(Op.NoTrans, A, ipiv, B)
    assert general_solve(A, B)[1] == 0
    for dtype in lc.DTYPES:
        a = np.array([[-4.0]]).astype(dtype)
        A = cc.to_matrix(a, 16)
        ipiv, info = lu_factorization(A)
        assert info == 0 and ipiv.tolist() == [0]
        assert A.to_global()[0, 0] == -4.0
        lc.check_padding(A)
        assert lu_rcond("one", A, 4.0) == 1.0
        B = cc.to_matrix(np.array([[2.0, 8.0]]).astype(dtype), 16)
        lu_solve(Op.ConjTrans, A, ipiv, B)
        assert B.to_global().tolist() == [[-0.5, -2.0]]
    Z = cc.to_matrix(np.zeros((1, 1)), 16)
    assert lu_factorization(Z)[1] == 1
    assert lu_rcond("one", Z, 0.0) == 0.0


def test_rejected_arguments():
    with pytest.raises(DlafAssertError):
        lu_factorization(Matrix.create(32, 48, 16, 16))
    with pytest.raises(DlafAssertError):
        lu_factorization(Matrix.create(32, 32, 16, 8))
    a = lc.make("scrambled", 40, "float64")
    A, ipiv, _ = lc.factor(a, 16, "cpu")
    with pytest.raises(DlafAssertError):
        lu_rcond("fro", A, 1.0)
    with pytest.raises(DlafAssertError, match="kernel"):
        lu_rcond("one", A, 1.0, method="kernel")
    with pytest.raises(DlafAssertError):
        lu_solve(Op.NoTrans, A, ipiv, Matrix.create(32, 2, 16, 16))
    with pytest.raises(DlafAssertError):
        lu_solve(Op.NoTrans, A, ipiv.to(torch.int64),
                 Matrix.create(40, 2, 16, 16))


def test_twin_pivot_rule_first_maximum():
    """CABS1 and the lowest row on ties, where the modulus would choose
    otherwise: |3 + 3i| < 6, but CABS1 ties them at 6."""
    sq = np.eye(4, dtype=np.complex128)
    sq[:, 0] = [1.0, 4.5, 3.0 + 3.0j, 6.0]
    A = cc.to_matrix(sq, 4)
    ipiv, _ = lu_factorization(A)
    assert int(ipiv[0]) == 2  # rows 2 and 3 tie at 6: the lower index wins
    st = torch.zeros((1, 1, 4, 4), dtype=torch.float64)
    st[0, 0, :, 0] = torch.tensor([1.0, -2.0, 2.0, 0.5])
    piv = torch.zeros(4, dtype=torch.int32)
    ops.lu_panel(st, 4, 0, piv, torch.zeros(1, dtype=torch.int32))
    assert int(piv[0]) == 1


def test_laswp_twin_roundtrip():
    rng = np.random.default_rng(5)
    for n, nb, ncols in ((70, 17, 3), (70, 17, 70)):
        b = rng.uniform(-1, 1, (n, ncols))
        B = cc.to_matrix(b, nb)
        piv = torch.tensor([rng.integers(j, n) for j in range(n)],
                           dtype=torch.int32)
        before = B.storage.clone()
        ops.laswp(B.storage, piv, 0, n, 0, ncols)
        want = np.array(b)
        for j, p in enumerate(piv.tolist()):
            want[[j, p]] = want[[p, j]]
        assert np.array_equal(B.to_global().numpy(), want)
        perm = ops.pivots_to_permutation(piv).numpy()
        assert np.array_equal(b[perm], want)
        ops.laswp(B.storage, piv, 0, n, 0, ncols, reverse=True)
        assert torch.equal(B.storage, before)
        # a column range leaves the other columns alone
        if ncols > 3:
            ops.laswp(B.storage, piv, 3, 40, 20, 55)
            got = B.to_global().numpy()
            assert np.array_equal(got[:, :20], b[:, :20])
            assert np.array_equal(got[:, 55:], b[:, 55:])
            part = np.array(b[:, 20:55])
            for j in range(3, 40):
                p = int(piv[j])
                part[[j, p]] = part[[p, j]]
            assert np.array_equal(got[:, 20:55], part)


def _dist_worker(rank, ws):
    grid = CommGrid(1, 2)
    A = Matrix.create(32, 32, 8, 8, dtype=torch.float64, grid=grid)
    B = Matrix.create(32, 2, 8, 8, dtype=torch.float64, grid=grid)
    msgs = []
    for call in (lambda: lu_factorization(A, grid),
                 lambda: general_solve(A, B, grid),
                 lambda: lu_rcond("one", A, 1.0, grid),
                 lambda: lu_solve(Op.NoTrans, A,
                                  torch.zeros(32, dtype=torch.int32), B,
                                  grid)):
        try:
            call()
        except DlafAssertError as err:
            msgs.append(str(err))
        else:
            msgs.append(None)
    return msgs


def test_distributed_grid_rejected():
    for msgs in run_distributed(_dist_worker, 2):
        for m in msgs:
            assert m is not None and "distributed" in m
