"""The pivoted panel and interchange kernels (csrc/lu_panel.hip) and the LU
drivers on the device. The (n, nb) of lu_cases.SHAPES are the smallest that
reach one tile, a partial last tile, nb below the inner block width (16, 17),
nb not a multiple of it (40), a misaligned tile base (nb = 17 in float32 /
complex64), a pivot row in a later tile than the top row (every multi-tile
scrambled / planted case), and, with lu_cases.BIG, several inner blocks per
tile over more than one workgroup of row locations. Matrices, references and
bounds: lu_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
import lu_cases as lc  # noqa: E402

from dlaf_amd import lu_factorization  # noqa: E402
from dlaf_amd.ops import tile_ops as ops  # noqa: E402
from dlaf_amd.ops._ext import get_ext  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ids = dict(ids=lambda s: f"{s[0]}-{s[1]}")


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES, **_ids)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_factor(kind, shape, dtype):
    n, nb = shape
    lc.check_factor(("kind", kind, n, dtype), nb, DEV,
                    pivots_must_match=kind != "random")


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_factor_big_tile(dtype):
    lc.check_factor(("kind", "scrambled", lc.BIG[0], dtype), lc.BIG[1], DEV)


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", [(40, 16), (70, 17), (165, 40)], **_ids)
def test_singular(shape, dtype):
    lc.check_singular(shape[0], shape[1], dtype, DEV)


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", lc.SHAPES + [lc.BIG], **_ids)
def test_solve(shape, dtype):
    lc.check_solve(shape[0], shape[1], dtype, DEV)


def test_solve_wide_rhs_takes_interchanges():
    lc.check_solve(100, 32, "float64", DEV, nrhs_list=(70,))


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", [(1, 16), (70, 17), (165, 40), lc.BIG],
                         **_ids)
def test_rcond_band_kernel(shape, dtype):
    for kind in ("scrambled", "random"):
        lc.check_rcond(kind, shape[0], shape[1], dtype, DEV, method="kernel")


def test_toeplitz_closed_form():
    lc.check_toeplitz(DEV, method="kernel")


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", [(70, 17), (165, 40), lc.BIG], **_ids)
def test_repeatable_and_matches_twin(shape, dtype):
    """Two runs give the same bits, ipiv included, and the pivots of the CPU
    twin."""
    n, nb = shape
    for kind in ("scrambled", "random") if n > 200 else lc.KINDS:
        a = lc.make(kind, n, dtype)
        A1, p1, i1 = lc.factor(a, nb, DEV)
        A2, p2, i2 = lc.factor(a, nb, DEV)
        assert i1 == i2 == 0
        assert torch.equal(p1, p2)
        assert torch.equal(A1.storage, A2.storage)
        if kind != "random":
            _, pc, _ = lc.factor(a, nb, "cpu")
            assert torch.equal(p1.cpu(), pc)


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("shape", [(70, 17), (165, 40), lc.BIG], **_ids)
def test_padding_below_the_matrix_is_never_read(shape, dtype):
    """NaN in the padding rows of the last tile row changes no bit of ipiv or
    of the factors."""
    n, nb = shape
    a = lc.make("scrambled", n, dtype)
    A1, p1, _ = lc.factor(a, nb, DEV)
    A2 = cc.to_matrix(a, nb, DEV)
    nt = A2.dist.nr_tiles[0]
    pad = nt * nb - n
    assert pad > 0
    A2.storage[nt - 1, :, nb - pad:, :] = float("nan")
    p2, info = lu_factorization(A2)
    assert info == 0
    assert torch.equal(p1, p2)
    assert torch.equal(A1.to_global(), A2.to_global())
    A2._set_identity_pad()
    assert torch.equal(A1.storage, A2.storage)


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_laswp_forward_then_reverse(dtype):
    rng = np.random.default_rng(17)
    n, nb = 165, 40
    piv = torch.tensor([rng.integers(j, n) for j in range(n)],
                       dtype=torch.int32)
    for ncols in (3, n):
        b = lc.rhs(n, 3, dtype) if ncols == 3 else lc.make("random", n, dtype)
        B = cc.to_matrix(b, nb, DEV)
        Bc = cc.to_matrix(b, nb, "cpu")
        before = B.storage.clone()
        ops.laswp(B.storage, piv.to(DEV), 0, n, 0, ncols)
        ops.laswp(Bc.storage, piv, 0, n, 0, ncols)
        assert torch.equal(B.storage.cpu(), Bc.storage)
        ops.laswp(B.storage, piv.to(DEV), 0, n, 0, ncols, reverse=True)
        assert torch.equal(B.storage, before)
    # a sub-range of pivots and columns, against the CPU twin
    B, Bc = cc.to_matrix(b, nb, DEV), cc.to_matrix(b, nb, "cpu")
    ops.laswp(B.storage, piv.to(DEV), 40, 120, 37, 130)
    ops.laswp(Bc.storage, piv, 40, 120, 37, 130)
    assert torch.equal(B.storage.cpu(), Bc.storage)
    perm = ops.pivots_to_permutation(piv.to(DEV))
    assert torch.equal(perm.cpu(), ops.pivots_to_permutation(piv))


def test_panel_leaves_other_tile_columns_alone():
    """One panel call writes tile column k (rows from k*nb) and ipiv only."""
    n, nb, k = 100, 32, 1
    a = lc.make("scrambled", n, "float64")
    A = cc.to_matrix(a, nb, DEV)
    before = A.storage.clone()
    ipiv = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    get_ext().lu_panel(A.storage, n, k, ipiv, info)
    after = A.storage
    keep = torch.ones(4, 4, dtype=torch.bool)
    keep[k:, k] = False
    assert torch.equal(after[keep], before[keep])
    assert bool((ipiv[:32] == -7).all()) and bool((ipiv[64:] == -7).all())
    p = ipiv[32:64].cpu().numpy()
    assert (p >= np.arange(32, 64)).all() and (p < n).all()
    assert int(info) == 0


def test_empty_launches_nothing():
    st = torch.zeros((0, 0, 16, 16), dtype=torch.float64, device=DEV)
    ipiv = torch.zeros(0, dtype=torch.int32, device=DEV)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    get_ext().lu_panel(st, 0, 0, ipiv, info)
    get_ext().laswp_tiles(st, ipiv, 0, 0, 0, 0, False)
    torch.cuda.synchronize()
    assert int(info) == 0
