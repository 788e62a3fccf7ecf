"""The shims p?porfs / pdsposv / pzcposv (and the dlaf_* functions under
them) on a 1x1 grid, against the library calls on the same matrices and the
bounds of refine_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
import refine_cases as rc  # noqa: E402

from dlaf_amd import UpLo, capi  # noqa: E402
from dlaf_amd.capi import DLAF_descriptor  # noqa: E402


@pytest.fixture()
def ctx():
    c = capi.dlaf_create_grid(1, 1)
    yield c
    capi.dlaf_free_grid(c)


def _device():
    return "cuda" if torch.cuda.is_available() else "cpu"


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_porfs(ctx, dtype, uplo):
    n, nb, nrhs = 37, 8, rc.NRHS
    ul = UpLo(uplo)
    a = np.array(cc.make_spd("wishart", n, dtype))
    b = np.array(rc.rhs_block(n, dtype))
    desca = DLAF_descriptor(n, n, nb, nb)
    descb = DLAF_descriptor(n, nrhs, nb, nb)
    af = a.copy()
    assert capi.pXpotrf(ctx, uplo, n, af, 1, 1, desca) == 0
    x = b.copy()
    assert capi.pXpotrs(ctx, uplo, n, nrhs, af, 1, 1, desca, x, 1, 1,
                        descb) == 0
    x0 = x.copy()
    keep = [a.copy(), af.copy(), b.copy()]
    ferr, berr = np.zeros(nrhs), np.zeros(nrhs)
    assert capi.pXporfs(ctx, uplo, n, nrhs, a, 1, 1, desca, af, 1, 1, desca,
                        b, 1, 1, descb, x, 1, 1, descb, ferr, berr) == 0
    for got, want in zip((a, af, b), keep):
        assert np.array_equal(got, want)  # only read
    # the direct call on the same numbers
    from dlaf_amd import cholesky_refine
    dev = _device()
    X = cc.to_matrix(x0, nb, dev)
    f2, b2 = cholesky_refine(ul, cc.to_matrix(a, nb, dev),
                             cc.to_matrix(af, nb, dev),
                             cc.to_matrix(b, nb, dev), X)
    assert np.array_equal(ferr, f2.numpy())
    assert np.array_equal(berr, b2.numpy())
    assert np.array_equal(x, X.to_global().cpu().numpy())
    rc.check_bounds(x, f2, b2, "wishart", n, dtype)
    # through the dlaf_* function, and the aliases
    x3, f3, b3 = x0.copy(), np.zeros(nrhs), np.zeros(nrhs)
    assert capi.dlaf_cholesky_refine(ctx, uplo, a, desca, af, desca, b, descb,
                                     x3, descb, f3, b3) == 0
    assert np.array_equal(x3, x) and np.array_equal(f3, ferr)
    assert (capi.dlaf_pdporfs is capi.pXporfs
            and capi.dlaf_psporfs is capi.pXporfs
            and capi.dlaf_pcporfs is capi.pXporfs
            and capi.dlaf_pzporfs is capi.pXporfs)


@pytest.mark.parametrize("dtype", rc.MIXED_DTYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_sposv(ctx, dtype, uplo):
    n, nb, nrhs = 37, 8, rc.NRHS
    a = np.array(cc.make_spd("wishart", n, dtype))
    b = np.array(rc.rhs_block(n, dtype))
    desca = DLAF_descriptor(n, n, nb, nb)
    descb = DLAF_descriptor(n, nrhs, nb, nb)
    keep = a.copy(), b.copy()
    x = np.zeros_like(b)
    iters, info = capi.pXsposv(ctx, uplo, n, nrhs, a, 1, 1, desca, b, 1, 1,
                               descb, x, 1, 1, descb)
    assert np.array_equal(a, keep[0]) and np.array_equal(b, keep[1])
    want, it2, info2 = rc.run_mixed(a, b, nb, UpLo(uplo), _device())
    assert (iters, info) == (it2, info2) and 0 <= iters <= 8 and info == 0
    assert np.array_equal(x, want)
    assert rc.mixed_criterion(a, b, x)
    x3 = np.zeros_like(b)
    assert capi.dlaf_cholesky_solve_mixed(ctx, uplo, a, desca, b, descb, x3,
                                          descb) == (iters, info)
    assert np.array_equal(x3, x)
    assert capi.dlaf_pdsposv is capi.pXsposv
    assert capi.dlaf_pzcposv is capi.pXsposv
    # leading part of larger buffers
    m = 20
    xs = np.zeros_like(b)
    it4, info4 = capi.pXsposv(ctx, uplo, m, 2, a, 1, 1, desca, b, 1, 1, descb,
                              xs, 1, 1, descb)
    assert info4 == 0 and 0 <= it4 <= 8
    assert rc.mixed_criterion(a[:m, :m], b[:m, :2], xs[:m, :2])
    assert not xs[m:].any() and not xs[:, 2:].any()


def test_potrf_info_is_cholesky_info(ctx):
    """capi._potrf_info is the algs-level scan: the failed pivot, 1-based."""
    from dlaf_amd import cholesky_info, cholesky_factorization
    n, nb = 37, 8
    a = np.array(cc.make_spd("wishart", n, "float64"))
    a[20, 20] = -1.0
    mat = cc.to_matrix(a, nb, _device())
    cholesky_factorization(UpLo.Lower, mat)
    assert cholesky_info(mat) == capi._potrf_info(mat) == 21
    desc = DLAF_descriptor(n, n, nb, nb)
    assert capi.pXpotrf(ctx, "L", n, a, 1, 1, desc) == 21
