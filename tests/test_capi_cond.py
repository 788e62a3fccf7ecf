"""The ScaLAPACK-style shims p?pocon / p?trcon / p?potrs (and the dlaf_*
functions under them) on a 1x1 grid, against the library calls on the same
matrix and the truths of cond_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402

from dlaf_amd import UpLo, Diag, triangular_rcond, capi  # noqa: E402
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
def test_pocon(ctx, dtype, uplo):
    n, nb = 37, 8
    ul = UpLo(uplo)
    a = np.array(cc.make_spd("wishart", n, dtype))
    desc = DLAF_descriptor(n, n, nb, nb)
    anorm = capi.pXlanhe(ctx, "1", uplo, n, a, 1, 1, desc)
    assert capi.pXpotrf(ctx, uplo, n, a, 1, 1, desc) == 0
    keep = a.copy()
    got = capi.pXpocon(ctx, uplo, n, a, 1, 1, desc, anorm)
    assert np.array_equal(a, keep)  # the factor is only read
    want, _, _ = cc.cholesky_rcond_of(cc.make_spd("wishart", n, dtype), nb,
                                      ul, _device())
    assert got == want
    an, ai = cc.spd_truth("wishart", n, dtype)
    cc.check_band(got, an, ai, n, dtype)
    assert capi.dlaf_cholesky_rcond(ctx, uplo, a, desc, anorm) == got
    assert capi.dlaf_pdpocon is capi.pXpocon
    assert capi.pXpocon(ctx, uplo, n, a, 1, 1, desc, 0.0) == 0.0


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_trcon(ctx, dtype, uplo):
    n, nb = 37, 8
    ul = UpLo(uplo)
    desc = DLAF_descriptor(n, n, nb, nb)
    for dg in (Diag.NonUnit, Diag.Unit):
        t = cc.make_triangular(n, dtype, ul, dg)
        a = cc.stored_with_garbage(t, ul, dg)
        mat = cc.to_matrix(a, nb, _device())
        for ch, name in (("1", "one"), ("O", "one"), ("I", "inf"),
                         ("i", "inf")):
            got = capi.pXtrcon(ctx, ch, uplo, dg.value, n, a, 1, 1, desc)
            assert got == triangular_rcond(name, ul, dg, mat)
            tt = t if name == "one" else t.T
            cc.check_band(got, cc.norm1(tt.astype(cc.wide(dtype))),
                          cc.inv_norm1(tt), n, dtype)
    assert capi.dlaf_pztrcon is capi.pXtrcon
    # leading part of a larger buffer
    sub = cc.to_matrix(a[:20, :20], nb, _device())
    assert (capi.pXtrcon(ctx, "1", uplo, "U", 20, a, 1, 1, desc)
            == triangular_rcond("one", ul, Diag.Unit, sub))


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_potrs(ctx, dtype, uplo):
    n, nb, nrhs = 37, 8, 3
    a0 = cc.make_spd("diagdom", n, dtype)
    a = np.array(a0)
    b0 = np.array(cc.make_spd("wishart", n, dtype))[:, :nrhs].copy()
    b = b0.copy()
    desca = DLAF_descriptor(n, n, nb, nb)
    descb = DLAF_descriptor(n, nrhs, nb, nb)
    assert capi.pXpotrf(ctx, uplo, n, a, 1, 1, desca) == 0
    keep = a.copy()
    assert capi.pXpotrs(ctx, uplo, n, nrhs, a, 1, 1, desca, b, 1, 1,
                        descb) == 0
    assert np.array_equal(a, keep)
    w = cc.wide(dtype)
    want = np.linalg.solve(a0.astype(w), b0.astype(w))
    assert np.abs(b - want).max() < cc.solve_tol(dtype, n + nrhs)
    assert capi.dlaf_pdpotrs is capi.pXpotrs
