"""The ScaLAPACK-style shims p?getrf / p?getrs / p?gecon / p?gesv (and the
dlaf_* functions under them) on a 1x1 grid, against the library calls on the
same matrix and the references of lu_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
import lu_cases as lc  # noqa: E402

from dlaf_amd import capi, lu_rcond  # noqa: E402
from dlaf_amd.capi import DLAF_descriptor  # noqa: E402
from dlaf_amd.core.asserts import DlafAssertError  # noqa: E402
from dist_utils import run_distributed  # noqa: E402


@pytest.fixture()
def ctx():
    c = capi.dlaf_create_grid(1, 1)
    yield c
    capi.dlaf_free_grid(c)


def _device():
    return "cuda" if torch.cuda.is_available() else "cpu"


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_getrf_getrs_gecon(ctx, dtype):
    n, nb, nrhs = 70, 17, 3
    a0 = lc.make("scrambled", n, dtype)
    a = np.array(a0)
    desca = DLAF_descriptor(n, n, nb, nb)
    descb = DLAF_descriptor(n, nrhs, nb, nb)
    norms = {ch: capi.pXlange(ctx, ch, n, n, a, 1, 1, desca)
             for ch in ("1", "I")}
    ipiv = np.zeros(n, dtype=np.int32)
    assert capi.pXgetrf(ctx, n, n, a, 1, 1, desca, ipiv) == 0
    # 1-based global row indices, the reference's own
    piv_ref, _, _ = lc.reference(("kind", "scrambled", n, dtype))
    assert np.array_equal(ipiv, piv_ref + 1)
    A, piv0, _ = lc.factor(a0, nb, _device())
    assert np.array_equal(a, A.to_global().cpu().numpy())
    keep, keep_piv = a.copy(), ipiv.copy()
    w = cc.wide(dtype)
    b0 = lc.rhs(n, nrhs, dtype)
    for ch, op in (("N", cc.OPS[0]), ("T", cc.OPS[1]), ("C", cc.OPS[2]),
                   ("n", cc.OPS[0])):
        b = np.array(b0)
        assert capi.pXgetrs(ctx, ch, n, nrhs, a, 1, 1, desca, ipiv, b, 1, 1,
                            descb) == 0
        want = np.linalg.solve(cc.apply_op(a0.astype(w), op), b0.astype(w))
        assert np.abs(b - want).max() < cc.solve_tol(dtype, n + nrhs)
    for ch, name in (("1", "one"), ("O", "one"), ("I", "inf")):
        got = capi.pXgecon(ctx, ch, n, a, 1, 1, desca, norms[ch if ch != "O"
                                                             else "1"])
        assert got == lu_rcond(name, A, norms[ch if ch != "O" else "1"])
        t = a0 if name == "one" else a0.T
        cc.check_band(got, cc.norm1(t.astype(w)), cc.inv_norm1(t), n, dtype)
    assert np.array_equal(a, keep) and np.array_equal(ipiv, keep_piv)
    assert capi.dlaf_lu_rcond(ctx, "1", a, desca, 0.0) == 0.0


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_gesv(ctx, dtype):
    n, nb, nrhs = 40, 16, 2
    a0 = lc.make("scrambled", n, dtype)
    b0 = lc.rhs(n, nrhs, dtype)
    a, b = np.array(a0), np.array(b0)
    desca = DLAF_descriptor(n, n, nb, nb)
    descb = DLAF_descriptor(n, nrhs, nb, nb)
    ipiv = np.zeros(n, dtype=np.int32)
    assert capi.pXgesv(ctx, n, nrhs, a, 1, 1, desca, ipiv, b, 1, 1,
                       descb) == 0
    w = cc.wide(dtype)
    want = np.linalg.solve(a0.astype(w), b0.astype(w))
    assert np.abs(b - want).max() < cc.solve_tol(dtype, n + nrhs)
    # the same as getrf + getrs, bitwise
    a2, b2 = np.array(a0), np.array(b0)
    ipiv2 = np.zeros(n, dtype=np.int32)
    capi.pXgetrf(ctx, n, n, a2, 1, 1, desca, ipiv2)
    capi.pXgetrs(ctx, "N", n, nrhs, a2, 1, 1, desca, ipiv2, b2, 1, 1, descb)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    assert np.array_equal(ipiv, ipiv2)
    # singular: info of the first zero pivot, B untouched
    c = 13
    s = np.array(lc.singular(n, dtype, (c,)))
    b = np.array(b0)
    assert capi.pXgesv(ctx, n, nrhs, s, 1, 1, desca, ipiv, b, 1, 1,
                       descb) == c + 1
    assert np.array_equal(b, b0)
    assert ipiv[c] == c + 1 and s[c, c] == 0


def test_aliases_and_leading_part(ctx):
    for p in "sdcz":
        assert getattr(capi, f"dlaf_p{p}getrf") is capi.pXgetrf
        assert getattr(capi, f"dlaf_p{p}getrs") is capi.pXgetrs
        assert getattr(capi, f"dlaf_p{p}gecon") is capi.pXgecon
        assert getattr(capi, f"dlaf_p{p}gesv") is capi.pXgesv
    # the leading 40 x 40 of a larger buffer; the rest is left alone
    n, nb = 40, 16
    big = np.full((70, 70), 1e30)
    a0 = lc.make("scrambled", n, "float64")
    big[:n, :n] = a0
    desc = DLAF_descriptor(70, 70, nb, nb)
    ipiv = np.zeros(n, dtype=np.int32)
    assert capi.pXgetrf(ctx, n, n, big, 1, 1, desc, ipiv) == 0
    A, piv0, _ = lc.factor(a0, nb, _device())
    assert np.array_equal(big[:n, :n], A.to_global().cpu().numpy())
    assert np.array_equal(ipiv, piv0.cpu().numpy() + 1)
    assert (big[n:, :] == 1e30).all() and (big[:, n:] == 1e30).all()
    with pytest.raises(AssertionError):
        capi.pXgetrf(ctx, 40, 30, big, 1, 1, desc, ipiv)


def _dist_worker(rank, ws):
    c = capi.dlaf_create_grid(1, 2)
    desc = DLAF_descriptor(32, 32, 8, 8)
    descb = DLAF_descriptor(32, 2, 8, 8)
    lm, ln = capi.dlaf_local_shape(c, desc)
    a = np.eye(lm, ln)
    b = np.zeros(capi.dlaf_local_shape(c, descb))
    ipiv = np.ones(32, dtype=np.int32)
    msgs = []
    for call in (
            lambda: capi.pXgetrf(c, 32, 32, a, 1, 1, desc, ipiv),
            lambda: capi.pXgetrs(c, "N", 32, 2, a, 1, 1, desc, ipiv, b, 1, 1,
                                 descb),
            lambda: capi.pXgecon(c, "1", 32, a, 1, 1, desc, 1.0),
            lambda: capi.pXgesv(c, 32, 2, a, 1, 1, desc, ipiv, b, 1, 1,
                                descb)):
        try:
            call()
        except DlafAssertError as err:
            msgs.append(str(err))
        else:
            msgs.append(None)
    capi.dlaf_free_grid(c)
    return msgs


def test_multi_rank_context_rejected():
    for msgs in run_distributed(_dist_worker, 2):
        for m in msgs:
            assert m is not None and "multi-rank" in m
