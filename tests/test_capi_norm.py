"""The ScaLAPACK-style norm shims (p?lange / p?lansy / p?lanhe / p?lantr and
dlaf_matrix_norm) against matrix_norm on the same matrix."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

from dlaf_amd import UpLo, Diag, matrix_norm, capi  # noqa: E402
from dlaf_amd.capi import DLAF_descriptor  # noqa: E402

CHARS = {"M": "max", "1": "one", "O": "one", "I": "inf", "F": "fro",
         "E": "fro"}


@pytest.fixture()
def ctx():
    c = capi.dlaf_create_grid(1, 1)
    yield c
    capi.dlaf_free_grid(c)


def _device():
    import torch
    return "cuda" if torch.cuda.is_available() else "cpu"


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_lange(ctx, dtype):
    m, n, nb = 37, 29, 8
    a = np.array(nc.make_general(m, n, dtype))
    mat = nc.to_matrix(a, nb, nb, _device())
    desc = DLAF_descriptor(m, n, nb, nb)
    for ch, name in CHARS.items():
        want = matrix_norm(name, mat)
        assert capi.pXlange(ctx, ch, m, n, a, 1, 1, desc) == want
        assert capi.pXlange(ctx, ch.lower(), m, n, a, 1, 1, desc) == want
    assert capi.dlaf_pdlange is capi.pXlange
    # leading part of a larger buffer
    sub = nc.to_matrix(a[:20, :13], nb, nb, _device())
    assert (capi.pXlange(ctx, "1", 20, 13, a, 1, 1, desc)
            == matrix_norm("one", sub))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_lanhe_lantr(ctx, dtype, uplo):
    n, nb = 37, 8
    ul = UpLo.Lower if uplo == "L" else UpLo.Upper
    a = nc.stored_with_garbage(nc.make_general(n, n, dtype), "hermitian", ul,
                               Diag.NonUnit)
    mat = nc.to_matrix(a, nb, nb, _device())
    desc = DLAF_descriptor(n, n, nb, nb)
    for ch, name in CHARS.items():
        want = matrix_norm(name, mat, uplo=ul, structure="hermitian")
        assert capi.pXlanhe(ctx, ch, uplo, n, a, 1, 1, desc) == want
        assert capi.pXlansy(ctx, ch, uplo, n, a, 1, 1, desc) == want
        for dg, d in (("N", Diag.NonUnit), ("U", Diag.Unit)):
            want = matrix_norm(name, mat, uplo=ul, structure="triangular",
                               diag=d)
            assert capi.pXlantr(ctx, ch, uplo, dg, n, n, a, 1, 1,
                                desc) == want
    assert (capi.dlaf_matrix_norm(ctx, "fro", "hermitian", uplo, "N", a, desc)
            == matrix_norm("fro", mat, uplo=ul, structure="hermitian"))


def test_input_is_not_modified(ctx):
    a = np.array(nc.make_general(21, 21, "float64"))
    keep = a.copy()
    capi.pXlansy(ctx, "F", "L", 21, a, 1, 1, DLAF_descriptor(21, 21, 8, 8))
    assert np.array_equal(a, keep)


def _dist_worker(rank, ws, gr, gc):
    m, n, nb = 37, 29, 8
    a = np.array(nc.make_general(m, n, "float64"))
    pr, pc = rank // gc, rank % gc
    rows = [i for i in range(m) if (i // nb) % gr == pr]
    cols = [j for j in range(n) if (j // nb) % gc == pc]
    loc = a[np.ix_(rows, cols)].copy()
    c = capi.dlaf_create_grid(gr, gc)
    out = [capi.pXlange(c, ch, m, n, loc, 1, 1, DLAF_descriptor(m, n, nb, nb))
           for ch in "M1IF"]
    capi.dlaf_free_grid(c)
    return out


def test_lange_distributed():
    outs = run_distributed(_dist_worker, 4, args=(2, 2))
    for o in outs[1:]:
        assert o == outs[0]
    a = np.array(nc.make_general(37, 29, "float64"))
    got = dict(zip(("max", "one", "inf", "fro"), outs[0]))
    nc.check_against_reference(got, a, "float64", "general", None,
                               Diag.NonUnit)
