"""matrix_norm on the CPU (the host twin of csrc/norms.hip): every norm,
structure and dtype against the longdouble reference of norm_cases.py,
masking of padding / other triangle / diagonal, NaN and inf propagation,
Frobenius at the ends of the exponent range, and distributed grids."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

from dlaf_amd import Matrix, UpLo, Diag, matrix_norm, max_norm  # noqa: E402

CASES = [(s, v) for s in nc.SHAPES for v in nc.variants_for(s[0], s[1])]


def _id(case):
    (m, n, mb, nb), (structure, uplo, diag) = case
    u = "" if uplo is None else uplo.value
    d = "unit" if diag == Diag.Unit else ""
    return f"{m}x{n}-{mb}x{nb}-{structure}{u}{d}"


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_norms_against_reference(case, dtype):
    (m, n, mb, nb), (structure, uplo, diag) = case
    nc.check_case(m, n, mb, nb, dtype, structure, uplo, diag, "cpu")


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_empty_matrix(dtype):
    mat = Matrix.create(0, 0, 4, 4, dtype=getattr(torch, dtype))
    for k in nc.NORMS:
        assert matrix_norm(k, mat) == 0.0
        assert matrix_norm(k, mat, uplo=UpLo.Lower,
                           structure="hermitian") == 0.0


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("uplo", [UpLo.Lower, UpLo.Upper])
def test_hermitian_ignores_other_triangle_and_diag_imag(dtype, uplo):
    """Bitwise the same with the unread storage clean or full of 1e30."""
    m, mb = 37, 8
    a = nc.make_general(m, m, dtype)
    clean = np.array(a)
    i, j = np.indices((m, m))
    if nc.is_complex(dtype):
        clean[i == j] = np.real(clean[i == j])
    dirty = nc.stored_with_garbage(a, "hermitian", uplo, Diag.NonUnit)
    g0 = nc.all_norms(nc.to_matrix(clean, mb, mb), "hermitian", uplo,
                      Diag.NonUnit)
    g1 = nc.all_norms(nc.to_matrix(dirty, mb, mb), "hermitian", uplo,
                      Diag.NonUnit)
    assert g0 == g1
    assert g0["one"] == g0["inf"]


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_max_equals_max_norm(dtype):
    a = nc.make_general(37, 29, dtype)
    mat = nc.to_matrix(a, 16, 16)
    sq = nc.to_matrix(nc.make_general(37, 37, dtype), 16, 16)
    pairs = [(matrix_norm("max", mat), max_norm(mat)),
             (matrix_norm("max", sq, uplo=UpLo.Lower, structure="triangular"),
              max_norm(sq, UpLo.Lower))]
    for got, old in pairs:
        if nc.is_complex(dtype):
            assert abs(got - old) <= 2 * nc.eps_of(dtype) * old
        else:
            assert got == old


def test_nan_and_inf_propagate():
    nc.check_nan_inf("cpu", "float64")
    nc.check_nan_inf("cpu", "complex64")


def test_frobenius_extremes():
    nc.check_fro_extremes("cpu")


def test_argument_checks():
    mat = nc.to_matrix(nc.make_general(5, 5, "float64"), 8, 8)
    with pytest.raises(Exception):
        matrix_norm("two", mat)
    with pytest.raises(Exception):
        matrix_norm("max", mat, structure="hermitian")  # uplo missing
    with pytest.raises(Exception):
        matrix_norm("max", mat, structure="banded")


# ---------------- distributed (gloo) ----------------

def _dist_worker(rank, ws, gr, gc, m, n, nb, dtype, structure):
    from dlaf_amd import CommGrid
    grid = CommGrid(gr, gc)
    uplo = UpLo.Lower if structure == "hermitian" else None
    a = nc.stored_with_garbage(nc.make_general(m, n, dtype), structure, uplo,
                               Diag.NonUnit)
    mat = nc.to_matrix(a, nb, nb, grid=grid)
    return nc.all_norms(mat, structure, uplo, Diag.NonUnit, grid)


@pytest.mark.parametrize("gr,gc", [(2, 2), (2, 3)])
@pytest.mark.parametrize("dtype", ["float64", "complex128"])
@pytest.mark.parametrize("m,n,structure", [(37, 29, "general"),
                                           (37, 37, "hermitian")])
def test_distributed(gr, gc, dtype, m, n, structure):
    outs = run_distributed(_dist_worker, gr * gc,
                           args=(gr, gc, m, n, 8, dtype, structure))
    for o in outs[1:]:
        assert o == outs[0]  # the same bits on every rank
    uplo = UpLo.Lower if structure == "hermitian" else None
    a = nc.stored_with_garbage(nc.make_general(m, n, dtype), structure, uplo,
                               Diag.NonUnit)
    nc.check_against_reference(outs[0], a, dtype, structure, uplo,
                               Diag.NonUnit)
