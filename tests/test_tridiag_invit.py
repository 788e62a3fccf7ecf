"""Tridiagonal eigenvectors by inverse iteration, host twin (CPU tensors).

Bounds are the D&C ones of ``tests/test_tridiag.py`` (1e-12*n, about 4500
n*eps*G); a float64 prototype of the algorithm measured at most 3.3 n*eps*G
on this grid (graded n = 257), LAPACK dstebz+dstein below 1.
"""

import numpy as np
import pytest
import torch

import tridiag_cases as tc
import invit_checks as ic
from dlaf_amd.ops._ext import get_ext
from dlaf_amd import (
    tridiagonal_eigensolver_bisect, tridiagonal_eigenvalues,
    tridiagonal_eigenvectors,
)


@pytest.mark.parametrize("n", ic.SIZES)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_full_range(family, n):
    ic.check_eigenvectors(family, n)


@pytest.mark.parametrize("ib,ie", ic.RANGES_257)
@pytest.mark.parametrize("family", ["random", "glued_wilkinson"])
def test_index_ranges(family, ib, ie):
    ic.check_eigenvectors(family, 257, ib, ie)


@pytest.mark.parametrize("family", ic.CHUNK_CASES)
def test_across_lds_chunk(family):
    ic.check_eigenvectors(family, 1025, 400, 520)


@pytest.mark.parametrize("family", ["random", "graded", "constant_diag"])
def test_several_column_chunks(family):
    """_work_cols=64 at n = 257: five kernel chunks, the last one partial."""
    Z = ic.check_eigenvectors(family, 257, _work_cols=64)
    # chunking is not visible in the result
    assert torch.equal(Z, ic.check_eigenvectors(family, 257))


def test_deterministic():
    d, e = tc.make_case("random", 257)
    d, e = torch.from_numpy(d), torch.from_numpy(e)
    w1, Z1 = tridiagonal_eigensolver_bisect(d, e, 17, 93)
    w2, Z2 = tridiagonal_eigensolver_bisect(d, e, 17, 93)
    assert torch.equal(w1, w2) and torch.equal(Z1, Z2)
    assert torch.equal(w1, tridiagonal_eigenvalues(d, e, 17, 93))


def test_degenerate_shapes():
    d = torch.tensor([2.5], dtype=torch.float64)
    e = torch.zeros(0, dtype=torch.float64)
    assert tridiagonal_eigenvectors(d, e, d).tolist() == [[1.0]]
    assert tridiagonal_eigenvectors(d, e, e).shape == (1, 0)
    assert tridiagonal_eigenvectors(e, e, e).shape == (0, 0)
    w, Z = tridiagonal_eigensolver_bisect(e, e)
    assert w.shape == (0,) and Z.shape == (0, 0)
    # all-zero T: identity columns
    z5, z4 = torch.zeros(5, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    Z = tridiagonal_eigenvectors(z5, z4, torch.zeros(3, dtype=torch.float64))
    assert torch.equal(Z, torch.eye(5, 3, dtype=torch.float64))


def test_scaling_invariance():
    """The driver scales T by 1/max(|d|, |e|): a matrix far from unit norm
    meets the same (relative) bounds."""
    n = 65
    d, e = tc.make_case("random", n)
    for s in (1e-100, 1e100):
        ds, es = torch.from_numpy(d * s), torch.from_numpy(e * s)
        w, Z = tridiagonal_eigensolver_bisect(ds, es)
        Zn, wn = Z.numpy(), w.numpy() / s
        TZ = d[:, None] * Zn
        TZ[:-1] += e[:, None] * Zn[1:]
        TZ[1:] += e[:, None] * Zn[:-1]
        scale = max(1.0, np.abs(d).max(), np.abs(e).max())
        assert np.abs(TZ - Zn * wn).max() < 1e-12 * n * scale
        assert np.abs(Zn.T @ Zn - np.eye(n)).max() < 1e-12 * n


@pytest.mark.parametrize("at_eigenvalues", [False, True],
                         ids=["midpoints", "eigenvalues"])
@pytest.mark.parametrize("n", ic.SOLVE_SIZES)
@pytest.mark.parametrize("family", ic.SOLVE_FAMILIES)
def test_shifted_solve_backward_error(family, n, at_eigenvalues):
    ic.check_solve(family, n, at_eigenvalues)


def test_shifted_solve_column_slice():
    """X may be a column slice of a wider row-major matrix (how the driver
    feeds one chunk): same bits as the contiguous solve."""
    ds, es, lam, t1, X = ic.solve_case("random", 65, True)
    full = ic.run_solve(ds, es, lam, t1, X, "cpu")
    Y = X.clone()
    view = Y[:, 10:40]
    assert not view.is_contiguous()
    work = torch.empty((3, 65, 64), dtype=torch.float64)
    get_ext().tridiag_shifted_solve(
        torch.from_numpy(ds), torch.from_numpy(es),
        torch.from_numpy(lam[10:40].copy()), tc.EPS * t1, view, work)
    assert torch.equal(Y[:, 10:40], full[:, 10:40])
    assert torch.equal(Y[:, :10], X[:, :10]) and torch.equal(Y[:, 40:], X[:, 40:])
