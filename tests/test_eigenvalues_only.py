"""Eigenvalues-only drivers (hermitian_eigenvalues and the generalized
variant): local, tiny, value-range, distributed (gloo) and the C-style API.

Tolerances are the ones ``tests/test_eigensolver.py`` uses for ``w`` of the
same dtype: 1e-11*n*scale (f64/c128), 1e-2 (single precision), 1e-9*n*scale
(generalized), 1e-10*n (distributed).
"""

import numpy as np
import pytest
import torch

from dlaf_amd import (
    CommGrid, Matrix, UpLo, hermitian_eigenvalues,
    hermitian_generalized_eigenvalues,
)
from dlaf_amd.core.asserts import DlafAssertError
from dlaf_amd.matrix import util as mutil
from dist_utils import run_distributed


def _herm(a):
    return torch.tril(a) + torch.tril(a, -1).mH


def _make(n, nb, dtype, seed, grid=None):
    mat = Matrix.create(n, n, nb, nb, dtype=dtype, grid=grid)
    mutil.set_random_hermitian(mat, seed=seed)
    return mat, _herm(mat.to_global())


def _wide(dtype):
    return torch.complex128 if dtype.is_complex else torch.float64


def _real(dtype):
    return {torch.float64: torch.float64, torch.float32: torch.float32,
            torch.complex128: torch.float64, torch.complex64: torch.float32}[dtype]


def _tol(dtype, n, wref):
    if dtype in (torch.float32, torch.complex64):
        return 1e-2
    return 1e-11 * n * max(1.0, float(np.abs(wref).max()))


CASES = [(torch.float64, 96, 16), (torch.float32, 96, 16),
         (torch.complex128, 96, 16), (torch.complex64, 96, 16),
         (torch.float64, 100, 32)]


@pytest.mark.parametrize("dtype,n,nb", CASES)
def test_hermitian_eigenvalues(dtype, n, nb):
    mat, a0 = _make(n, nb, dtype, seed=51)
    wref = np.linalg.eigvalsh(a0.to(_wide(dtype)).numpy())
    w = hermitian_eigenvalues(UpLo.Lower, mat)
    assert w.dtype == _real(dtype) and w.shape == (n,)
    wn = w.numpy().astype(np.float64)
    assert np.all(np.diff(wn) >= 0)
    assert np.abs(wn - wref).max() < _tol(dtype, n, wref)


@pytest.mark.parametrize("dtype,n,nb", CASES)
def test_index_and_value_range(dtype, n, nb):
    mat, a0 = _make(n, nb, dtype, seed=52)
    wref = np.linalg.eigvalsh(a0.to(_wide(dtype)).numpy())
    w_idx = hermitian_eigenvalues(UpLo.Lower, mat, eigenvalues_index_begin=10,
                                  eigenvalues_index_end=40)
    assert w_idx.shape == (30,)
    assert np.abs(w_idx.numpy().astype(np.float64) - wref[10:40]).max() \
        < _tol(dtype, n, wref)
    # half-open [vl, vu) midway between reference eigenvalues 9/10 and 39/40
    vl = 0.5 * (wref[9] + wref[10])
    vu = 0.5 * (wref[39] + wref[40])
    mat2, _ = _make(n, nb, dtype, seed=52)
    w_val = hermitian_eigenvalues(UpLo.Lower, mat2,
                                  eigenvalues_value_range=(vl, vu))
    assert w_val.shape == (30,)
    assert torch.equal(w_val, w_idx)


def test_value_range_excludes_index_range():
    mat, _ = _make(32, 8, torch.float64, seed=53)
    with pytest.raises(DlafAssertError):
        hermitian_eigenvalues(UpLo.Lower, mat, eigenvalues_index_begin=2,
                              eigenvalues_value_range=(0.0, 1.0))


def test_overwrites_like_the_eigensolver():
    """mat is left with the same band + reflectors as hermitian_eigensolver."""
    from dlaf_amd import hermitian_eigensolver
    m1, _ = _make(96, 16, torch.float64, seed=54)
    m2, _ = _make(96, 16, torch.float64, seed=54)
    hermitian_eigenvalues(UpLo.Lower, m1)
    hermitian_eigensolver(UpLo.Lower, m2)
    assert torch.equal(m1.to_global(), m2.to_global())


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
def test_tiny_path(dtype):
    n, nb = 8, 16
    mat, a0 = _make(n, nb, dtype, seed=55)
    wref = np.linalg.eigvalsh(a0.numpy())
    w = hermitian_eigenvalues(UpLo.Lower, mat)
    assert w.dtype == torch.float64
    assert np.abs(w.numpy() - wref).max() < _tol(dtype, n, wref)
    mat2, _ = _make(n, nb, dtype, seed=55)
    vl, vu = 0.5 * (wref[1] + wref[2]), 0.5 * (wref[5] + wref[6])
    w2 = hermitian_eigenvalues(UpLo.Lower, mat2,
                               eigenvalues_value_range=(vl, vu))
    assert torch.equal(w2, w[2:6])


def _gen_reference(a0, b0):
    """eigvalsh(L^-1 A L^-H) with numpy only."""
    L = np.linalg.cholesky(b0)
    Li = np.linalg.inv(L)
    c = Li @ a0 @ Li.conj().T
    return np.linalg.eigvalsh(0.5 * (c + c.conj().T))


@pytest.mark.parametrize("factorized", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
def test_generalized(dtype, factorized):
    n, nb = 96, 16
    A = Matrix.create(n, n, nb, nb, dtype=dtype)
    B = Matrix.create(n, n, nb, nb, dtype=dtype)
    mutil.set_random_hermitian(A, seed=61)
    mutil.set_random_hermitian_positive_definite(B, seed=62)
    a0, b0 = _herm(A.to_global()).numpy(), _herm(B.to_global()).numpy()
    wref = _gen_reference(a0, b0)
    if factorized:
        from dlaf_amd import cholesky_factorization
        cholesky_factorization(UpLo.Lower, B)
    w = hermitian_generalized_eigenvalues(UpLo.Lower, A, B,
                                          factorized=factorized)
    scale = max(1.0, float(np.abs(wref).max()))
    assert np.abs(w.numpy() - wref).max() < 1e-9 * n * scale


# ---------------- distributed (gloo) ----------------

def _dist_worker(rank, ws, gr, gc, n, nb, dtype_str, ib, ie):
    import torch.distributed as dist
    dtype = getattr(torch, dtype_str)
    grid = CommGrid(gr, gc)
    A, a0 = _make(n, nb, dtype, seed=71, grid=grid)
    w = hermitian_eigenvalues(UpLo.Lower, A, grid, eigenvalues_index_begin=ib,
                              eigenvalues_index_end=ie)
    gath = [torch.empty_like(w) for _ in range(ws)]
    dist.all_gather(gath, w.contiguous())
    same = all(torch.equal(g, gath[0]) for g in gath)
    wref = np.linalg.eigvalsh(a0.numpy())[ib:ie]
    return same, tuple(w.shape), float(np.abs(w.numpy() - wref).max())


@pytest.mark.parametrize("ib,ie", [(0, 96), (10, 40)])
@pytest.mark.parametrize("dtype_str", ["float64", "complex128"])
def test_distributed_2x2(dtype_str, ib, ie):
    n = 96
    out = run_distributed(_dist_worker, 4,
                          args=(2, 2, n, 16, dtype_str, ib, ie))
    for same, shape, werr in out:
        assert same, "ranks returned different bits"
        assert shape == (ie - ib,)
        assert werr < 1e-10 * n, f"werr={werr}"


# ---------------- C-style API ----------------

@pytest.mark.parametrize("uplo", ["L", "U"])
def test_capi_eigenvalues(uplo):
    from dlaf_amd import capi
    n, nb = 48, 16
    rng = np.random.default_rng(5)
    a0 = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    a0 = (a0 + a0.conj().T) / 2
    wref = np.linalg.eigvalsh(a0)
    # hand over only the named triangle
    loc = np.asfortranarray(np.tril(a0) if uplo == "L" else np.triu(a0))
    ctx = capi.dlaf_create_grid(1, 1)
    desc = capi.DLAF_descriptor(n, n, nb, nb, ld=n)
    w = np.zeros(n)
    assert capi.dlaf_hermitian_eigenvalues(ctx, uplo, loc, desc, w) == 0
    assert np.abs(w - wref).max() < 1e-11 * n * max(1.0, np.abs(wref).max())
    loc = np.asfortranarray(np.tril(a0) if uplo == "L" else np.triu(a0))
    w2 = np.zeros(n)
    assert capi.dlaf_hermitian_eigenvalues(ctx, uplo, loc, desc, w2,
                                           il=5, iu=20) == 0
    assert np.array_equal(w2[:15], w[5:20])
    capi.dlaf_free_grid(ctx)


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_capi_generalized_eigenvalues(uplo):
    from dlaf_amd import capi
    n, nb = 48, 16
    rng = np.random.default_rng(6)
    a0 = rng.standard_normal((n, n))
    a0 = (a0 + a0.T) / 2
    b0 = rng.standard_normal((n, n))
    b0 = b0 @ b0.T + n * np.eye(n)
    wref = _gen_reference(a0, b0)
    tri = np.tril if uplo == "L" else np.triu
    a, b = np.asfortranarray(tri(a0)), np.asfortranarray(tri(b0))
    ctx = capi.dlaf_create_grid(1, 1)
    desc = capi.DLAF_descriptor(n, n, nb, nb, ld=n)
    w = np.zeros(n)
    assert capi.dlaf_hermitian_generalized_eigenvalues(
        ctx, uplo, a, desc, b, desc, w) == 0
    capi.dlaf_free_grid(ctx)
    assert np.abs(w - wref).max() < 1e-9 * n * max(1.0, np.abs(wref).max())
