"""The Hermitian vector-product kernel (csrc/hemv.hip) and, on top of it,
cholesky_refine, cholesky_solve_expert and cholesky_solve_mixed on the device.
The (n, nb) of cond_cases.SOLVE_SHAPES are the smallest that reach one tile, a
partial last tile, misaligned tile bases (nb=17 in float32 / complex64: the
scalar path), two and three tile rows, and a tile of several strips and column
blocks with a ragged last one (nb=160). Bounds and matrices: refine_cases.py."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cond_cases as cc  # noqa: E402
import refine_cases as rc  # noqa: E402

from dlaf_amd import (  # noqa: E402
    UpLo, HermitianVectorProduct, TriangularVectorSolver, Diag,
)
from dlaf_amd.ops._ext import get_ext  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ids = dict(ids=lambda s: f"{s[0]}-{s[1]}")
_uids = dict(ids=lambda u: u.value)


def _product(n, nb, dtype, uplo, kind="wishart"):
    a = rc.stored_hermitian(cc.make_spd(kind, n, dtype), uplo)
    hv = HermitianVectorProduct(uplo, cc.to_matrix(a, nb, DEV),
                                method="kernel")
    assert hv.method == "kernel"
    return hv


def _raw(hv, storage, x, want_abs=True, fill=0.0, xtail=0.0):
    """The kernel on padded vectors, y and yabs prefilled with ``fill``, the
    tail of x with ``xtail``; returns the whole padded (y, yabs)."""
    d = hv.A.dist
    pad = d.nr_tiles[0] * d.nb
    rdt = hv._apad.dtype
    xp = torch.full((pad,), xtail, dtype=hv.A.dtype, device=DEV)
    xp[: hv.n] = torch.from_numpy(np.array(x)).to(DEV)
    y = torch.full((pad,), fill, dtype=hv.A.dtype, device=DEV)
    yabs = (torch.full((pad,), fill, dtype=rdt, device=DEV) if want_abs
            else torch.empty(0, dtype=rdt, device=DEV))
    get_ext().hemv_tiles(storage, xp, y, yabs, hv.n,
                         int(hv.uplo == UpLo.Upper))
    return y, yabs


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, **_ids)
def test_kernel_product(shape, dtype):
    n, nb = shape
    x = torch.from_numpy(np.array(rc.vector(n, dtype))).to(DEV)
    for uplo in cc.UPLOS:
        hv = _product(n, nb, dtype, uplo)
        y, yabs = hv.apply(x, want_abs=True)
        assert y.dtype == x.dtype and y.shape == x.shape
        assert not yabs.is_complex() and yabs.shape == x.shape
        rc.check_product(y.cpu().numpy(), yabs.cpu().numpy(), "wishart", n,
                         dtype)


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("shape", cc.SOLVE_SHAPES, **_ids)
def test_kernel_repeatable_and_padding(shape, dtype):
    """Two calls give the same bits; NaN all over the padding of the tiles
    and in the tail of x changes nothing; the tails of y and yabs stay as
    they were; leaving yabs out gives the same y."""
    n, nb = shape
    x = rc.vector(n, dtype)
    for uplo in cc.UPLOS:
        hv = _product(n, nb, dtype, uplo)
        nt = hv.A.dist.nr_tiles[0]
        pad = nt * nb - n
        dirty = hv._storage.clone()
        if pad:
            dirty[nt - 1, :, nb - pad:, :] = float("nan")
            dirty[:, nt - 1, :, nb - pad:] = float("nan")
        y1, a1 = _raw(hv, hv._storage, x, fill=7.0)
        y2, a2 = _raw(hv, hv._storage, x, fill=7.0)
        y3, a3 = _raw(hv, dirty, x, fill=7.0, xtail=float("nan"))
        y4, _ = _raw(hv, hv._storage, x, want_abs=False, fill=7.0)
        assert torch.equal(y1, y2) and torch.equal(a1, a2), uplo
        assert torch.equal(y1, y3) and torch.equal(a1, a3), uplo
        assert torch.equal(y1, y4), uplo
        assert bool((y1[n:] == 7.0).all()) and bool((a1[n:] == 7.0).all())
        xin = torch.from_numpy(np.array(x)).to(DEV)
        via, via_abs = hv.apply(xin, want_abs=True)
        assert torch.equal(via, y1[:n]) and torch.equal(via_abs, a1[:n])
        assert torch.equal(hv.apply(xin), y1[:n])


@pytest.mark.parametrize("dtype", ["float32", "float64", "complex64"])
def test_unaligned_storage_takes_scalar_path(dtype):
    """A storage starting 4 or 8 bytes into the allocation cannot use 16-byte
    loads; the result is the one of the aligned storage."""
    n, nb = 100, 32
    x = rc.vector(n, dtype)
    for uplo in cc.UPLOS:
        hv = _product(n, nb, dtype, uplo)
        src = hv._storage
        flat = torch.zeros(src.numel() + 1, dtype=src.dtype, device=DEV)
        flat[1:] = src.reshape(-1)
        shifted = flat[1:].view(src.shape)
        assert shifted.data_ptr() % 16 != 0
        want, want_abs = _raw(hv, src, x)
        got, got_abs = _raw(hv, shifted, x)
        assert torch.equal(got, want) and torch.equal(got_abs, want_abs)


def test_empty_storage_launches_nothing():
    st = torch.zeros((0, 0, 16, 16), dtype=torch.float64, device=DEV)
    v = torch.zeros(0, dtype=torch.float64, device=DEV)
    get_ext().hemv_tiles(st, v, v.clone(), v.clone(), 0, 0)
    torch.cuda.synchronize()
    assert get_ext().hemv_work_size(0, 16) == 0


def test_auto_picks_the_kernel_on_the_device():
    A = cc.to_matrix(cc.make_spd("wishart", 40, "float64"), 16, DEV)
    assert HermitianVectorProduct(UpLo.Lower, A).method == "kernel"
    assert TriangularVectorSolver(UpLo.Lower, Diag.NonUnit, A).method == "kernel"


@pytest.mark.parametrize("dtype", cc.DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, **_uids)
@pytest.mark.parametrize("kind", cc.SPD_KINDS)
@pytest.mark.parametrize("shape", rc.REFINE_SHAPES, **_ids)
def test_refine_kernel(shape, kind, uplo, dtype):
    n, nb = shape
    x, ferr, berr = rc.run_refine(kind, n, nb, dtype, uplo, DEV, "kernel")
    rc.check_bounds(x, ferr, berr, kind, n, dtype)  # (a), (b)
    rc.check_band(ferr.numpy(), rc.blocked_ferr(kind, n, nb, dtype, uplo))
    x, ferr, berr = rc.run_refine(kind, n, nb, dtype, uplo, DEV, "kernel",
                                  perturb=True)
    rc.check_bounds(x, ferr, berr, kind, n, dtype)  # (d)


@pytest.mark.parametrize("dtype", rc.MIXED_DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, **_uids)
@pytest.mark.parametrize("kind", cc.SPD_KINDS)
@pytest.mark.parametrize("shape", rc.REFINE_SHAPES, **_ids)
def test_mixed_converges(shape, kind, uplo, dtype):
    rc.check_mixed_spd(kind, shape[0], shape[1], dtype, uplo, DEV)


@pytest.mark.parametrize("dtype", rc.MIXED_DTYPES)
@pytest.mark.parametrize("uplo", cc.UPLOS, **_uids)
def test_mixed_falls_back(uplo, dtype):
    rc.check_mixed_fallback(dtype, uplo, DEV)
    rc.check_mixed_overflow(dtype, uplo, DEV)


def test_mixed_uses_the_kernel_up_to_its_nrhs_limit(monkeypatch):
    """Both residual routes converge to the criterion: the vector kernel
    (nrhs = 3 <= MIXED_KERNEL_MAX_NRHS) and hermitian_multiplication."""
    from dlaf_amd.algs import refine
    calls = []
    real = refine.HermitianVectorProduct.apply

    def counting(self, *a, **k):
        calls.append(self.method)
        return real(self, *a, **k)

    monkeypatch.setattr(refine.HermitianVectorProduct, "apply", counting)
    rc.check_mixed_spd("graded", 100, 32, "float64", UpLo.Lower, DEV)
    assert calls and set(calls) == {"kernel"}
    del calls[:]
    monkeypatch.setattr(refine, "MIXED_KERNEL_MAX_NRHS", 2)
    rc.check_mixed_spd("graded", 100, 32, "float64", UpLo.Lower, DEV)
    assert not calls


def test_expert_is_its_parts():
    rc.check_expert(DEV, "kernel")
