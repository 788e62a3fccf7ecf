"""Fused tile Cholesky (one launch per 64-column block): factor, every dinv
block, strided views, failed pivots, the invert-only entry, and bitwise
reproducibility next to a trailing-update-sized GEMM on another stream.

References are ``torch.linalg.cholesky`` in float64 / complex128 on the CPU;
tolerances are those of ``test_gpu_kernels.test_potrf_tile``.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dlaf_amd.ops import tile_ops as ops  # noqa: E402
from dlaf_amd.types import Op  # noqa: E402
from test_gpu_kernels import DTYPES, _rand, _tol  # noqa: E402


def _wide(dtype):
    return torch.complex128 if dtype.is_complex else torch.float64


def _spd(n, dtype, seed):
    torch.manual_seed(seed)
    a = _rand((n, n), dtype).cpu()
    return a @ a.mH + n * torch.eye(n, dtype=dtype)


def _bytes(t):
    return t.cpu().contiguous().numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 17, 63, 64, 65, 100, 128, 130, 448, 500, 512])
def test_factor_and_every_dinv_block(dtype, n):
    if dtype.is_complex and n == 100:
        n = 60
    a = _spd(n, dtype, 3)
    tile = a.to("cuda")
    dinv = ops.potrf_tile(tile)
    torch.cuda.synchronize()
    ref = torch.linalg.cholesky(a.to(_wide(dtype)))
    got = torch.tril(tile.cpu().to(ref.dtype))
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"factor err={err:.3e} scale={scale:.3e}")
    assert err <= _tol(dtype, n) * scale * 10, f"err={err}"

    bsz = dinv.shape[-1]
    nblocks = (n + bsz - 1) // bsz
    assert dinv.shape[0] == nblocks
    for d in range(nblocks):
        c0 = d * bsz
        bs = min(bsz, n - c0)
        dd = dinv[d].cpu()
        prod = dd[:bs, :bs].to(ref.dtype) @ ref[c0:c0 + bs, c0:c0 + bs]
        err = (prod - torch.eye(bs, dtype=ref.dtype)).abs().max().item()
        print(f"dinv[{d}] err={err:.3e}")
        assert err <= _tol(dtype, n) * 100, f"dinv[{d}] err={err}"
        # outside the live part: exactly the identity
        ext = dd.clone()
        ext[:bs, :bs] = 0
        want = torch.eye(bsz, dtype=dtype)
        want[:bs, :bs] = 0
        assert torch.equal(ext, want), f"dinv[{d}] not identity-extended"
        # the inverse of a lower-triangular block is lower triangular
        assert torch.equal(torch.triu(dd, 1), torch.zeros_like(dd))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [130, 500])
def test_strided_view_no_stray_writes(dtype, n):
    r0, c0 = 3, 5
    buf = torch.full((n + 7, n + 13), float("nan"), dtype=dtype, device="cuda")
    a = _spd(n, dtype, 5)
    buf[r0:r0 + n, c0:c0 + n] = a.to("cuda")
    before = buf.cpu().clone()
    tile = buf[r0:r0 + n, c0:c0 + n]
    assert tile.stride(0) > n
    ops.potrf_tile(tile)
    torch.cuda.synchronize()
    after = buf.cpu().clone()
    ref = torch.linalg.cholesky(a.to(_wide(dtype)))
    got = torch.tril(after[r0:r0 + n, c0:c0 + n].to(ref.dtype))
    err = (got - ref).abs().max().item()
    assert err <= _tol(dtype, n) * ref.abs().max().item() * 10, f"err={err}"
    # blank the lower triangle of the window on both sides; everything else
    # (outside the window, and the strict upper triangle inside) is untouched
    for t in (before, after):
        w = t[r0:r0 + n, c0:c0 + n]
        w.copy_(torch.triu(w, 1))
    assert _bytes(before) == _bytes(after)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
@pytest.mark.parametrize("fail_at", [70, 0])
def test_failed_pivot(dtype, fail_at):
    n = 128
    a = _spd(n, dtype, 7)
    ref = torch.linalg.cholesky(a)
    # make the pivot at fail_at equal to -1: the leading minor of order
    # fail_at + 1 is the first non-positive one
    row = ref[fail_at, :fail_at]
    a[fail_at, fail_at] = (row * row.conj()).sum().real - 1.0
    _, info = torch.linalg.cholesky_ex(a)
    assert int(info) == fail_at + 1
    tile = a.to("cuda")
    ops.potrf_tile(tile)
    torch.cuda.synchronize()
    got = tile.cpu()
    diag = torch.diagonal(got)
    nan = torch.isnan(diag.real) | (torch.isnan(diag.imag) if dtype.is_complex else False)
    assert bool(nan[fail_at]), "no NaN on the failed pivot"
    assert not bool(nan[:fail_at].any()), "NaN before the failed pivot"
    if fail_at:
        # columns before the failed pivot do not depend on it
        gl = torch.tril(got)[:, :fail_at]
        err = (gl - ref[:, :fail_at]).abs().max().item()
        assert err <= _tol(dtype, n) * ref.abs().max().item() * 10, f"err={err}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 37])
def test_invert_only_block(dtype, n):
    torch.manual_seed(11)
    bsz = ops.potrf_bsz(dtype)
    L = torch.tril(_rand((n, n), dtype).cpu()) + 2 * n ** 0.5 * torch.eye(n, dtype=dtype)
    # the strict upper triangle of an already-factored tile is not read
    blk = L + torch.triu(torch.full((n, n), float("nan"), dtype=dtype), 1)
    dev = blk.to("cuda")
    before = _bytes(dev)
    out = torch.full((bsz, bsz), float("nan"), dtype=dtype, device="cuda")
    ops.get_ext().factor_invert_block(dev, n, dev.stride(0), out, False)
    torch.cuda.synchronize()
    assert _bytes(dev) == before, "invert-only wrote the block"
    T = out.cpu()
    w = _wide(dtype)
    err = (T[:n, :n].to(w) @ L.to(w) - torch.eye(n, dtype=w)).abs().max().item()
    assert err <= _tol(dtype, n) * 100, f"err={err}"
    rest = T.clone()
    rest[:n, :n] = 0
    want = torch.eye(bsz, dtype=dtype)
    want[:n, :n] = 0
    assert torch.equal(rest, want)
    assert torch.equal(torch.triu(T, 1), torch.zeros_like(T))


def test_bitwise_under_load():
    """potrf_tile on the high-priority stream while a batch of 512^3 tile
    products fills the GPU from another stream: same bits as run alone, for
    three tiles back to back through one dinv and one side workspace."""
    from dlaf_amd.runtime import get_runtime

    nb, dtype, dev = 512, torch.float64, torch.device("cuda", torch.cuda.current_device())
    tiles = [_spd(nb, dtype, 20 + i).to(dev) for i in range(3)]
    solo = []
    for t in tiles:
        x = t.clone()
        dinv = ops.potrf_tile(x)
        torch.cuda.synchronize()
        solo.append((_bytes(x), _bytes(dinv)))

    nt = 256
    A = torch.randn(nt, nb, nb, dtype=dtype, device=dev)
    C = torch.zeros_like(A)
    ts = nb * nb
    offs = [i * ts for i in range(nt)]
    descs = torch.from_numpy(ops.make_descs(offs, offs, offs)).to(dev)
    rt = get_runtime(dev)
    hp, lo = rt.hp_streams[0], rt.np_streams[0]
    work = [t.clone() for t in tiles]
    dinv = ops.dinv_workspace(nb, dtype, dev)
    got = []
    torch.cuda.synchronize()
    with torch.cuda.stream(lo):
        for _ in range(2):
            ops.gemm_fused(C, A, A, descs, nb, nb, nb, nb, nb, nb, Op.NoTrans, Op.Trans, 1.0, 0.0)
    with torch.cuda.stream(hp):
        side = ops.potrf_side_workspace(nb, dtype, dev)
        for x in work:
            ops.potrf_tile(x, dinv)
            assert ops.potrf_side_workspace(nb, dtype, dev) is side
            got.append(dinv.clone())
    busy = not lo.query()  # the GEMM batch was still running when the last tile was queued
    torch.cuda.synchronize()
    print(f"gemm batch still running after queuing: {busy}")
    for i in range(3):
        assert _bytes(work[i]) == solo[i][0], f"tile {i} differs under load"
        assert _bytes(got[i]) == solo[i][1], f"dinv of tile {i} differs under load"
