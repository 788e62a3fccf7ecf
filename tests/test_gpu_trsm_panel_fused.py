"""Single-launch panel TRSM (csrc/trsm_panel.hip): X <- X * tril(L)^-H for a
list of tiles, against ``torch.linalg.solve_triangular`` in float64 on the CPU.

The bound is that of ``test_gpu_kernels.test_trsm_panel``,
``_tol(dtype, nb) * (max|ref| + 1) * 100``. The blocked recurrence itself, run
on the CPU in the working precision at these shapes, sits at 1e-16 (double)
and 1e-7 (single), six and five orders under it.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dlaf_amd.ops import tile_ops as ops  # noqa: E402
from dlaf_amd.types import Op  # noqa: E402
from test_gpu_kernels import _rand, _tol  # noqa: E402

DTYPES = [dt for dt in (torch.float64, torch.float32, torch.complex128,
                        torch.complex64) if ops.has_trsm_panel_fused(dt)]


def _wide(dtype):
    return torch.complex128 if dtype.is_complex else torch.float64


def _bytes(t):
    return t.cpu().contiguous().numpy().tobytes()


def _factor(nb, dtype, seed, dinv_from):
    """(L on the GPU with NaN in its strict upper triangle, dinv, tril(L) in
    the wide type on the CPU) for the Cholesky factor of a a^H + nb I."""
    torch.manual_seed(seed)
    a = _rand((nb, nb), dtype).cpu()
    a = a @ a.mH + nb * torch.eye(nb, dtype=dtype)
    bsz = ops.potrf_bsz(dtype)
    nblocks = (nb + bsz - 1) // bsz
    if dinv_from == "potrf":
        L = a.to("cuda")
        dinv = ops.potrf_tile(L)
    else:
        L = torch.linalg.cholesky(a).contiguous().to("cuda")
        # only the live bs x bs part of a block is written: whatever lies
        # outside it must not be read
        dinv = torch.full((nblocks, bsz, bsz), float("nan"), dtype=dtype,
                          device="cuda")
        for d in range(nblocks):
            c0 = d * bsz
            bs = min(bsz, nb - c0)
            ops.get_ext().trtri_lower(L[c0:, c0:], dinv[d], bs, L.stride(0),
                                      bsz, False)
    torch.cuda.synchronize()
    Lw = torch.tril(L.cpu().to(_wide(dtype)))
    L += torch.triu(torch.full((nb, nb), float("nan"), dtype=dtype,
                               device="cuda"), 1)
    return L, dinv, Lw


def _ref(Lw, x):
    return torch.linalg.solve_triangular(Lw.mH, x.cpu().to(Lw.dtype),
                                         upper=True, left=False)


def _check(got, ref, dtype, nb, what):
    err = (got.cpu().to(ref.dtype) - ref).abs().max().item()
    scale = ref.abs().max().item() + 1
    bound = _tol(dtype, nb) * scale * 100
    print(f"{what}: err={err:.3e} bound={bound:.3e}")
    assert np.isfinite(err) and err <= bound, f"{what}: err={err} bound={bound}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dinv_from", ["potrf", "trtri"])
@pytest.mark.parametrize("mb,nb", [(1, 1), (17, 17), (64, 64), (65, 65),
                                   (130, 130), (448, 448), (512, 512),
                                   (70, 130)])
def test_solve_against_reference(dtype, dinv_from, mb, nb):
    L, dinv, Lw = _factor(nb, dtype, 5, dinv_from)
    ntiles = 3
    panel = _rand((ntiles, mb, nb), dtype)
    x0 = panel.clone()
    offs = [i * mb * nb for i in range(ntiles)]
    ops.trsm_panel_right_lowerH(panel, offs, L, dinv, mb, nb, nb)
    torch.cuda.synchronize()
    for i in range(ntiles):
        _check(panel[i], _ref(Lw, x0[i]), dtype, nb, f"tile {i}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strip", [16, 32])
def test_every_strip_height(dtype, strip):
    """The strip height is chosen from the call shape; both kernels are also
    run directly, with a ragged last strip and block."""
    mb, nb, ntiles = 150, 200, 2
    L, dinv, Lw = _factor(nb, dtype, 6, "potrf")
    panel = _rand((ntiles, mb, nb), dtype)
    x0 = panel.clone()
    offs = torch.tensor([i * mb * nb for i in range(ntiles)], device="cuda")
    ops.trsm_panel_fused(panel, offs, L, dinv, mb, nb, nb, strip=strip)
    torch.cuda.synchronize()
    for i in range(ntiles):
        _check(panel[i], _ref(Lw, x0[i]), dtype, nb, f"strip {strip} tile {i}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb", [130, 500])
def test_no_stray_accesses(dtype, nb):
    """Tiles scattered inside a NaN-filled buffer with ld > nb: bytes outside
    the tiles stay as they were and no NaN reaches a result."""
    mb, ld = nb - 3, nb + 7
    span = (mb - 1) * ld + nb
    offs = [2 * span + 40, 11, span + 23]  # out of order, with gaps
    buf = torch.full((3 * span + 64,), float("nan"), dtype=dtype, device="cuda")
    L, dinv, Lw = _factor(nb, dtype, 7, "potrf")
    x0 = _rand((len(offs), mb, nb), dtype)

    def window(t, o):
        return t[o:o + mb * ld + nb - ld].as_strided((mb, nb), (ld, 1))

    for i, o in enumerate(offs):
        window(buf, o).copy_(x0[i])
    before = buf.cpu().clone()
    ops.trsm_panel_right_lowerH(buf, offs, L, dinv, mb, nb, ld)
    torch.cuda.synchronize()
    after = buf.cpu().clone()
    for i, o in enumerate(offs):
        got = window(after, o).clone()
        assert bool(torch.isfinite(got).all()), f"tile {i} not finite"
        _check(got, _ref(Lw, x0[i]), dtype, nb, f"tile {i}")
    for t in (before, after):
        for o in offs:
            window(t, o).zero_()
    assert _bytes(before) == _bytes(after), "bytes outside the tiles changed"


@pytest.mark.parametrize("dtype", DTYPES)
def test_old_path_against_new(dtype):
    nb, ntiles = 256, 3
    L, dinv, Lw = _factor(nb, dtype, 8, "potrf")
    x0 = _rand((ntiles, nb, nb), dtype)
    offs = [i * nb * nb for i in range(ntiles)]
    old, new = x0.clone(), x0.clone()
    ops.trsm_panel_right_lowerH(old, offs, L, dinv, nb, nb, nb, fused=False)
    ops.trsm_panel_right_lowerH(new, offs, L, dinv, nb, nb, nb, fused=True)
    torch.cuda.synchronize()
    for i in range(ntiles):
        _check(new[i], old[i].cpu().to(_wide(dtype)), dtype, nb, f"tile {i}")


def test_bitwise_repeat_and_under_load():
    """Two runs give the same bytes, and so does a run on the high-priority
    stream while a batch of 512^3 tile products fills the GPU from another."""
    from dlaf_amd.runtime import get_runtime

    nb, dtype = 512, torch.float64
    dev = torch.device("cuda", torch.cuda.current_device())
    L, dinv, _ = _factor(nb, dtype, 9, "potrf")
    ntiles = 3
    x0 = _rand((ntiles, nb, nb), dtype)
    offs = torch.tensor([i * nb * nb for i in range(ntiles)], device=dev)
    runs = []
    for _ in range(2):
        x = x0.clone()
        ops.trsm_panel_fused(x, offs, L, dinv, nb, nb, nb)
        torch.cuda.synchronize()
        runs.append(_bytes(x))
    assert runs[0] == runs[1], "two solo runs differ"

    nt = 256
    A = torch.randn(nt, nb, nb, dtype=dtype, device=dev)
    C = torch.zeros_like(A)
    ts = nb * nb
    boffs = [i * ts for i in range(nt)]
    descs = torch.from_numpy(ops.make_descs(boffs, boffs, boffs)).to(dev)
    rt = get_runtime(dev)
    hp, lo = rt.hp_streams[0], rt.np_streams[0]
    x = x0.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(lo):
        for _ in range(2):
            ops.gemm_fused(C, A, A, descs, nb, nb, nb, nb, nb, nb,
                           Op.NoTrans, Op.Trans, 1.0, 0.0)
    with torch.cuda.stream(hp):
        ops.trsm_panel_fused(x, offs, L, dinv, nb, nb, nb)
    busy = not lo.query()
    torch.cuda.synchronize()
    print(f"gemm batch still running after queuing: {busy}")
    assert _bytes(x) == runs[0], "run under load differs from the solo run"

