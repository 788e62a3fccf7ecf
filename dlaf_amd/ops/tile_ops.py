"""Mid-level tile operations with CPU (torch) / GPU (native HIP) dispatch.

The GPU path is descriptor-driven and FUSED: one call covers a list of tile
triples and becomes one kernel launch. ``ext.batch_gemm`` enters
csrc/gemm_tiles.hip, which runs full-tile non-aliased batches on the glds
kernels of csrc/gemm_tiles_v2.hip and edge shapes / in-place panel applies on
its own guarded kernels; every batch runs on these in-tree kernels. The CPU
path loops over tiles with torch.linalg — it is the reference backend (the analog of the
reference's Backend::MC per-tile blaspp/lapackpp calls) and the
oracle the GPU kernels are tested against.

Conventions: tiles are row-major views; ``op`` follows dlaf_amd.types.Op;
for real dtypes ConjTrans == Trans. Triangular solves on GPU are performed
against block inverses (see csrc/factor.hip docstring).
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ..types import Op, is_complex
from ._ext import get_ext, has_ext

_OP_CODE = {Op.NoTrans: 0, Op.Trans: 1, Op.ConjTrans: 2}


def _opc(op: Op) -> int:
    return _OP_CODE[op]


def _alpha_parts(alpha) -> Tuple[float, float]:
    c = complex(alpha)
    return (c.real, c.imag)


def make_descs(c_offs, a_offs, b_offs, ktiles=1, a_kstride=0, b_kstride=0) -> np.ndarray:
    """[n, 6] int64 GemmDesc table (csrc/kernels.h). Offsets are per row;
    ``ktiles`` and the K strides are scalars or per-row sequences."""
    n = len(c_offs)
    d = np.empty((n, 6), dtype=np.int64)
    d[:, 0] = np.asarray(c_offs, dtype=np.int64)
    d[:, 1] = np.asarray(a_offs, dtype=np.int64)
    d[:, 2] = np.asarray(b_offs, dtype=np.int64)
    d[:, 3] = ktiles
    d[:, 4] = a_kstride
    d[:, 5] = b_kstride
    return d


def gemm_fused(
    C_base: torch.Tensor,
    A_base: torch.Tensor,
    B_base: torch.Tensor,
    descs,
    M: int,
    N: int,
    K: int,
    lda: int,
    ldb: int,
    ldc: int,
    opA: Op,
    opB: Op,
    alpha,
    beta,
    inplace: bool = False,
) -> None:
    """GPU fused batched GEMM. ``descs``: np.ndarray [n,6] or device tensor.

    Set ``inplace=True`` when a desc's C block aliases its A block (panel
    applies) — it selects the kernel geometry that reads all of A before
    writing C.
    """
    ext = get_ext()
    if isinstance(descs, np.ndarray):
        descs = torch.from_numpy(descs).to(C_base.device, non_blocking=True)
    ar, ai = _alpha_parts(alpha)
    br, bi = _alpha_parts(beta)
    # In-place safety: the kernels guarantee X = X*op(B) in place only while
    # one column block spans all of N (every workgroup reads all of its A
    # rows before any C write). Wider N would let a finished workgroup's C
    # epilogue race another's A reads — stage op(A)'s tiles into a scratch
    # buffer and run the ordinary non-aliased kernel instead.
    bn_safe = 64 if C_base.dtype.is_complex else 128
    if inplace and N > bn_safe and C_base.is_cuda:
        assert opA is Op.NoTrans, "in-place staging implemented for opA=N"
        dd = descs.view(-1, 6)
        assert int(dd[:, 3].max()) <= 1, "in-place staging expects ktiles == 1"
        nd = dd.shape[0]
        af = A_base.reshape(-1)
        ridx = torch.arange(M, device=C_base.device, dtype=torch.int64) * lda
        kidx = torch.arange(K, device=C_base.device, dtype=torch.int64)
        idx = dd[:, 1].view(nd, 1, 1) + ridx.view(1, M, 1) + kidx.view(1, 1, K)
        scratch = af.index_select(0, idx.reshape(-1)).view(nd, M, K)
        dd2 = dd.clone()
        dd2[:, 1] = torch.arange(nd, device=C_base.device, dtype=torch.int64) * (M * K)
        ext.batch_gemm(
            C_base.reshape(-1), scratch.reshape(-1), B_base.reshape(-1), dd2,
            M, N, K, K, ldb, ldc, _opc(opA), _opc(opB), ar, ai, br, bi, False,
        )
        return
    ext.batch_gemm(
        C_base.reshape(-1), A_base.reshape(-1), B_base.reshape(-1), descs,
        M, N, K, lda, ldb, ldc, _opc(opA), _opc(opB), ar, ai, br, bi, inplace,
    )


def ptr_array(base: torch.Tensor, offs) -> torch.Tensor:
    """Device int64 array of addresses base.data_ptr() + off*itemsize for the
    rocBLAS pointer-array batched path. ``offs`` in element units."""
    if not torch.is_tensor(offs):
        offs = torch.as_tensor(offs, dtype=torch.int64)
    offs = offs.to(base.device, torch.int64, non_blocking=True)
    return offs * base.element_size() + base.data_ptr()


def gemm_batched_lib(dt_ref: torch.Tensor, ptrC: torch.Tensor, ptrA: torch.Tensor,
                     ptrB: torch.Tensor, M: int, N: int, K: int,
                     lda: int, ldb: int, ldc: int, opA: Op, opB: Op,
                     alpha, beta) -> None:
    """rocBLAS batched GEMM over precomputed device pointer arrays.

    Uniform-shape batches only (one K-product per C tile, no aliasing among
    C entries). No algorithm routes here: the glds fused kernel matches it on
    the uniform nb=512 f64 trailing shape (62.8 vs 62.5 TF in one probe). It
    stays as the comparison point of ``tools/microbench.py``.
    """
    ar, ai = _alpha_parts(alpha)
    br, bi = _alpha_parts(beta)
    get_ext().lib_gemm_batched(dt_ref, ptrC, ptrA, ptrB, M, N, K,
                               lda, ldb, ldc, _opc(opA), _opc(opB), ar, ai, br, bi)


def _t(x: torch.Tensor, op: Op) -> torch.Tensor:
    if op is Op.NoTrans:
        return x
    if op is Op.Trans:
        return x.mT
    return x.mH


def gemm_tile(C: torch.Tensor, A: torch.Tensor, B: torch.Tensor, opA: Op, opB: Op, alpha, beta) -> None:
    """CPU single-tile GEMM: C = alpha*op(A)op(B) + beta*C."""
    prod = _t(A, opA) @ _t(B, opB)
    if beta == 0:
        C.copy_(alpha * prod)
    else:
        C.mul_(beta).add_(prod, alpha=alpha)


# ---------------- factorization tile ops ----------------

def potrf_bsz(dtype: torch.dtype) -> int:
    """Diagonal-block size of the tile Cholesky: the extension's
    ``kPotrfBsz`` (csrc/kernels.h), the same for every dtype. CPU-only
    installs without the extension use the same 64."""
    return get_ext().POTRF_BSZ if has_ext() else 64


def dinv_workspace(nb: int, dtype: torch.dtype, device) -> torch.Tensor:
    bsz = potrf_bsz(dtype)
    nblocks = (nb + bsz - 1) // bsz
    return torch.empty((nblocks, bsz, bsz), dtype=dtype, device=device)


_POTRF_SIDE_CACHE = {}


def potrf_side_workspace(nb: int, dtype: torch.dtype, device) -> torch.Tensor:
    """Side workspace of the fused tile Cholesky (two halves of nb x bsz, see
    csrc/potrf_plan.h), cached per (nb, dtype, device) and per stream: it
    carries nothing between calls, but two calls running at once must not
    share one."""
    device = torch.device(device)
    key = (nb, dtype, str(device), torch.cuda.current_stream(device).cuda_stream)
    t = _POTRF_SIDE_CACHE.get(key)
    if t is None:
        bsz = potrf_bsz(dtype)
        nblocks = (nb + bsz - 1) // bsz
        t = torch.empty((2, nblocks * bsz, bsz), dtype=dtype, device=device)
        _POTRF_SIDE_CACHE[key] = t
    return t


def potrf_tile(tile: torch.Tensor, dinv: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """In-place lower Cholesky of a padded tile.

    On GPU also fills/returns ``dinv`` (diagonal-block inverses) for the panel
    TRSM-as-GEMM. On CPU returns None (panel solve uses solve_triangular).
    """
    n = tile.shape[0]
    assert tile.shape[0] == tile.shape[1] and tile.stride(1) == 1
    if tile.is_cuda:
        if dinv is None:
            dinv = dinv_workspace(n, tile.dtype, tile.device)
        side = potrf_side_workspace(n, tile.dtype, tile.device)
        get_ext().potrf_tile(tile, n, tile.stride(0), dinv, side)
        return dinv
    L, inf = torch.linalg.cholesky_ex(tile)
    tile.copy_(L)
    if int(inf) > 0:
        # match the GPU kernel's failure mode (sqrt of a bad pivot -> NaN on
        # that diagonal) so callers detect non-SPD inputs uniformly via the
        # diagonal scan in capi._potrf_info
        tile[int(inf) - 1, int(inf) - 1] = float("nan")
    return None


def trtri_tile(L: torch.Tensor, out: torch.Tensor, unit_diag: bool = False) -> None:
    """out = tril(L)^-1 (full tile written: upper part zeroed)."""
    n = L.shape[0]
    if L.is_cuda:
        get_ext().trtri_lower(L, out, n, L.stride(0), out.stride(0), unit_diag)
        return
    eye = torch.eye(n, dtype=L.dtype, device=L.device)
    T = torch.linalg.solve_triangular(
        torch.tril(L) if not unit_diag else torch.tril(L, -1) + eye,
        eye, upper=False, unitriangular=unit_diag,
    )
    out.copy_(torch.tril(T))


def gemm_items(
    C_base: torch.Tensor,
    A_base: torch.Tensor,
    B_base: torch.Tensor,
    items: Sequence[Tuple[int, int, int]],
    nb: int,
    opA: Op,
    opB: Op,
    alpha,
    beta,
    inplace: bool = False,
) -> None:
    """Tile-triple GEMM over element offsets into flat bases, CPU or GPU.

    ``items``: sequence of (c_off, a_off, b_off). GPU: ONE fused kernel launch.
    CPU: loop over reshaped nb x nb views (the reference MC backend analog).
    """
    if not len(items):
        return
    if C_base.is_cuda:
        c, a, b = zip(*items)
        gemm_fused(C_base, A_base, B_base, make_descs(c, a, b),
                   nb, nb, nb, nb, nb, nb, opA, opB, alpha, beta, inplace=inplace)
        return
    ts = nb * nb
    cv, av, bv = C_base.reshape(-1), A_base.reshape(-1), B_base.reshape(-1)
    for c, a, b in items:
        gemm_tile(cv[c:c + ts].view(nb, nb), av[a:a + ts].view(nb, nb),
                  bv[b:b + ts].view(nb, nb), opA, opB, alpha, beta)


def tri_inverse_full(A: torch.Tensor, lower: bool, unit: bool = False) -> torch.Tensor:
    """Full-tile inverse of a triangular tile (other triangle zeroed).

    GPU: native column-parallel ``trtri_lower`` kernel (upper handled via
    T = (trtri_lower(A^H))^H). CPU: solve_triangular against the identity.
    Used by the TRSM/TRMM/inverse algorithms to turn per-tile triangular
    solves into fused GEMMs (TRSM-as-GEMM, see csrc/factor.hip).
    """
    n = A.shape[0]
    if A.is_cuda:
        if lower:
            return _tri_inv_lower_gpu(A, unit)
        # resolve_conj: for n == 1 the adjoint view is already contiguous, so
        # contiguous() alone leaves a lazy conjugate bit the kernel never sees
        tmp = A.mH.contiguous().resolve_conj()
        return _tri_inv_lower_gpu(tmp, unit).mH.contiguous().resolve_conj()
    eye = torch.eye(n, dtype=A.dtype, device=A.device)
    if unit:
        tri = torch.tril(A, -1) + eye if lower else torch.triu(A, 1) + eye
    else:
        tri = torch.tril(A) if lower else torch.triu(A)
    return torch.linalg.solve_triangular(tri, eye, upper=not lower, unitriangular=False)


def _tri_inv_lower_gpu(L: torch.Tensor, unit: bool) -> torch.Tensor:
    """Recursive blocked lower-triangular inverse on GPU.

    inv([[A, 0], [B, C]]) = [[inv(A), 0], [-inv(C) B inv(A), inv(C)]]:
    two half-size recursions + two GEMMs; base case = the native
    column-parallel ``trtri_lower`` kernel (fast at <= 128). Replaces a
    single large trtri launch that serializes over columns (21.9 ms for a
    512 tile -> ~0.2 ms).
    """
    n = L.shape[0]
    if n <= 128:
        out = torch.empty_like(L) if L.stride(1) == 1 else \
            torch.empty((n, n), dtype=L.dtype, device=L.device)
        Lc = L if L.stride(1) == 1 else L.contiguous()
        get_ext().trtri_lower(Lc, out, n, Lc.stride(0), out.stride(0), unit)
        return out
    h = ((n + 1) // 2 + 63) // 64 * 64
    h = min(h, n - 1)
    Ai = _tri_inv_lower_gpu(L[:h, :h], unit)
    Ci = _tri_inv_lower_gpu(L[h:, h:], unit)
    out = torch.zeros((n, n), dtype=L.dtype, device=L.device)
    out[:h, :h] = Ai
    out[h:, h:] = Ci
    out[h:, :h] = -(Ci @ (L[h:, :h] @ Ai))
    return out


def tri_inverse_full_many(tiles, lower: bool = True, unit: bool = False):
    """tri_inverse_full over a list of independent tiles, overlapped across
    the runtime's streams (each inverse is a chain of single/few-workgroup
    launches — serial on one stream, they cover each other's latency on
    several; measured 42 ms -> ~12 ms for 64 nb=512 f64 tiles)."""
    tiles = list(tiles)
    if not tiles:
        return []
    if not tiles[0].is_cuda or len(tiles) == 1:
        return [tri_inverse_full(t, lower, unit) for t in tiles]
    from ..runtime import get_runtime
    rt = get_runtime(tiles[0].device)
    streams = list(rt.np_streams) + list(rt.hp_streams)
    cur = torch.cuda.current_stream(tiles[0].device)
    outs = [None] * len(tiles)
    used = streams[: min(len(streams), len(tiles))]
    for st in used:
        st.wait_stream(cur)
    for i, t in enumerate(tiles):
        with torch.cuda.stream(used[i % len(used)]):
            outs[i] = tri_inverse_full(t, lower, unit)
    for st in used:
        cur.wait_stream(st)
    for o in outs:
        o.record_stream(cur)
    return outs


def tri_mask(A: torch.Tensor, lower: bool, unit: bool = False) -> torch.Tensor:
    """Masked copy of a triangular tile (for TRMM diag-block multiplies)."""
    if unit:
        eye = torch.eye(A.shape[0], dtype=A.dtype, device=A.device)
        return (torch.tril(A, -1) if lower else torch.triu(A, 1)) + eye
    return torch.tril(A) if lower else torch.triu(A)


def has_trsm_panel_fused(dtype: torch.dtype) -> bool:
    """Whether ``dtype`` has the single-launch panel TRSM kernel
    (csrc/trsm_panel.hip): the real types. The others run the blocked solve
    as ``gemm_fused`` launches."""
    return dtype in (torch.float64, torch.float32)


def trsm_panel_fused(panel_base: torch.Tensor, tile_offs: torch.Tensor,
                     L_diag: torch.Tensor, dinv: torch.Tensor, mb: int,
                     nb: int, ld: int, strip: int = 0) -> None:
    """X <- X * tril(L)^-H in ONE launch for the tiles (mb x nb, row stride
    ``ld``) at the element offsets ``tile_offs`` (device int64, each tile
    inside ``panel_base``: the kernel cannot check them). ``strip`` = 0 leaves
    the strip height to the kernel."""
    assert L_diag.stride(1) == 1
    get_ext().trsm_panel(panel_base.reshape(-1), tile_offs, L_diag,
                         L_diag.stride(0), dinv, mb, nb, ld, strip)


def trsm_panel_right_lowerH(
    panel_base: torch.Tensor,
    tile_offs: Sequence[int],
    L_diag: torch.Tensor,
    dinv: torch.Tensor,
    mb: int,
    nb: int,
    ld: int,
    fused: Optional[bool] = None,
) -> None:
    """Solve X * op(L)^H = X for every panel tile in place (L lower-triangular).

    GPU blocked algorithm per inner block d (bsz = dinv block size):
        X[:, d] -= X[:, :d] @ L[d, :d]^H
        X[:, d]  = X[:, d] @ dinv[d]^H
    Real dtypes run all of it in one launch (``trsm_panel_fused``); complex
    dtypes, and ``fused=False``, run two ``gemm_fused`` launches per block,
    each fused over all panel tiles. This is the panel step of right-looking
    Cholesky (reference ``factorization/cholesky/impl.h:151-189``
    trsmPanelTile).
    """
    assert panel_base.is_cuda
    if fused is None:
        fused = has_trsm_panel_fused(panel_base.dtype)
    if fused:
        offs = np.asarray(tile_offs, dtype=np.int64)
        if len(offs) == 0:
            return
        assert offs.min() >= 0 and \
            int(offs.max()) + (mb - 1) * ld + nb <= panel_base.numel(), \
            "tile outside the panel base"
        trsm_panel_fused(panel_base,
                         torch.from_numpy(offs).to(panel_base.device),
                         L_diag, dinv, mb, nb, ld)
        return
    opc = Op.ConjTrans if is_complex(panel_base.dtype) else Op.Trans
    bsz = dinv.shape[-1]
    nblocks = (nb + bsz - 1) // bsz
    offs = np.asarray(tile_offs, dtype=np.int64)
    ld_l = L_diag.stride(0)
    for d in range(nblocks):
        c0 = d * bsz
        bs = min(bsz, nb - c0)
        if d > 0:
            # X[:, c0:c0+bs] -= X[:, :c0] @ (L[c0:c0+bs, :c0])^H
            descs = make_descs(offs + c0, offs, [c0 * ld_l] * len(offs))
            gemm_fused(
                panel_base, panel_base, L_diag, descs,
                mb, bs, c0, ld, ld_l, ld,
                Op.NoTrans, opc, -1.0, 1.0,
            )
        # X[:, c0:c0+bs] @= dinv[d]^H  (in place; wide-BN kernel variant)
        descs = make_descs(offs + c0, offs + c0, [0] * len(offs))
        gemm_fused(
            panel_base, panel_base, dinv[d], descs,
            mb, bs, bs, ld, bsz, ld,
            Op.NoTrans, opc, 1.0, 0.0, inplace=True,
        )


# ---------------- LU with partial pivoting ----------------

def _cabs1(x: torch.Tensor) -> torch.Tensor:
    """|re| + |im|: the magnitude LAPACK's i?amax compares."""
    return x.real.abs() + x.imag.abs() if x.is_complex() else x.abs()


def lu_panel(storage: torch.Tensor, n: int, k: int, ipiv: torch.Tensor,
             info: torch.Tensor) -> None:
    """In-place LU with partial pivoting of tile column ``k`` of the square
    storage ``[nt, nt, nb, nb]``: rows ``k*nb .. n-1``, columns ``k*nb ..
    min((k+1)*nb, n)-1``. The pivot of a column is the FIRST row of the
    largest CABS1 value; a zero pivot leaves its column unscaled and puts its
    1-based index into ``info`` (one int32) unless one is there already.
    ``ipiv[g]`` (int32, 0-based) is set for the panel's columns; the
    interchanges are applied to the panel's own columns only.

    GPU: csrc/lu_panel.hip (a missing extension raises). CPU: the same rule
    in plain torch, column by column."""
    if storage.is_cuda:
        get_ext().lu_panel(storage, n, k, ipiv, info)
        return
    nt, nb = storage.shape[0], storage.shape[2]
    g0 = k * nb
    m = n - g0
    if m <= 0:
        return
    nc = min(nb, m)
    P = storage[k:, k].reshape(-1, nb)[:m, :nc].clone()
    for j in range(nc):
        p = j + int(torch.argmax(_cabs1(P[j:, j])))  # first maximum
        ipiv[g0 + j] = g0 + p
        if p != j:
            P[[j, p]] = P[[p, j]]
        piv = P[j, j]
        if piv == 0:
            if int(info[0]) == 0:
                info[0] = g0 + j + 1
            continue
        P[j + 1:, j] = P[j + 1:, j] / piv
        if j + 1 < nc:
            P[j + 1:, j + 1:] -= torch.outer(P[j + 1:, j], P[j, j + 1:])
    for i in range(k, nt):
        r0 = (i - k) * nb
        rows = min(nb, m - r0)
        storage[i, k, :rows, :nc] = P[r0:r0 + rows]


def laswp(storage: torch.Tensor, ipiv: torch.Tensor, s0: int, s1: int,
          c0: int, c1: int, reverse: bool = False) -> None:
    """Row interchanges on a ``[lr, lc, mb, nb]`` tile storage: for s in
    ``[s0, s1)`` (from ``s1 - 1`` down when ``reverse``) rows s and
    ``ipiv[s]`` (0-based) swap in the element columns ``[c0, c1)``."""
    if s1 <= s0 or c1 <= c0:
        return
    if storage.is_cuda:
        get_ext().laswp_tiles(storage, ipiv, s0, s1, c0, c1, reverse)
        return
    mb, nb = storage.shape[2], storage.shape[3]
    piv = ipiv[s0:s1].tolist()
    order = range(s1 - 1, s0 - 1, -1) if reverse else range(s0, s1)
    for s in order:
        p = piv[s - s0]
        if p == s:
            continue
        x = storage[s // mb, :, s % mb, :]
        y = storage[p // mb, :, p % mb, :]
        for j in range(c0 // nb, (c1 - 1) // nb + 1):
            lo, hi = max(c0 - j * nb, 0), min(c1 - j * nb, nb)
            tmp = x[j, lo:hi].clone()
            x[j, lo:hi] = y[j, lo:hi]
            y[j, lo:hi] = tmp


def pivots_to_permutation(ipiv: torch.Tensor) -> torch.Tensor:
    """int64 ``perm`` with ``(P B)[i] = B[perm[i]]`` for the interchanges
    ``ipiv`` applied in order: the interchanges run once on the index vector
    (on the device through ``laswp``'s kernel, nothing read back)."""
    n = ipiv.shape[0]
    if ipiv.is_cuda:
        v = torch.arange(n, dtype=torch.float64, device=ipiv.device)
        if n:
            laswp(v.view(1, 1, n, 1), ipiv, 0, n, 0, 1)
        return v.to(torch.int64)
    perm = list(range(n))
    for j, p in enumerate(ipiv.tolist()):
        perm[j], perm[p] = perm[p], perm[j]
    return torch.tensor(perm, dtype=torch.int64)
