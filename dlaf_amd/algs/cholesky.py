"""Tiled Cholesky factorization (POTRF), local and distributed.

Counterpart of the reference's ``factorization/cholesky/impl.h`` (local
151-189, distributed 192-313): right-looking algorithm

    for k:  L_kk = potrf(A_kk)
            L_ik = A_ik * L_kk^-H              (panel TRSM, i > k)
            A_ij -= L_ik * L_jk^H              (trailing HERK/GEMM, i >= j > k)

MI355X-native differences from the reference:
* per-tile task flood -> FUSED kernels: the whole panel solve is ONE launch
  per k in the real dtypes (csrc/trsm_panel.hip; a handful of launches in the
  complex ones) and the whole trailing update is ONE launch per k (descriptor
  list over the rank's local tiles);
* panel TRSM runs against diagonal-block inverses computed during potrf_tile
  (TRSM-as-GEMM, csrc/factor.hip);
* every GemmDesc for the whole factorization is precomputed and uploaded to
  the device ONCE per (shape, grid) — the k-loop performs no H2D traffic;
* MPI Ibcast chains -> RCCL broadcasts on the row/col process groups: the
  column panel is ONE contiguous broadcast along the row direction, the
  transposed row panel is per-tile broadcasts along the column direction
  (reference ``broadcast_panel.h:78-189`` semantics).

Lower is described above; local Upper (A = U^H U) runs natively on
upper-stored tiles (``_cholesky_local_upper``) and distributed Upper goes
through a storage transpose to the Lower path.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ..types import UpLo, Op, is_complex
from ..matrix.matrix import Matrix
from ..matrix.panel import Panel
from ..comm.grid import CommGrid
from ..comm import collectives as coll
from ..ops import tile_ops as ops
from ..runtime import get_runtime


def _op_conj(dtype) -> Op:
    return Op.ConjTrans if is_complex(dtype) else Op.Trans


def _cpu_trsm_tile(diag: torch.Tensor, tile: torch.Tensor) -> None:
    # X * diag^H = tile  ->  solve_triangular(diag^H upper, left=False)
    X = torch.linalg.solve_triangular(diag.mH, tile, upper=True, left=False)
    tile.copy_(X)


def _compute_dinv(diag: torch.Tensor, dinv: torch.Tensor) -> torch.Tensor:
    """Diagonal-block inverses of a (lower-triangular) padded tile (GPU)."""
    nb = diag.shape[0]
    bsz = dinv.shape[-1]
    ext = ops.get_ext()
    for d in range((nb + bsz - 1) // bsz):
        c0 = d * bsz
        bs = min(bsz, nb - c0)
        ext.factor_invert_block(diag[c0:, c0:], bs, diag.stride(0), dinv[d], False)
    return dinv


class _DescTable:
    """All GemmDescs of a factorization, device-resident, sliced per step,
    and next to them the per-step tile-offset lists of the single-launch
    panel TRSM (one flat int64 array)."""

    def __init__(self):
        self._rows: List[np.ndarray] = []
        self._index: Dict = {}
        self._dev: Optional[torch.Tensor] = None
        self._n = 0
        self._offs: List[np.ndarray] = []
        self._offs_index: Dict = {}
        self._offs_dev: Optional[torch.Tensor] = None
        self._noffs = 0

    def add(self, key, rows: np.ndarray):
        if len(rows) == 0:
            return
        self._index[key] = (self._n, len(rows))
        self._rows.append(rows)
        self._n += len(rows)

    def add_offs(self, key, offs: np.ndarray):
        if len(offs) == 0:
            return
        self._offs_index[key] = (self._noffs, len(offs))
        self._offs.append(np.asarray(offs, dtype=np.int64))
        self._noffs += len(offs)

    def upload(self, device):
        if self._n:
            cat = np.concatenate(self._rows, axis=0)
            self._dev = torch.from_numpy(cat).to(device)
        if self._noffs:
            self._offs_dev = torch.from_numpy(np.concatenate(self._offs)).to(device)
        self._rows = None
        self._offs = None

    def get_offs(self, key) -> Optional[torch.Tensor]:
        loc = self._offs_index.get(key)
        if loc is None:
            return None
        s, n = loc
        return self._offs_dev[s : s + n]

    def get(self, key) -> Optional[torch.Tensor]:
        loc = self._index.get(key)
        if loc is None:
            return None
        s, n = loc
        return self._dev[s : s + n]


class _BoundedCache(dict):
    """Insertion-ordered bound on the descriptor-table cache (round-1
    finding: a long-lived process sweeping shapes leaked device memory)."""
    LIMIT = 24

    def __setitem__(self, k, v):
        if k not in self and len(self) >= self.LIMIT:
            del self[next(iter(self))]
        super().__setitem__(k, v)


_PLAN_CACHE: Dict = _BoundedCache()


def _trsm_plan_rows(table: _DescTable, key_prefix, offs: np.ndarray, nb: int,
                    ld_l: int, bsz: int, dtype) -> None:
    """The panel solve's device-resident plan: the tile-offset list for the
    single-launch kernel where ``dtype`` has it, else the descs of the blocked
    TRSM-as-GEMM (per inner block d)."""
    if ops.has_trsm_panel_fused(dtype):
        table.add_offs((key_prefix, "trsm"), offs)
        return
    nblocks = (nb + bsz - 1) // bsz
    for d in range(nblocks):
        c0 = d * bsz
        if d > 0:
            table.add((key_prefix, "trsm_upd", d), ops.make_descs(offs + c0, offs, np.full(len(offs), c0 * ld_l)))
        table.add((key_prefix, "trsm_apply", d), ops.make_descs(offs + c0, offs + c0, np.zeros(len(offs), dtype=np.int64)))


def _run_trsm_panel(table: _DescTable, key_prefix, base: torch.Tensor,
                    L_diag: torch.Tensor, dinv: torch.Tensor, nb: int,
                    opc: Op) -> None:
    offs = table.get_offs((key_prefix, "trsm"))
    if offs is not None:
        ops.trsm_panel_fused(base, offs, L_diag, dinv, nb, nb, nb)
        return
    bsz = dinv.shape[-1]
    nblocks = (nb + bsz - 1) // bsz
    ld_l = L_diag.stride(0)
    for d in range(nblocks):
        c0 = d * bsz
        bs = min(bsz, nb - c0)
        if d > 0:
            descs = table.get((key_prefix, "trsm_upd", d))
            if descs is not None:
                ops.gemm_fused(base, base, L_diag, descs, nb, bs, c0,
                               nb, ld_l, nb, Op.NoTrans, opc, -1.0, 1.0)
        descs = table.get((key_prefix, "trsm_apply", d))
        if descs is not None:
            ops.gemm_fused(base, base, dinv[d], descs, nb, bs, bs,
                           nb, bsz, nb, Op.NoTrans, opc, 1.0, 0.0, inplace=True)


# ---------------- local ----------------

def _local_plan(mat: Matrix) -> _DescTable:
    d = mat.dist
    key = ("chol_local", d.nr_tiles, d.nb, mat.dtype, str(mat.device))
    plan = _PLAN_CACHE.get(key)
    if plan is not None:
        return plan
    nt = d.nr_tiles[0]
    nb = d.nb
    bsz = ops.potrf_bsz(mat.dtype)
    table = _DescTable()
    for k in range(nt):
        rows = np.arange(k + 1, nt)
        offs = np.array([mat.tile_offset((int(i), k)) for i in rows], dtype=np.int64)
        if len(offs):
            _trsm_plan_rows(table, ("k", k), offs, nb, nb, bsz, mat.dtype)
            # trailing split for lookahead:
            #   head = next panel column (j == k+1), factored eagerly on the
            #          high-priority stream so potrf(k+1) is not blocked;
            #   tail = the rest (j >= k+2), the bulk, on the update stream.
            def _descs_for(js_range):
                c, a, b = [], [], []
                for j in js_range:
                    for i in range(j, nt):
                        c.append(mat.tile_offset((i, j)))
                        a.append(mat.tile_offset((i, k)))
                        b.append(mat.tile_offset((j, k)))
                return ops.make_descs(np.array(c, dtype=np.int64),
                                      np.array(a, dtype=np.int64),
                                      np.array(b, dtype=np.int64)) if c else None
            h = _descs_for([k + 1])
            if h is not None:
                table.add(("k", k, "head"), h)
            t = _descs_for(range(k + 2, nt))
            if t is not None:
                table.add(("k", k, "tail"), t)
    table.upload(mat.device)
    _PLAN_CACHE[key] = table
    return table


def _cholesky_local(mat: Matrix) -> None:
    d = mat.dist
    nt = d.nr_tiles[0]
    nb = d.nb
    gpu = mat.device.type == "cuda"
    opc = _op_conj(mat.dtype)
    if gpu:
        # Lookahead schedule on two streams (see plan docstring):
        #   Sp (high prio): potrf(k) + panel TRSM(k) + head update (col k+1)
        #   Su:             tail update (cols >= k+2) — the bulk of the flops
        # P(k) waits tail(k-2); head(k) waits tail(k-1); tail(k) waits P(k).
        table = _local_plan(mat)
        dinv = ops.dinv_workspace(nb, mat.dtype, mat.device)
        st = mat.storage
        rt = get_runtime(mat.device)
        sp, su = rt.hp_streams[0], rt.np_streams[0]
        cur = torch.cuda.current_stream(mat.device)
        sp.wait_stream(cur)
        su.wait_stream(cur)
        ev_tail = [None] * nt
        for k in range(nt):
            with torch.cuda.stream(sp):
                if k >= 2 and ev_tail[k - 2] is not None:
                    sp.wait_event(ev_tail[k - 2])
                diag = mat.tile((k, k))
                ops.potrf_tile(diag, dinv)
                _run_trsm_panel(table, ("k", k), st, diag, dinv, nb, opc)
                ev_p = torch.cuda.Event()
                ev_p.record(sp)
                head = table.get(("k", k, "head"))
                if head is not None:
                    if k >= 1 and ev_tail[k - 1] is not None:
                        sp.wait_event(ev_tail[k - 1])
                    ops.gemm_fused(st, st, st, head, nb, nb, nb, nb, nb, nb,
                                   Op.NoTrans, opc, -1.0, 1.0)
            tail = table.get(("k", k, "tail"))
            if tail is not None:
                with torch.cuda.stream(su):
                    su.wait_event(ev_p)
                    ops.gemm_fused(st, st, st, tail, nb, nb, nb, nb, nb, nb,
                                   Op.NoTrans, opc, -1.0, 1.0)
                    ev = torch.cuda.Event()
                    ev.record(su)
                    ev_tail[k] = ev
        cur.wait_stream(sp)
        cur.wait_stream(su)
    else:
        for k in range(nt):
            diag = mat.tile((k, k))
            ops.potrf_tile(diag, None)
            for i in range(k + 1, nt):
                _cpu_trsm_tile(diag, mat.tile((i, k)))
            for j in range(k + 1, nt):
                for i in range(j, nt):
                    ops.gemm_tile(mat.tile((i, j)), mat.tile((i, k)), mat.tile((j, k)),
                                  Op.NoTrans, opc, -1.0, 1.0)


# ---------------- native Upper (local) ----------------

def _upper_plan(mat: Matrix) -> _DescTable:
    d = mat.dist
    key = ("chol_local_U", d.nr_tiles, d.nb, mat.dtype, str(mat.device))
    plan = _PLAN_CACHE.get(key)
    if plan is not None:
        return plan
    nt = d.nr_tiles[0]
    nb = d.nb
    bsz = ops.potrf_bsz(mat.dtype)
    nblocks = (nb + bsz - 1) // bsz
    table = _DescTable()
    for k in range(nt):
        cols = np.arange(k + 1, nt)
        offs = np.array([mat.tile_offset((k, int(j))) for j in cols],
                        dtype=np.int64)
        if len(offs):
            # row-panel left-solve per inner block d:
            #   upd: X[c0:c0+bs, :] -= Td[c0:c0+bs, :c0] @ X[:c0, :]
            #   apply: X[c0:c0+bs, :] = dinv[d] @ scratch[c0 rows]
            for dd in range(nblocks):
                c0 = dd * bsz
                if dd > 0:
                    table.add(("Uk", k, "upd", dd),
                              ops.make_descs(offs + c0 * nb,
                                             np.full(len(offs), c0 * nb), offs))
                table.add(("Uk", k, "apply", dd),
                          ops.make_descs(offs + c0 * nb,
                                         np.zeros(len(offs), dtype=np.int64),
                                         np.arange(len(offs), dtype=np.int64) * (bsz * nb)))

            def _descs_for(i_range):
                c, a, b = [], [], []
                for i in i_range:
                    for j in range(i, nt):
                        c.append(mat.tile_offset((i, j)))
                        a.append(mat.tile_offset((k, i)))
                        b.append(mat.tile_offset((k, j)))
                return ops.make_descs(np.array(c, dtype=np.int64),
                                      np.array(a, dtype=np.int64),
                                      np.array(b, dtype=np.int64)) if c else None
            h = _descs_for([k + 1])
            if h is not None:
                table.add(("Uk", k, "head"), h)
            t = _descs_for(range(k + 2, nt))
            if t is not None:
                table.add(("Uk", k, "tail"), t)
    table.upload(mat.device)
    _PLAN_CACHE[key] = table
    return table


def _cholesky_local_upper(mat: Matrix) -> None:
    """Native Upper factorization A = U^H U over upper-stored tiles (no
    storage transpose; reference ``factorization/cholesky/impl.h:317``
    call_U). The diagonal factor runs on a conj-transposed nb x nb scratch
    (O(nb^2) per step); the row panel gets a LEFT blocked solve
    U[k,j] = Lkk^{-1} A[k,j]; the trailing update is
    A[i,j] -= A[k,i]^H A[k,j] with the same two-stream lookahead as Lower.
    """
    d = mat.dist
    nt = d.nr_tiles[0]
    nb = d.nb
    gpu = mat.device.type == "cuda"
    opc = _op_conj(mat.dtype)
    st = mat.storage  # full padded tiles (identity diag pad)
    if not gpu:
        for k in range(nt):
            Td = st[k, k].mH.contiguous()
            ops.potrf_tile(Td, None)
            st[k, k].copy_(torch.tril(Td).mH)
            L = torch.tril(Td)
            for j in range(k + 1, nt):
                t = st[k, j]
                t.copy_(torch.linalg.solve_triangular(L, t, upper=False))
            for i in range(k + 1, nt):
                for j in range(i, nt):
                    ops.gemm_tile(st[i, j], st[k, i], st[k, j],
                                  opc, Op.NoTrans, -1.0, 1.0)
        return

    table = _upper_plan(mat)
    dinv = ops.dinv_workspace(nb, mat.dtype, mat.device)
    bsz = dinv.shape[-1]
    nblocks = (nb + bsz - 1) // bsz
    Td = torch.empty((nb, nb), dtype=mat.dtype, device=mat.device)
    scratch = torch.empty((nt, bsz, nb), dtype=mat.dtype, device=mat.device)
    rt = get_runtime(mat.device)
    sp, su = rt.hp_streams[0], rt.np_streams[0]
    cur = torch.cuda.current_stream(mat.device)
    sp.wait_stream(cur)
    su.wait_stream(cur)
    ev_tail = [None] * nt
    for k in range(nt):
        with torch.cuda.stream(sp):
            if k >= 2 and ev_tail[k - 2] is not None:
                sp.wait_event(ev_tail[k - 2])
            Td.copy_(st[k, k].mH)
            ops.potrf_tile(Td, dinv)
            st[k, k].copy_(torch.tril(Td).mH)
            # blocked LEFT solve of the row panel
            m_cols = nt - (k + 1)
            if m_cols > 0:
                for dd in range(nblocks):
                    c0 = dd * bsz
                    bs = min(bsz, nb - c0)
                    descs = table.get(("Uk", k, "upd", dd))
                    if descs is not None and c0 > 0:
                        ops.gemm_fused(st, Td, st, descs, bs, nb, c0,
                                       nb, nb, nb, Op.NoTrans, Op.NoTrans,
                                       -1.0, 1.0)
                    # stage the block rows, then scratch-multiply back
                    blk = st[k, k + 1:nt, c0:c0 + bs, :]
                    scratch[: m_cols, :bs].copy_(blk)
                    descs = table.get(("Uk", k, "apply", dd))
                    if descs is not None:
                        ops.gemm_fused(st, dinv[dd], scratch.view(-1), descs,
                                       bs, nb, bs, bsz, nb, nb,
                                       Op.NoTrans, Op.NoTrans, 1.0, 0.0)
            ev_p = torch.cuda.Event()
            ev_p.record(sp)
            head = table.get(("Uk", k, "head"))
            if head is not None:
                if k >= 1 and ev_tail[k - 1] is not None:
                    sp.wait_event(ev_tail[k - 1])
                ops.gemm_fused(st, st, st, head, nb, nb, nb, nb, nb, nb,
                               opc, Op.NoTrans, -1.0, 1.0)
        tail = table.get(("Uk", k, "tail"))
        if tail is not None:
            with torch.cuda.stream(su):
                su.wait_event(ev_p)
                ops.gemm_fused(st, st, st, tail, nb, nb, nb, nb, nb, nb,
                               opc, Op.NoTrans, -1.0, 1.0)
                ev = torch.cuda.Event()
                ev.record(su)
                ev_tail[k] = ev
    cur.wait_stream(sp)
    cur.wait_stream(su)


# ---------------- distributed ----------------

def _dist_plan(mat: Matrix) -> _DescTable:
    d = mat.dist
    key = ("chol_dist", d.nr_tiles, d.nb, (d.grid_rows, d.grid_cols),
           (d.rank_row, d.rank_col), mat.dtype, str(mat.device))
    plan = _PLAN_CACHE.get(key)
    if plan is not None:
        return plan
    nt = d.nr_tiles[0]
    nb = d.nb
    ts = nb * nb
    bsz = ops.potrf_bsz(mat.dtype)
    lr, lc = d.local_nr_tiles
    table = _DescTable()
    for k in range(nt):
        kr, kc = d.rank_of_tile((k, k))
        li0 = d.next_local_tile_row(k + 1)
        if d.rank_col == kc and lr - li0 > 0:
            rows_g = [d.global_tile_of_local((li, 0))[0] for li in range(li0, lr)]
            offs = np.array([mat.tile_offset((i, k)) for i in rows_g], dtype=np.int64)
            _trsm_plan_rows(table, ("k", k), offs, nb, nb, bsz, mat.dtype)
        # trailing on local tiles, split for lookahead: head = global col k+1
        # (unblocks step k+1's panel), tail = the bulk
        lj0 = d.next_local_tile_col(k + 1)
        ch, ah, bh = [], [], []
        c, a, b = [], [], []
        for lj in range(lj0, lc):
            j = d.global_tile_of_local((0, lj))[1]
            dst = (ch, ah, bh) if j == k + 1 else (c, a, b)
            for li in range(d.next_local_tile_row(j), lr):
                dst[0].append(mat.local_tile_offset(li, lj))
                dst[1].append(li * ts)
                dst[2].append(lj * ts)
        if ch:
            table.add(("k", k, "head"), ops.make_descs(np.array(ch), np.array(ah), np.array(bh)))
        if c:
            table.add(("k", k, "trail"), ops.make_descs(np.array(c), np.array(a), np.array(b)))
    table.upload(mat.device)
    _PLAN_CACHE[key] = table
    return table


def _cholesky_dist(mat: Matrix, grid: CommGrid) -> None:
    d = mat.dist
    nt = d.nr_tiles[0]
    nb = d.nb
    gpu = mat.device.type == "cuda"
    if gpu:
        _cholesky_dist_gpu(mat, grid)
        return
    opc = _op_conj(mat.dtype)

    col_panel = Panel(Panel.COL, d, mat.dtype, mat.device)  # L[i,k] by local row
    row_panel = Panel(Panel.ROW, d, mat.dtype, mat.device)  # L[j,k] by local col
    diag_ws = torch.zeros((nb, nb), dtype=mat.dtype, device=mat.device)

    for k in range(nt):
        kr, kc = d.rank_of_tile((k, k))
        on_panel_col = d.rank_col == kc
        li0 = d.next_local_tile_row(k + 1)
        lr = d.local_nr_tiles[0]

        if on_panel_col:
            if d.rank_row == kr:
                diag = mat.tile((k, k))
                ops.potrf_tile(diag, None)
            else:
                diag = diag_ws
            if grid.col_group is not None:
                coll.broadcast(diag, grid.global_rank_of_col_member(kr), grid.col_group)
            for li in range(li0, lr):
                i = d.global_tile_of_local((li, 0))[0]
                _cpu_trsm_tile(diag, mat.tile((i, k)))
                col_panel.slot(li).copy_(mat.tile((i, k)))

        # column panel: one contiguous broadcast along the row direction
        if grid.row_group is not None and lr - li0 > 0:
            coll.broadcast(
                col_panel.range_view(li0, lr),
                grid.global_rank_of_row_member(kc),
                grid.row_group,
            )

        # transposed panel: per-tile broadcasts along the column direction
        lj0 = d.next_local_tile_col(k + 1)
        lc = d.local_nr_tiles[1]
        for lj in range(lj0, lc):
            j = d.global_tile_of_local((0, lj))[1]
            jr = d.rank_of_tile_row(j)
            if d.rank_row == jr:
                lji = d.next_local_tile_row(j)
                row_panel.slot(lj).copy_(col_panel.slot(lji))
            if grid.col_group is not None:
                coll.broadcast(
                    row_panel.slot(lj), grid.global_rank_of_col_member(jr), grid.col_group
                )

        for lj in range(lj0, lc):
            j = d.global_tile_of_local((0, lj))[1]
            for li in range(d.next_local_tile_row(j), lr):
                ops.gemm_tile(
                    mat.local_tile((li, lj)), col_panel.slot(li), row_panel.slot(lj),
                    Op.NoTrans, opc, -1.0, 1.0,
                )


def _cholesky_dist_gpu(mat: Matrix, grid: CommGrid) -> None:
    """Distributed GPU Cholesky with comm/compute-overlapped lookahead.

    Two streams (the reference's priority-based lookahead,
    ``factorization/cholesky/impl.h:280-282``, recast for fused kernels):
      sp: panel path + RCCL collectives for step k — depends only on the
          HEAD update of step k-1 (column k), so it overlaps the bulk
          trailing GEMM of step k-1 running on su;
      su: head(k) (column k+1 only) then tail(k) (columns >= k+2).
    Panels are double-buffered; reuse of a buffer set waits on the tail
    event of the step that last read it.
    """
    d = mat.dist
    nt = d.nr_tiles[0]
    nb = d.nb
    opc = _op_conj(mat.dtype)
    table = _dist_plan(mat)
    panels = [
        (Panel(Panel.COL, d, mat.dtype, mat.device), Panel(Panel.ROW, d, mat.dtype, mat.device)),
        (Panel(Panel.COL, d, mat.dtype, mat.device), Panel(Panel.ROW, d, mat.dtype, mat.device)),
    ]
    diag_ws = torch.zeros((nb, nb), dtype=mat.dtype, device=mat.device)
    dinv = ops.dinv_workspace(nb, mat.dtype, mat.device)

    rt = get_runtime(mat.device)
    sp, su = rt.hp_streams[0], rt.np_streams[0]
    cur = torch.cuda.current_stream(mat.device)
    sp.wait_stream(cur)
    su.wait_stream(cur)
    ev_head = [None] * (nt + 1)
    ev_tail = [None] * (nt + 1)
    lr = d.local_nr_tiles[0]
    lc = d.local_nr_tiles[1]

    for k in range(nt):
        kr, kc = d.rank_of_tile((k, k))
        on_panel_col = d.rank_col == kc
        li0 = d.next_local_tile_row(k + 1)
        lj0 = d.next_local_tile_col(k + 1)
        col_panel, row_panel = panels[k % 2]

        with torch.cuda.stream(sp):
            if k >= 1 and ev_head[k - 1] is not None:
                sp.wait_event(ev_head[k - 1])      # column k fully updated
            if k >= 2 and ev_tail[k - 2] is not None:
                sp.wait_event(ev_tail[k - 2])      # panel buffer set reuse
            if on_panel_col:
                if d.rank_row == kr:
                    diag = mat.tile((k, k))
                    ops.potrf_tile(diag, dinv)
                else:
                    diag = diag_ws
                if grid.col_group is not None:
                    coll.broadcast(diag, grid.global_rank_of_col_member(kr), grid.col_group)
                if d.rank_row != kr:
                    _compute_dinv(diag, dinv)
                if li0 < lr:
                    _run_trsm_panel(table, ("k", k), mat.storage, diag, dinv, nb, opc)
                for li in range(li0, lr):
                    i = d.global_tile_of_local((li, 0))[0]
                    col_panel.slot(li).copy_(mat.tile((i, k)))
            if grid.row_group is not None and lr - li0 > 0:
                coll.broadcast(col_panel.range_view(li0, lr),
                               grid.global_rank_of_row_member(kc), grid.row_group)
            for lj in range(lj0, lc):
                j = d.global_tile_of_local((0, lj))[1]
                jr = d.rank_of_tile_row(j)
                if d.rank_row == jr:
                    row_panel.slot(lj).copy_(col_panel.slot(d.next_local_tile_row(j)))
                if grid.col_group is not None:
                    coll.broadcast(row_panel.slot(lj),
                                   grid.global_rank_of_col_member(jr), grid.col_group)
            ev_b = torch.cuda.Event()
            ev_b.record(sp)

        with torch.cuda.stream(su):
            su.wait_event(ev_b)
            head = table.get(("k", k, "head"))
            if head is not None:
                ops.gemm_fused(mat.storage, col_panel.storage, row_panel.storage, head,
                               nb, nb, nb, nb, nb, nb, Op.NoTrans, opc, -1.0, 1.0)
            e = torch.cuda.Event()
            e.record(su)
            ev_head[k] = e
            tail = table.get(("k", k, "trail"))
            if tail is not None:
                ops.gemm_fused(mat.storage, col_panel.storage, row_panel.storage, tail,
                               nb, nb, nb, nb, nb, nb, Op.NoTrans, opc, -1.0, 1.0)
            e2 = torch.cuda.Event()
            e2.record(su)
            ev_tail[k] = e2

    cur.wait_stream(sp)
    cur.wait_stream(su)


def cholesky_factorization(uplo: UpLo, mat: Matrix, grid: Optional[CommGrid] = None) -> None:
    """In-place Cholesky: A = L L^H (Lower) or A = U^H U (Upper).

    Upper runs through the U = L^H storage-transpose reduction (reference
    ``factorization/cholesky/impl.h:317`` implements call_U natively)."""
    from ..core.asserts import dlaf_assert
    d = mat.dist
    dlaf_assert(d.m == d.n and d.mb == d.nb,
                "square matrix with square tiles required", d.size,
                d.tile_size)
    g = grid if grid is not None else mat.grid
    if uplo == UpLo.Upper:
        if g is None or not g.distributed:
            _cholesky_local_upper(mat)   # native call_U (no transposes)
            return
        # distributed Upper: storage-transpose reduction (the reference's
        # call_U is native there too — future work)
        from ._uplo import transpose_storage
        transpose_storage(mat)
        cholesky_factorization(UpLo.Lower, mat, grid)
        transpose_storage(mat)
        return
    if g is None or not g.distributed:
        _cholesky_local(mat)
    else:
        _cholesky_dist(mat, g)
