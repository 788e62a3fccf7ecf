"""Norms of a distributed matrix.

``max_norm`` is the per-tile max-abs loop described below. ``matrix_norm``
computes the max, one, infinity and Frobenius norms of a general, Hermitian
or triangular matrix from ONE pass over the local tile storage: the HIP kernel
of ``csrc/norms.hip`` on the device, ``_partials_host`` (the host twin, the
same masking rules in torch) on the CPU. Both give, per rank, the absolute
sums per local row and column, max |a| and Blue's three sum-of-squares
accumulators; ``matrix_norm`` scatters the sums to global indices, all-reduces
them over the full grid and finishes the requested norm on the host.

Max-norm of a distributed matrix (``max_norm``).

Counterpart of ``auxiliary/norm/mc.h:1-163`` (per-tile lange/lantr max-abs +
MAX reduce to rank {0,0}); here the result is all-reduced so every rank
returns the same scalar (the reference's callers broadcast it anyway).
``uplo=Lower`` restricts to the lower triangle + diagonal (Hermitian
matrices); padding is excluded by using logical tile views.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from ..types import UpLo, Diag
from ..core.asserts import dlaf_assert
from ..ops._ext import get_ext
from ..matrix.matrix import Matrix
from ..comm.grid import CommGrid
from ..comm import collectives as coll


def max_norm(mat: Matrix, uplo: UpLo = None, grid: Optional[CommGrid] = None) -> float:
    """Largest absolute element of the (triangle of the) distributed matrix."""
    d = mat.dist
    g = grid if grid is not None else mat.grid
    best = torch.zeros((), dtype=torch.float64, device=mat.device)
    for li, lj in d.iter_local_tiles():
        gi, gj = d.global_tile_of_local((li, lj))
        t = mat.tile_logical((gi, gj))
        if uplo == UpLo.Lower:
            if gi < gj:
                continue
            if gi == gj:
                t = torch.tril(t)
        elif uplo == UpLo.Upper:
            if gi > gj:
                continue
            if gi == gj:
                t = torch.triu(t)
        if t.numel():
            m = t.abs().max().to(torch.float64)
            best = torch.maximum(best, m)
    if g is not None and g.distributed:
        coll.all_reduce_max(best, g.full_group)
    return float(best.item())


# ---- one-pass norms --------------------------------------------------------

_NORMS = ("max", "one", "inf", "fro")
_STRUCTURES = {"general": 0, "hermitian": 1, "triangular": 2}

# Blue's thresholds and scalings for double (LAPACK 3.10 la_constants); the
# kernel uses the same numbers
_TSML, _TBIG = 2.0 ** -511, 2.0 ** 486
_SSML, _SBIG = 2.0 ** 537, 2.0 ** -538


def _tile_geometry(d) -> Tuple[int, int, int, int]:
    """(gr0, grs, gc0, gcs): local tile l is global tile g0 + l * gs."""
    return (d.global_tile_of_local((0, 0))[0], d.grid_rows,
            d.global_tile_of_local((0, 0))[1], d.grid_cols)


def _partials_host(storage: torch.Tensor, m: int, n: int, gr0: int, grs: int,
                   gc0: int, gcs: int, structure: int, upper: bool,
                   unit_diag: bool):
    """Host twin of ``matrix_norms``: (rows, cols, scal) in float64.

    Written for clarity, not for size: it holds about ten float64 temporaries
    of the storage's shape (masks, moduli, the ``where`` results), so a large
    CPU matrix needs that much memory."""
    tr, tc, mb, nb = storage.shape
    dev = storage.device
    gr = ((gr0 + torch.arange(tr, device=dev) * grs)[:, None] * mb
          + torch.arange(mb, device=dev)[None, :])[:, None, :, None]
    gc = ((gc0 + torch.arange(tc, device=dev) * gcs)[:, None] * nb
          + torch.arange(nb, device=dev)[None, :])[None, :, None, :]
    mask = (gr < m) & (gc < n)
    if structure != 0:
        mask = mask & ((gc >= gr) if upper else (gc <= gr))
    diag = mask & (gr == gc)
    cplx = storage.is_complex()
    single = storage.dtype in (torch.float32, torch.complex64)
    if cplx:
        parts = [storage.real.abs().to(torch.float64),
                 storage.imag.abs().to(torch.float64)]
        # complex64 squares are safe in float64; complex128 needs hypot
        av = (torch.sqrt(parts[0] ** 2 + parts[1] ** 2) if single
              else torch.hypot(parts[0], parts[1]))
    else:
        parts = [storage.abs().to(torch.float64)]
        av = parts[0]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    one = torch.ones((), dtype=torch.float64, device=dev)
    if structure == 1:
        # |Re a_ii| on the diagonal, imaginary part ignored
        av = torch.where(diag, parts[0], av)
        if cplx:
            parts[1] = torch.where(diag, zero, parts[1])
    if structure == 2 and unit_diag:
        av = torch.where(diag, one, av)
        parts[0] = torch.where(diag, one, parts[0])
        if cplx:
            parts[1] = torch.where(diag, zero, parts[1])
    av = torch.where(mask, av, zero)
    cols = av.sum(dim=(0, 2)).reshape(-1)
    rowv = torch.where(diag, zero, av) if structure == 1 else av
    rows = rowv.sum(dim=(1, 3)).reshape(-1)
    vmax = av.max()  # torch's max propagates NaN
    # off-diagonal elements of a Hermitian matrix stand for two
    wgt = torch.where(diag, one, 2 * one) if structure == 1 else one
    sml, med, big = zero, zero, zero
    for p in parts:
        p = torch.where(mask, p, zero)
        if single:
            med = med + (wgt * p * p).sum()
            continue
        isbig, issml = p > _TBIG, p < _TSML
        big = big + (wgt * torch.where(isbig, p * _SBIG, zero) ** 2).sum()
        sml = sml + (wgt * torch.where(issml, p * _SSML, zero) ** 2).sum()
        med = med + (wgt * torch.where(isbig | issml, zero, p) ** 2).sum()
    return rows, cols, torch.stack([vmax, sml, med, big])


def _local_partials(mat: Matrix, structure: int, upper: bool, unit_diag: bool):
    d = mat.dist
    lr, lc = d.local_nr_tiles
    dev = mat.device
    if lr == 0 or lc == 0:
        z = torch.zeros
        return (z(lr * d.mb, dtype=torch.float64, device=dev),
                z(lc * d.nb, dtype=torch.float64, device=dev),
                z(4, dtype=torch.float64, device=dev))
    gr0, grs, gc0, gcs = _tile_geometry(d)
    st = mat.storage
    if st.is_cuda:
        # a missing kernel is an error: get_ext() raises
        return get_ext().matrix_norms(st.contiguous(), d.m, d.n, gr0, grs,
                                      gc0, gcs, structure, int(upper),
                                      unit_diag)
    return _partials_host(st, d.m, d.n, gr0, grs, gc0, gcs, structure, upper,
                          unit_diag)


def _global_index(ntiles_local: int, tile: int, g0: int, gs: int, size: int,
                  device) -> torch.Tensor:
    """Global element index of every local row (column); >= size on padding."""
    t = g0 + torch.arange(ntiles_local, device=device) * gs
    return (t[:, None] * tile
            + torch.arange(tile, device=device)[None, :]).reshape(-1)


def _blue_finish(sml: float, med: float, big: float) -> float:
    """sqrt of the sum of squares held in Blue's accumulators (as dnrm2)."""
    nan_med = med != med
    if big > 0:
        if med > 0 or nan_med:
            big += (med * _SBIG) * _SBIG
        return math.sqrt(big) / _SBIG
    if sml > 0:
        if med > 0 or nan_med:
            if nan_med:
                return float("nan")
            ymed, ysml = math.sqrt(med), math.sqrt(sml) / _SSML
            ymin, ymax = min(ymed, ysml), max(ymed, ysml)
            return ymax * math.sqrt(1.0 + (ymin / ymax) ** 2)
        return math.sqrt(sml) / _SSML
    return math.sqrt(med) if med == med else float("nan")


def matrix_norm(norm: str, mat: Matrix, *, uplo: Optional[UpLo] = None,
                structure: str = "general", diag: Diag = Diag.NonUnit,
                grid: Optional[CommGrid] = None) -> float:
    """Norm of the distributed matrix; the same float on every rank.

    ``norm``: ``"max"`` (largest |a_ij|), ``"one"`` (largest column sum),
    ``"inf"`` (largest row sum) or ``"fro"``. ``structure``:
    ``"general"``; ``"hermitian"`` (only the ``uplo`` triangle is read, an
    off-diagonal element stands for its mirror image too, the diagonal counts
    as ``|Re a_ii|``); ``"triangular"`` (the other triangle is ignored;
    ``Diag.Unit`` counts the diagonal as 1 whatever is stored). The identity
    padding of partial edge tiles is never part of the matrix. NaN
    propagates; an empty matrix has norm 0.
    """
    dlaf_assert(norm in _NORMS, "norm must be one of", _NORMS, norm)
    dlaf_assert(structure in _STRUCTURES, "structure must be one of",
                tuple(_STRUCTURES), structure)
    code = _STRUCTURES[structure]
    dlaf_assert(code == 0 or uplo in (UpLo.Lower, UpLo.Upper),
                "uplo is required for hermitian and triangular matrices")
    d = mat.dist
    dlaf_assert(code != 1 or d.m == d.n, "hermitian matrix must be square",
                d.size)
    if d.m == 0 or d.n == 0:
        return 0.0
    g = grid if grid is not None else mat.grid
    rows, cols, scal = _local_partials(mat, code, uplo == UpLo.Upper,
                                       diag == Diag.Unit)
    if g is not None and g.distributed:
        # scatter the local sums to global indices and add over all ranks;
        # the accumulators ride along. MAX travels separately, and a NaN it
        # may drop is restored from the (NaN-carrying) sums.
        lr, lc = d.local_nr_tiles
        gr0, grs, gc0, gcs = _tile_geometry(d)
        buf = torch.zeros(d.m + d.n + 3, dtype=torch.float64,
                          device=mat.device)
        gi = _global_index(lr, d.mb, gr0, grs, d.m, mat.device)
        buf[gi[gi < d.m]] = rows[gi < d.m]
        gj = _global_index(lc, d.nb, gc0, gcs, d.n, mat.device)
        buf[d.m + gj[gj < d.n]] = cols[gj < d.n]
        buf[d.m + d.n:] = scal[1:]
        vmax = scal[:1].clone()
        coll.all_reduce_sum(buf, g.full_group)
        coll.all_reduce_max(vmax, g.full_group)
        rows, cols = buf[: d.m], buf[d.m: d.m + d.n]
        scal = torch.cat([vmax, buf[d.m + d.n:]])
    if code == 1:
        # stored column sum + strict stored row sum = full column sum
        rows = cols = rows[: d.n] + cols[: d.n]
    out = torch.cat([scal, cols.max()[None], rows.max()[None]]).tolist()
    vmax, sml, med, big, cmax, rmax = out
    if sml != sml or med != med or big != big:
        vmax = float("nan")
    if norm == "max":
        return vmax
    if norm == "one":
        return cmax
    if norm == "inf":
        return rmax
    return _blue_finish(sml, med, big)
