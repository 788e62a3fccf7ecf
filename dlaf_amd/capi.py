"""ScaLAPACK-style drop-in API over local block-cyclic buffers.

Counterpart of the reference's C API (``include/dlaf_c/*``, ``src/c_api/*``):
grid management by integer context, ScaLAPACK-style descriptors, and
``p?potrf / p?potri / p?trtri / p?syevd / p?heevd / p?sygvd / p?hegvd``
entry points, the norms ``p?lange / p?lansy / p?lanhe / p?lantr``, the
condition estimates ``p?pocon / p?trcon``, the solve ``p?potrs``, its
refinement ``p?porfs`` and the mixed-precision solves ``pdsposv / pzcposv``, and
the general-matrix ``p?getrf / p?getrs / p?gesv / p?gecon`` (single-rank
contexts), all operating on the caller's LOCAL block-cyclic column-major buffer (numpy or
torch). Each call wraps the buffer into a tiled ``Matrix``
(mirrored to the GPU when available), runs the native algorithm, and copies
the result back — the flow of the reference's ``src/c_api/eigensolver/
eigensolver.h:30-73`` (host matrix -> MatrixMirror -> algorithm -> copy back).

Python is this framework's C-API surface (the package is the library); the
function names and argument conventions mirror the reference's so ScaLAPACK
callers can map 1:1.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from .types import UpLo, Diag, Op
from .core.asserts import dlaf_assert
from .core.distribution import Distribution
from .comm.grid import CommGrid
from .matrix.matrix import Matrix
from .algs.cholesky import cholesky_factorization
from .algs.inverse import inverse_from_cholesky_factor, triangular_inverse
from .algs.eigensolver import hermitian_eigensolver, hermitian_generalized_eigensolver
from .algs.tridiag_bisect import (hermitian_eigenvalues,
                                  hermitian_generalized_eigenvalues)
from .algs.norm import matrix_norm
from .algs.condition import cholesky_rcond, triangular_rcond, cholesky_solve
from .algs.refine import cholesky_info, cholesky_refine, cholesky_solve_mixed
from .algs.lu import lu_factorization, lu_solve, lu_rcond


@dataclass
class DLAF_descriptor:
    """ScaLAPACK-like descriptor (reference ``include/dlaf_c/desc.h``)."""
    m: int
    n: int
    mb: int
    nb: int
    isrc: int = 0
    jsrc: int = 0
    i: int = 1
    j: int = 1
    ld: int = 0


_grids: Dict[int, CommGrid] = {}
_next_ctx = [1]


def dlaf_create_grid(nprow: int, npcol: int, order: str = "R",
                     device: Optional[torch.device] = None) -> int:
    """Create a process grid context (reference ``dlaf_c/grid.h``).

    Row-major rank order only (the reference supports both; RCCL ranks here
    are torch.distributed ranks, which this framework orders row-major).

    Multi-process grids (nprow*npcol > 1): if torch.distributed is not yet
    initialized, it is initialized here from the torchrun/launcher
    environment (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT) — RCCL when
    a GPU is visible, gloo otherwise. This is the C-ABI entry path for
    multi-rank callers (reference: ``src/c_api/grid.cpp`` builds the
    CommunicatorGrid from the caller's MPI_Comm; here the rendezvous is the
    launcher environment instead of MPI).
    """
    assert order.upper().startswith("R"), "row-major rank ordering only"
    import torch.distributed as tdist
    if (nprow * npcol > 1 and tdist.is_available()
            and not tdist.is_initialized()):
        import os
        assert "RANK" in os.environ and "WORLD_SIZE" in os.environ, (
            "multi-process grid: launch with torchrun-style env "
            "(RANK/WORLD_SIZE/MASTER_ADDR/MASTER_PORT)")
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        tdist.init_process_group(backend=backend)
    grid = CommGrid(nprow, npcol, device=device)
    ctx = _next_ctx[0]
    _next_ctx[0] += 1
    _grids[ctx] = grid
    return ctx


def dlaf_local_shape(ctx: int, desc: "DLAF_descriptor"):
    """Rank-local (rows, cols) of the block-cyclic buffer described by
    ``desc`` on grid ``ctx`` — used by the C ABI (csrc/capi/dlaf_c.cpp) to
    wrap the caller's LOCAL panel with the right shape on >1x1 grids."""
    g = _grid(ctx)
    d = Distribution(desc.m, desc.n, desc.mb, desc.nb,
                     g.grid_rows, g.grid_cols, g.rank_row, g.rank_col,
                     desc.isrc, desc.jsrc)
    lm, ln = d.local_size
    return int(lm), int(ln)


def dlaf_free_grid(ctx: int) -> None:
    _grids.pop(ctx, None)


def _grid(ctx: int) -> CommGrid:
    return _grids[ctx]


def _device_for(grid: CommGrid):
    if torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


def _wrap_local(a_local, desc: DLAF_descriptor, grid: CommGrid, device) -> Matrix:
    """Tiled device Matrix from the caller's local block-cyclic buffer."""
    t = torch.as_tensor(a_local)
    assert desc.i == 1 and desc.j == 1, "sub-matrix offsets not supported"
    dist = Distribution(desc.m, desc.n, desc.mb, desc.nb,
                        grid.grid_rows, grid.grid_cols, grid.rank_row, grid.rank_col,
                        desc.isrc, desc.jsrc)
    mat = Matrix(dist, t.dtype, device, grid if grid.distributed else None)
    lr, lc = dist.local_nr_tiles
    for li in range(lr):
        for lj in range(lc):
            gi, gj = dist.global_tile_of_local((li, lj))
            tsr, tsc = dist.tile_size_of((gi, gj))
            blk = t[li * desc.mb: li * desc.mb + tsr, lj * desc.nb: lj * desc.nb + tsc]
            mat.storage[li, lj, :tsr, :tsc] = blk.to(device)
    mat._set_identity_pad()
    return mat


def _unwrap_local(mat: Matrix, a_local) -> None:
    t = torch.as_tensor(a_local)
    dist = mat.dist
    lr, lc = dist.local_nr_tiles
    for li in range(lr):
        for lj in range(lc):
            gi, gj = dist.global_tile_of_local((li, lj))
            tsr, tsc = dist.tile_size_of((gi, gj))
            blk = mat.storage[li, lj, :tsr, :tsc].to(t.device if t.is_cuda else "cpu")
            t[li * dist.mb: li * dist.mb + tsr, lj * dist.nb: lj * dist.nb + tsc] = blk
    if isinstance(a_local, np.ndarray):
        a_local[:] = t.numpy()


def _potrf_info(mat: Matrix, grid=None) -> int:
    """info > 0 when the input was not positive definite: the failed-pivot
    scan of ``algs.refine.cholesky_info``, the same on every rank."""
    return cholesky_info(mat, grid)


def dlaf_cholesky_factorization(ctx: int, uplo: str, a_local, desc: DLAF_descriptor) -> int:
    """``dlaf_cholesky_factorization_{s,d,c,z}`` analog; returns info (0 = ok,
    > 0 = leading minor of that order not positive definite)."""
    ul = UpLo.Upper if uplo.upper() == "U" else UpLo.Lower
    grid = _grid(ctx)
    dev = _device_for(grid)
    mat = _wrap_local(a_local, desc, grid, dev)
    cholesky_factorization(ul, mat, grid if grid.distributed else None)
    info = _potrf_info(mat, grid)
    _unwrap_local(mat, a_local)
    return info


def dlaf_inverse_from_cholesky_factor(ctx: int, uplo: str, a_local,
                                      desc: DLAF_descriptor) -> int:
    ul = UpLo.Upper if uplo.upper() == "U" else UpLo.Lower
    grid = _grid(ctx)
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    inverse_from_cholesky_factor(ul, mat, grid if grid.distributed else None)
    _unwrap_local(mat, a_local)
    return 0


def dlaf_triangular_inverse(ctx: int, uplo: str, diag: str, a_local,
                            desc: DLAF_descriptor) -> int:
    ul = UpLo.Upper if uplo.upper() == "U" else UpLo.Lower
    grid = _grid(ctx)
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    triangular_inverse(ul, Diag.Unit if diag.upper() == "U" else Diag.NonUnit,
                       mat, grid if grid.distributed else None)
    _unwrap_local(mat, a_local)
    return 0


def dlaf_hermitian_eigensolver(ctx: int, uplo: str, a_local, desc: DLAF_descriptor,
                               w_out, z_local, descz: DLAF_descriptor,
                               il: int = 0, iu: Optional[int] = None) -> int:
    """``dlaf_{symmetric,hermitian}_eigensolver[_partial_spectrum]`` analog.

    w_out: [n] real output buffer; z_local: local eigenvector buffer.
    """
    grid = _grid(ctx)
    dev = _device_for(grid)
    mat = _wrap_local(a_local, desc, grid, dev)
    if uplo.upper() == "U":
        # A is Hermitian: conj-transposing the storage turns the given upper
        # triangle into the lower triangle the pipeline reads.
        from .algs._uplo import transpose_storage
        transpose_storage(mat)
    w, evecs = hermitian_eigensolver(UpLo.Lower, mat, grid if grid.distributed else None,
                                     eigenvalues_index_begin=il,
                                     eigenvalues_index_end=iu)
    wt = torch.as_tensor(w_out)
    wt[: w.shape[0]] = w.cpu().to(wt.dtype)
    if isinstance(w_out, np.ndarray):
        w_out[: w.shape[0]] = wt[: w.shape[0]].numpy()
    _unwrap_local(evecs, z_local)
    _unwrap_local(mat, a_local)
    return 0


def dlaf_hermitian_generalized_eigensolver(ctx: int, uplo: str, a_local,
                                           desca: DLAF_descriptor, b_local,
                                           descb: DLAF_descriptor, w_out,
                                           z_local, descz: DLAF_descriptor,
                                           factorized: bool = False) -> int:
    grid = _grid(ctx)
    dev = _device_for(grid)
    mat_a = _wrap_local(a_local, desca, grid, dev)
    mat_b = _wrap_local(b_local, descb, grid, dev)
    if uplo.upper() == "U":
        from .algs._uplo import transpose_storage
        transpose_storage(mat_a)
        transpose_storage(mat_b)
    w, evecs = hermitian_generalized_eigensolver(
        UpLo.Lower, mat_a, mat_b, grid if grid.distributed else None,
        factorized=factorized)
    wt = torch.as_tensor(w_out)
    wt[: w.shape[0]] = w.cpu().to(wt.dtype)
    if isinstance(w_out, np.ndarray):
        w_out[: w.shape[0]] = wt[: w.shape[0]].numpy()
    _unwrap_local(evecs, z_local)
    _unwrap_local(mat_b, b_local)
    return 0


def _store_w(w: torch.Tensor, w_out) -> None:
    wt = torch.as_tensor(w_out)
    wt[: w.shape[0]] = w.cpu().to(wt.dtype)
    if isinstance(w_out, np.ndarray):
        w_out[: w.shape[0]] = wt[: w.shape[0]].numpy()


def dlaf_hermitian_eigenvalues(ctx: int, uplo: str, a_local,
                               desc: DLAF_descriptor, w_out, il: int = 0,
                               iu: Optional[int] = None) -> int:
    """Eigenvalues only (``jobz='N'``) of the Hermitian matrix in ``a_local``.

    w_out: [n] real output buffer; eigenvalues ``il <= k < iu`` (0-based,
    ascending) land in ``w_out[:iu-il]``. ``a_local`` is overwritten as by
    ``dlaf_hermitian_eigensolver``.
    """
    grid = _grid(ctx)
    dev = _device_for(grid)
    mat = _wrap_local(a_local, desc, grid, dev)
    if uplo.upper() == "U":
        from .algs._uplo import transpose_storage
        transpose_storage(mat)
    w = hermitian_eigenvalues(UpLo.Lower, mat,
                              grid if grid.distributed else None,
                              eigenvalues_index_begin=il,
                              eigenvalues_index_end=iu)
    _store_w(w, w_out)
    _unwrap_local(mat, a_local)
    return 0


def dlaf_hermitian_generalized_eigenvalues(ctx: int, uplo: str, a_local,
                                           desca: DLAF_descriptor, b_local,
                                           descb: DLAF_descriptor, w_out,
                                           factorized: bool = False) -> int:
    """Eigenvalues only of A x = lambda B x; ``b_local`` is overwritten with
    its Cholesky factor as by ``dlaf_hermitian_generalized_eigensolver``."""
    grid = _grid(ctx)
    dev = _device_for(grid)
    mat_a = _wrap_local(a_local, desca, grid, dev)
    mat_b = _wrap_local(b_local, descb, grid, dev)
    if uplo.upper() == "U":
        from .algs._uplo import transpose_storage
        transpose_storage(mat_a)
        transpose_storage(mat_b)
    w = hermitian_generalized_eigenvalues(
        UpLo.Lower, mat_a, mat_b, grid if grid.distributed else None,
        factorized=factorized)
    _store_w(w, w_out)
    _unwrap_local(mat_b, b_local)
    return 0


# LAPACK norm characters -> matrix_norm names
_NORM_CHAR = {"M": "max", "1": "one", "O": "one", "I": "inf", "F": "fro",
              "E": "fro"}
_STRUCT_CHAR = {"G": "general", "H": "hermitian", "S": "hermitian",
                "T": "triangular"}


def dlaf_matrix_norm(ctx: int, norm: str, structure: str, uplo: Optional[str],
                     diag: str, a_local, desc: DLAF_descriptor) -> float:
    """Norm of the matrix in ``a_local`` (which is only read).

    norm: 'M', '1' / 'O', 'I', 'F' / 'E' (LAPACK) or a ``matrix_norm`` name;
    structure: 'G'eneral, 'H'ermitian / 'S'ymmetric (real), 'T'riangular or a
    ``matrix_norm`` name; uplo 'L' / 'U' (ignored for general); diag 'N' /
    'U' (triangular only). Every rank of the grid gets the same value.
    """
    grid = _grid(ctx)
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    name = _NORM_CHAR.get(str(norm).upper(), norm)
    struct = _STRUCT_CHAR.get(str(structure).upper(), structure)
    ul = None
    if struct != "general":
        ul = UpLo.Upper if str(uplo).upper() == "U" else UpLo.Lower
    return matrix_norm(name, mat, uplo=ul, structure=struct,
                       diag=Diag.Unit if str(diag).upper() == "U"
                       else Diag.NonUnit,
                       grid=grid if grid.distributed else None)


def _uplo(uplo: str) -> UpLo:
    return UpLo.Upper if str(uplo).upper() == "U" else UpLo.Lower


def dlaf_cholesky_rcond(ctx: int, uplo: str, a_local, desc: DLAF_descriptor,
                        anorm: float) -> float:
    """Estimated reciprocal one-norm condition number of the Hermitian
    positive definite matrix whose Cholesky factor (as left by
    ``dlaf_cholesky_factorization``) is in the ``uplo`` triangle of
    ``a_local``, which is only read. ``anorm`` is the one-norm of the matrix
    before factorization (``dlaf_matrix_norm(ctx, '1', 'H', uplo, ...)``).
    Every rank of the grid gets the same value."""
    grid = _grid(ctx)
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    return cholesky_rcond(_uplo(uplo), mat, float(anorm),
                          grid if grid.distributed else None)


def dlaf_triangular_rcond(ctx: int, norm: str, uplo: str, diag: str, a_local,
                          desc: DLAF_descriptor) -> float:
    """Estimated reciprocal condition number of the triangular matrix in the
    ``uplo`` triangle of ``a_local`` (only read). norm: '1' / 'O' or 'I'
    (LAPACK) or ``"one"`` / ``"inf"``; diag 'N' / 'U'."""
    grid = _grid(ctx)
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    name = _NORM_CHAR.get(str(norm).upper(), norm)
    return triangular_rcond(name, _uplo(uplo),
                            Diag.Unit if str(diag).upper() == "U"
                            else Diag.NonUnit, mat,
                            grid if grid.distributed else None)


def dlaf_cholesky_solve(ctx: int, uplo: str, a_local, desca: DLAF_descriptor,
                        b_local, descb: DLAF_descriptor) -> int:
    """Solve A X = B with the Cholesky factor of A in the ``uplo`` triangle of
    ``a_local`` (only read); ``b_local`` is overwritten with X."""
    grid = _grid(ctx)
    dev = _device_for(grid)
    fac = _wrap_local(a_local, desca, grid, dev)
    rhs = _wrap_local(b_local, descb, grid, dev)
    cholesky_solve(_uplo(uplo), fac, rhs, grid if grid.distributed else None)
    _unwrap_local(rhs, b_local)
    return 0


def dlaf_cholesky_refine(ctx: int, uplo: str, a_local, desca: DLAF_descriptor,
                         af_local, descaf: DLAF_descriptor, b_local,
                         descb: DLAF_descriptor, x_local,
                         descx: DLAF_descriptor, ferr_out, berr_out) -> int:
    """Refine the solution in ``x_local`` of A X = B and store the forward
    error bounds and backward errors (``cholesky_refine``) in ``ferr_out`` /
    ``berr_out`` ([nrhs] real buffers). ``a_local`` holds A, ``af_local`` its
    Cholesky factor, ``b_local`` B; the three are only read."""
    grid = _grid(ctx)
    dev = _device_for(grid)
    g = grid if grid.distributed else None
    mat = _wrap_local(a_local, desca, grid, dev)
    fac = _wrap_local(af_local, descaf, grid, dev)
    rhs = _wrap_local(b_local, descb, grid, dev)
    sol = _wrap_local(x_local, descx, grid, dev)
    ferr, berr = cholesky_refine(_uplo(uplo), mat, fac, rhs, sol, g)
    _store_w(ferr, ferr_out)
    _store_w(berr, berr_out)
    _unwrap_local(sol, x_local)
    return 0


def dlaf_cholesky_solve_mixed(ctx: int, uplo: str, a_local,
                              desca: DLAF_descriptor, b_local,
                              descb: DLAF_descriptor, x_local,
                              descx: DLAF_descriptor):
    """Solve A X = B (float64 / complex128) with a single precision
    factorization and double precision refinement (``cholesky_solve_mixed``);
    ``x_local`` receives X. Returns ``(iters, info)``. ``a_local`` and
    ``b_local`` are only read: the factor is not left in ``a_local``."""
    grid = _grid(ctx)
    dev = _device_for(grid)
    mat = _wrap_local(a_local, desca, grid, dev)
    rhs = _wrap_local(b_local, descb, grid, dev)
    sol, iters, info = cholesky_solve_mixed(
        _uplo(uplo), mat, rhs, grid if grid.distributed else None)
    if sol is not None:
        _unwrap_local(sol, x_local)
    return iters, info


# ---- LU with partial pivoting (single-rank contexts) ----

_TRANS_CHAR = {"N": Op.NoTrans, "T": Op.Trans, "C": Op.ConjTrans}


def _single_rank(grid: CommGrid, what: str) -> None:
    dlaf_assert(not grid.distributed,
                f"{what}: LU is not implemented on a multi-rank "
                "(distributed) grid; use a 1 x 1 context",
                (grid.grid_rows, grid.grid_cols))


def _ipiv_in(ipiv, n: int, device) -> torch.Tensor:
    """The caller's 1-based pivots as the library's 0-based int32 vector."""
    t = torch.as_tensor(ipiv).reshape(-1)[:n]
    return (t.to(torch.int64) - 1).to(device=device, dtype=torch.int32)


def dlaf_lu_factorization(ctx: int, a_local, desc: DLAF_descriptor,
                          ipiv_out) -> int:
    """``P A = L U`` in place on ``a_local`` (``lu_factorization``).
    ``ipiv_out`` ([n] int32 buffer) receives the 1-based global row indices
    of LAPACK / ScaLAPACK: row j was interchanged with row ``ipiv[j - 1]``.
    Returns info: 0, or the 1-based index of the first zero pivot."""
    grid = _grid(ctx)
    _single_rank(grid, "dlaf_lu_factorization")
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    ipiv, info = lu_factorization(mat)
    out = torch.as_tensor(ipiv_out)
    out.reshape(-1)[: desc.n] = (ipiv + 1).to(device=out.device,
                                               dtype=out.dtype)
    _unwrap_local(mat, a_local)
    return info


def dlaf_lu_solve(ctx: int, trans: str, a_local, desca: DLAF_descriptor,
                  ipiv, b_local, descb: DLAF_descriptor) -> int:
    """Solve op(A) X = B with the factors and 1-based pivots of
    ``dlaf_lu_factorization`` (both only read); trans 'N' / 'T' / 'C';
    ``b_local`` is overwritten with X."""
    grid = _grid(ctx)
    _single_rank(grid, "dlaf_lu_solve")
    dev = _device_for(grid)
    fac = _wrap_local(a_local, desca, grid, dev)
    rhs = _wrap_local(b_local, descb, grid, dev)
    lu_solve(_TRANS_CHAR[str(trans).upper()], fac,
             _ipiv_in(ipiv, desca.n, dev), rhs)
    _unwrap_local(rhs, b_local)
    return 0


def dlaf_lu_rcond(ctx: int, norm: str, a_local, desc: DLAF_descriptor,
                  anorm: float) -> float:
    """Estimated reciprocal condition number ('1' / 'O' or 'I') of the matrix
    whose LU factors are in ``a_local`` (only read); ``anorm`` is that norm
    of the matrix before it was factored."""
    grid = _grid(ctx)
    _single_rank(grid, "dlaf_lu_rcond")
    mat = _wrap_local(a_local, desc, grid, _device_for(grid))
    return lu_rcond(_NORM_CHAR.get(str(norm).upper(), norm), mat,
                    float(anorm))


# ---- ScaLAPACK-style shims (reference dlaf_c/...: dlaf_p{s,d,c,z}potrf etc.) ----

def _sl_desc(n, mb, nb, uplo_n=None, m=None) -> DLAF_descriptor:
    return DLAF_descriptor(m if m is not None else n, n, mb, nb)


def pXpotrf(ctx: int, uplo: str, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor) -> int:
    assert (ia, ja) == (1, 1)
    return dlaf_cholesky_factorization(ctx, uplo, a_local, desca)


def pXpotri(ctx: int, uplo: str, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor) -> int:
    assert (ia, ja) == (1, 1)
    return dlaf_inverse_from_cholesky_factor(ctx, uplo, a_local, desca)


def pXtrtri(ctx: int, uplo: str, diag: str, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor) -> int:
    assert (ia, ja) == (1, 1)
    return dlaf_triangular_inverse(ctx, uplo, diag, a_local, desca)


def pXsyevd(ctx: int, uplo: str, n: int, a_local, desca: DLAF_descriptor,
            w_out, z_local, descz: DLAF_descriptor) -> int:
    return dlaf_hermitian_eigensolver(ctx, uplo, a_local, desca, w_out, z_local, descz)


def pXsygvd(ctx: int, uplo: str, n: int, a_local, desca, b_local, descb,
            w_out, z_local, descz) -> int:
    return dlaf_hermitian_generalized_eigensolver(ctx, uplo, a_local, desca,
                                                  b_local, descb, w_out, z_local, descz)


def _norm_desc(desca: DLAF_descriptor, m: int, n: int) -> DLAF_descriptor:
    """desca restricted to its leading m x n part (ia = ja = 1)."""
    assert 0 <= m <= desca.m and 0 <= n <= desca.n, (m, n, desca)
    return DLAF_descriptor(m, n, desca.mb, desca.nb, desca.isrc, desca.jsrc,
                           1, 1, desca.ld)


def pXlange(ctx: int, norm: str, m: int, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor) -> float:
    assert (ia, ja) == (1, 1)
    return dlaf_matrix_norm(ctx, norm, "G", None, "N", a_local,
                            _norm_desc(desca, m, n))


def pXlanhe(ctx: int, norm: str, uplo: str, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor) -> float:
    assert (ia, ja) == (1, 1)
    return dlaf_matrix_norm(ctx, norm, "H", uplo, "N", a_local,
                            _norm_desc(desca, n, n))


pXlansy = pXlanhe  # real symmetric; complex-symmetric zlansy is not provided


def pXlantr(ctx: int, norm: str, uplo: str, diag: str, m: int, n: int, a_local,
            ia: int, ja: int, desca: DLAF_descriptor) -> float:
    assert (ia, ja) == (1, 1)
    return dlaf_matrix_norm(ctx, norm, "T", uplo, diag, a_local,
                            _norm_desc(desca, m, n))


def pXpocon(ctx: int, uplo: str, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor, anorm: float) -> float:
    """rcond of p?pocon (its workspace arguments have no counterpart)."""
    assert (ia, ja) == (1, 1)
    return dlaf_cholesky_rcond(ctx, uplo, a_local, _norm_desc(desca, n, n),
                               anorm)


def pXtrcon(ctx: int, norm: str, uplo: str, diag: str, n: int, a_local,
            ia: int, ja: int, desca: DLAF_descriptor) -> float:
    """rcond of p?trcon."""
    assert (ia, ja) == (1, 1)
    return dlaf_triangular_rcond(ctx, norm, uplo, diag, a_local,
                                 _norm_desc(desca, n, n))


def pXpotrs(ctx: int, uplo: str, n: int, nrhs: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor, b_local, ib: int, jb: int,
            descb: DLAF_descriptor) -> int:
    assert (ia, ja) == (1, 1) and (ib, jb) == (1, 1)
    return dlaf_cholesky_solve(ctx, uplo, a_local, _norm_desc(desca, n, n),
                               b_local, _norm_desc(descb, n, nrhs))


def pXporfs(ctx: int, uplo: str, n: int, nrhs: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor, af_local, iaf: int, jaf: int,
            descaf: DLAF_descriptor, b_local, ib: int, jb: int,
            descb: DLAF_descriptor, x_local, ix: int, jx: int,
            descx: DLAF_descriptor, ferr_out, berr_out) -> int:
    """p?porfs (its workspace arguments have no counterpart)."""
    assert (ia, ja) == (1, 1) and (iaf, jaf) == (1, 1)
    assert (ib, jb) == (1, 1) and (ix, jx) == (1, 1)
    return dlaf_cholesky_refine(ctx, uplo, a_local, _norm_desc(desca, n, n),
                                af_local, _norm_desc(descaf, n, n), b_local,
                                _norm_desc(descb, n, nrhs), x_local,
                                _norm_desc(descx, n, nrhs), ferr_out,
                                berr_out)


def pXsposv(ctx: int, uplo: str, n: int, nrhs: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor, b_local, ib: int, jb: int,
            descb: DLAF_descriptor, x_local, ix: int, jx: int,
            descx: DLAF_descriptor):
    """dsposv / zcposv over block-cyclic buffers; returns (iter, info)."""
    assert (ia, ja) == (1, 1) and (ib, jb) == (1, 1) and (ix, jx) == (1, 1)
    return dlaf_cholesky_solve_mixed(ctx, uplo, a_local,
                                     _norm_desc(desca, n, n), b_local,
                                     _norm_desc(descb, n, nrhs), x_local,
                                     _norm_desc(descx, n, nrhs))


def pXgetrf(ctx: int, m: int, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor, ipiv_out) -> int:
    """p?getrf for square matrices; ipiv 1-based global row indices."""
    assert (ia, ja) == (1, 1) and m == n, "square matrices at (1, 1) only"
    return dlaf_lu_factorization(ctx, a_local, _norm_desc(desca, n, n),
                                 ipiv_out)


def pXgetrs(ctx: int, trans: str, n: int, nrhs: int, a_local, ia: int,
            ja: int, desca: DLAF_descriptor, ipiv, b_local, ib: int, jb: int,
            descb: DLAF_descriptor) -> int:
    assert (ia, ja) == (1, 1) and (ib, jb) == (1, 1)
    return dlaf_lu_solve(ctx, trans, a_local, _norm_desc(desca, n, n), ipiv,
                         b_local, _norm_desc(descb, n, nrhs))


def pXgecon(ctx: int, norm: str, n: int, a_local, ia: int, ja: int,
            desca: DLAF_descriptor, anorm: float) -> float:
    """rcond of p?gecon (its workspace arguments have no counterpart)."""
    assert (ia, ja) == (1, 1)
    return dlaf_lu_rcond(ctx, norm, a_local, _norm_desc(desca, n, n), anorm)


def pXgesv(ctx: int, n: int, nrhs: int, a_local, ia: int, ja: int,
           desca: DLAF_descriptor, ipiv_out, b_local, ib: int, jb: int,
           descb: DLAF_descriptor) -> int:
    """p?gesv: factor, then solve unless info > 0 (B is then untouched)."""
    assert (ia, ja) == (1, 1) and (ib, jb) == (1, 1)
    da = _norm_desc(desca, n, n)
    info = dlaf_lu_factorization(ctx, a_local, da, ipiv_out)
    if info == 0:
        dlaf_lu_solve(ctx, "N", a_local, da, ipiv_out, b_local,
                      _norm_desc(descb, n, nrhs))
    return info


# dtype-suffixed aliases matching the reference's C symbol names
dlaf_pdpotrf = dlaf_pspotrf = dlaf_pcpotrf = dlaf_pzpotrf = pXpotrf
dlaf_pdpotri = dlaf_pspotri = dlaf_pcpotri = dlaf_pzpotri = pXpotri
dlaf_pdtrtri = dlaf_pstrtri = dlaf_pctrtri = dlaf_pztrtri = pXtrtri
dlaf_pdsyevd = dlaf_pssyevd = pXsyevd
dlaf_pcheevd = dlaf_pzheevd = pXsyevd
dlaf_pdsygvd = dlaf_pssygvd = pXsygvd
dlaf_pchegvd = dlaf_pzhegvd = pXsygvd
dlaf_pdlange = dlaf_pslange = dlaf_pclange = dlaf_pzlange = pXlange
dlaf_pdlansy = dlaf_pslansy = pXlansy
dlaf_pclanhe = dlaf_pzlanhe = pXlanhe
dlaf_pdlantr = dlaf_pslantr = dlaf_pclantr = dlaf_pzlantr = pXlantr
dlaf_pdpocon = dlaf_pspocon = dlaf_pcpocon = dlaf_pzpocon = pXpocon
dlaf_pdtrcon = dlaf_pstrcon = dlaf_pctrcon = dlaf_pztrcon = pXtrcon
dlaf_pdpotrs = dlaf_pspotrs = dlaf_pcpotrs = dlaf_pzpotrs = pXpotrs
dlaf_pdporfs = dlaf_psporfs = dlaf_pcporfs = dlaf_pzporfs = pXporfs
dlaf_pdsposv = dlaf_pzcposv = pXsposv
dlaf_pdgetrf = dlaf_psgetrf = dlaf_pcgetrf = dlaf_pzgetrf = pXgetrf
dlaf_pdgetrs = dlaf_psgetrs = dlaf_pcgetrs = dlaf_pzgetrs = pXgetrs
dlaf_pdgecon = dlaf_psgecon = dlaf_pcgecon = dlaf_pzgecon = pXgecon
dlaf_pdgesv = dlaf_psgesv = dlaf_pcgesv = dlaf_pzgesv = pXgesv
