"""The tiled BLAS-3 checks of ``blas3_cases.py`` on the device: the
``device.type == "cuda"`` branches of TRSM, TRMM, HEMM, GEMM, TRTRI, POTRI and
HEGST (descriptor tables, panel offsets, in-place staging, two-stream
schedules), which share no code with the torch branches that
``test_blas3_cases.py`` and ``test_triangular.py`` run. Inputs, references,
the bound C = 8 and the shape tables are in ``blas3_cases.py``.

No case can pass on a torch fallback: counting spies on the extension's
``batch_gemm`` and ``trtri_lower`` assert the launch counts that the
algorithms' schedules imply (for nt tile rows of the triangular / Hermitian
matrix):

    GEMM              1 fused launch, whatever the tile grid
    TRSM, TRMM        2 nt - 1 (one diagonal step per k, one update but the last)
    TRSM Left/Lower/NoTrans  nt + (nt - 1) + (nt - 2): solve, head, tail
    HEMM              3 nt - 2 (stored part, mirrored part, diagonal)
    TRSM, TRTRI, POTRI  ``trtri_lower`` once per leaf of every diagonal tile
    HEGST Lower       twice that (hoisted inverses and the diagonal transform)

``_hegst_local_upper`` is torch by design (correctness-grade per-tile ops) and
is exempt: its launch counts must be zero. Fast-path spies on
``_trsm_lln_local_gpu`` and ``_trtri_local_gpu`` assert that the two-stream
paths are entered exactly for Left/Lower/NoTrans and for nt > 2, and nowhere
else. The two-stream paths also run twice from the same input (LLN TRSM at
nt = 5, TRTRI at nt = 11) and must give bitwise equal results: the summation
order is fixed, so a difference is a missing event.

Measured on an MI355X, maxima over all cases and shapes in units of k eps
(bound 8):

                  TRSM   TRMM   HEMM   GEMM   TRTRI  POTRI  HEGST
    float32       0.05   0.08   0.04   0.12   0.02   0.08   0.03
    float64       0.05   0.06   0.05   0.07   0.04   0.14   0.04
    complex64     0.05   0.07   0.04   0.08   0.06   0.10   0.02
    complex128    0.06   0.11   0.05   0.10   0.05   0.13   0.03

The maxima sit at the orders below nb (20 at nb = 32), where the unit is
smallest; they are of the size of the CPU path's (``blas3_cases.py``), the
largest difference being 0.09 (complex128 GEMM). Every case passed at the
first run: the device paths read no NaN, keep the padding and repeat bitwise.
Wall time of this file on an MI355X: 12 s for its 1532 cases.

Not run on the device: mutants. The K stride ``b_ks`` of ``_general_local``
and the chunk offsets of ``_trtri_local_gpu`` have no CPU path; by reading,
``b_ks = ts`` for NoTrans would walk B along a tile row instead of down a
tile column, which differ in every GEMM shape here with 4 K tiles and 2 tile
columns, and an off-by-one in ``tile_off(k + 2 + c, k)`` pairs every chunk
with the wrong tile of column k from nt = 3 on; either error is of the size
of the data, 1e6 (float32) to 1e15 (float64) times the bound.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blas3_cases as bc  # noqa: E402

from dlaf_amd.algs import inverse as inverse_mod  # noqa: E402
from dlaf_amd.algs import triangular as triangular_mod  # noqa: E402
from dlaf_amd.ops._ext import get_ext  # noqa: E402
from dlaf_amd.types import Diag, Op, Side, UpLo  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture
def spy(monkeypatch):
    """Counts the extension's batch_gemm and trtri_lower launches and the
    entries into the two two-stream fast paths."""
    ext = get_ext()
    real_gemm, real_trtri = ext.batch_gemm, ext.trtri_lower
    real_lln = triangular_mod._trsm_lln_local_gpu
    real_tt = inverse_mod._trtri_local_gpu
    calls = {"batch_gemm": 0, "trtri_lower": 0, "lln": 0, "trtri_fast": 0}

    def batch_gemm(C, *args):
        assert C.is_cuda
        calls["batch_gemm"] += 1
        return real_gemm(C, *args)

    def trtri_lower(L, T, *args):
        assert L.is_cuda and T.is_cuda
        calls["trtri_lower"] += 1
        return real_trtri(L, T, *args)

    def lln(*args):
        calls["lln"] += 1
        return real_lln(*args)

    def trtri_fast(*args):
        calls["trtri_fast"] += 1
        return real_tt(*args)

    monkeypatch.setattr(ext, "batch_gemm", batch_gemm)
    monkeypatch.setattr(ext, "trtri_lower", trtri_lower)
    monkeypatch.setattr(triangular_mod, "_trsm_lln_local_gpu", lln)
    monkeypatch.setattr(inverse_mod, "_trtri_local_gpu", trtri_fast)
    return calls


def leaves(n: int) -> int:
    """Kernel launches of the recursive split of ``tri_inverse_full``."""
    if n <= 128:
        return 1
    h = min(((n + 1) // 2 + 63) // 64 * 64, n - 1)
    return leaves(h) + leaves(n - h)


def is_lln(case) -> bool:
    side, uplo, op, _ = case
    return side == Side.Left and uplo == UpLo.Lower and op == Op.NoTrans


def expect(spy, **want):
    torch.cuda.synchronize()
    full = {"batch_gemm": 0, "trtri_lower": 0, "lln": 0, "trtri_fast": 0}
    full.update(want)
    if full["batch_gemm"] is None:      # at least one launch, count not modelled
        assert spy["batch_gemm"] >= 1, spy
        full["batch_gemm"] = spy["batch_gemm"]
    assert spy == full, (spy, full)


TRI_ALL = [(s, u, o, d) for s in bc.SIDES for u in bc.UPLOS for o in bc.OPS
           for d in bc.DIAGS]
TRI_NC = [(s, u, o, d) for s in bc.SIDES for u in bc.UPLOS for o in bc.OPS_NC
          for d in bc.DIAGS]
TRI_CASES = ([(c, s) for c in TRI_ALL for s in bc.TRI_SHAPES_32]
             + [(c, s) for c in TRI_NC for s in bc.TRI_SHAPES_BIG])
TRI_IDS = [bc._case(*c, *s) for c, s in TRI_CASES]


def trsm_counts(case, nb, ka, repeat=False):
    nt = bc.nt_of(ka, nb)
    runs = 2 if repeat else 1
    gemms = nt + max(nt - 1, 0) + max(nt - 2, 0) if is_lln(case) else 2 * nt - 1
    return dict(batch_gemm=runs * gemms, trtri_lower=runs * nt * leaves(nb),
                lln=runs * int(is_lln(case)))


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("case,shape", TRI_CASES, ids=TRI_IDS)
def test_trsm_gpu(case, shape, dtype, spy):
    nb, ka, _ = shape
    repeat = is_lln(case) and bc.nt_of(ka, nb) >= 5
    bc.check_trsm(*case, *shape, dtype, device=DEV, tag="gpu", repeat=repeat)
    expect(spy, **trsm_counts(case, nb, ka, repeat))


@pytest.mark.parametrize("dtype", bc.REAL_DTYPES)
def test_trsm_right_nb256_gpu(dtype, spy):
    """Right side at nb = 256: the recursive tile inverse and the staged
    in-place multiply of the real dtypes."""
    case = (Side.Right, UpLo.Lower, Op.ConjTrans, Diag.NonUnit)
    nb, ka, _ = bc.TRI_SHAPE_256
    bc.check_trsm(*case, *bc.TRI_SHAPE_256, dtype, device=DEV, tag="gpu")
    expect(spy, **trsm_counts(case, nb, ka))


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("case,shape", TRI_CASES, ids=TRI_IDS)
def test_trmm_gpu(case, shape, dtype, spy):
    nb, ka, _ = shape
    bc.check_trmm(*case, *shape, dtype, device=DEV, tag="gpu")
    expect(spy, batch_gemm=2 * bc.nt_of(ka, nb) - 1)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.TRI_SHAPES_32 + bc.TRI_SHAPES_BIG)
@pytest.mark.parametrize("uplo", bc.UPLOS)
@pytest.mark.parametrize("side", bc.SIDES)
def test_hemm_gpu(side, uplo, shape, dtype, spy):
    nb, ka, _ = shape
    bc.check_hemm(side, uplo, *shape, dtype, device=DEV, tag="gpu")
    expect(spy, batch_gemm=3 * bc.nt_of(ka, nb) - 2)


@pytest.mark.parametrize("dtype,opA,opB",
                         [(dt, a, b) for dt in bc.DTYPES for a, b in bc.gemm_ops(dt)])
@pytest.mark.parametrize("shape", bc.GEMM_SHAPES)
def test_gemm_gpu(shape, dtype, opA, opB, spy):
    bc.check_gemm(opA, opB, *shape, dtype, device=DEV, tag="gpu")
    expect(spy, batch_gemm=1)


def trtri_counts(nb, n, runs=1):
    nt = bc.nt_of(n, nb)
    return dict(batch_gemm=None if nt > 1 else 0,
                trtri_lower=runs * nt * leaves(nb), trtri_fast=runs * int(nt > 2))


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.TRTRI_SHAPES)
@pytest.mark.parametrize("diag", bc.DIAGS)
@pytest.mark.parametrize("uplo", bc.UPLOS)
def test_trtri_gpu(uplo, diag, shape, dtype, spy):
    nb, n = shape
    repeat = bc.nt_of(n, nb) >= 11
    bc.check_trtri(uplo, diag, *shape, dtype, device=DEV, tag="gpu", repeat=repeat)
    expect(spy, **trtri_counts(nb, n, 2 if repeat else 1))


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("diag", bc.DIAGS)
@pytest.mark.parametrize("ksplit", bc.KSPLITS)
def test_trtri_ksplit_gpu(ksplit, diag, dtype, spy, monkeypatch):
    """nt = 11 with 9 planes of one tile and with chunks of 3, 3, 3."""
    monkeypatch.setenv("DLAF_TRTRI_KSPLIT", str(ksplit))
    nb, n = bc.TRTRI_KSPLIT_SHAPE
    bc.check_trtri(UpLo.Lower, diag, nb, n, dtype, device=DEV, tag="gpu",
                   repeat=True, note=f"/ksplit{ksplit}")
    expect(spy, **trtri_counts(nb, n, 2))


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.POTRI_SHAPES)
@pytest.mark.parametrize("uplo", bc.UPLOS)
def test_potri_gpu(uplo, shape, dtype, spy):
    nb, n = shape
    bc.check_potri(uplo, *shape, dtype, device=DEV, tag="gpu")
    counts = trtri_counts(nb, n)
    counts["batch_gemm"] = None          # the LAUUM stage always launches
    expect(spy, **counts)


HEGST_CASES = ([(u, s, dt) for u in bc.UPLOS for s in bc.HEGST_SHAPES
                for dt in bc.DTYPES]
               + [(UpLo.Lower, bc.HEGST_SHAPE_256, dt) for dt in bc.REAL_DTYPES])


@pytest.mark.parametrize("uplo,shape,dtype", HEGST_CASES,
                         ids=[bc._case(u, *s, dt) for u, s, dt in HEGST_CASES])
def test_hegst_gpu(uplo, shape, dtype, spy):
    nb, n = shape
    bc.check_hegst(uplo, *shape, dtype, device=DEV, tag="gpu")
    if uplo == UpLo.Upper:
        expect(spy)                      # torch by design: nothing launched
    else:
        expect(spy, batch_gemm=None,
               trtri_lower=2 * bc.nt_of(n, nb) * leaves(nb))
