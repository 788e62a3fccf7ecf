"""Reduction to band on the device against the inputs and an independent
product of elementary reflectors: the cooperative panel QR kernel
(csrc/panel_qr.hip), the triangular inverse kernels behind
``tri_inverse_full`` (csrc/factor.hip), ``t_factor`` on top of them, and the
whole stage with its back-transform. Cases, checks and the bound C = 8 are in
``red2band_cases.py``; the same assertions run on CPU tensors in
``test_red2band_stage.py``.

No case can pass on a fallback: counting spies on the extension's ``panel_qr``
and ``trtri_lower`` assert that the panel kernel ran exactly once per panel
(once per layout of a panel case, ``len(panels)`` times per stage case) and
that the inverse kernel ran once per leaf of the recursive split (at least
once per ``t_factor``), every output must live on the device, and warnings are
errors. Panels are factored one at a time on the current stream.

Measured on an MI355X, maxima over all shapes, kinds and layouts, in the units
of ``red2band_cases.py`` (bound 8):

                  panel QR       inverse        T      whole stage
                  rec    orth    left   right   wy     sim    orth   eig    bt
    float32       0.42   0.65    0.13   0.20    0.18   0.40   0.59   0.15   0.20
    float64       0.61   1.00    0.25   0.25    0.11   0.51   0.50   0.32   0.22
    complex64     0.64   0.73    0.26   0.26    0.07   0.52   0.50   0.30   0.47
    complex128    0.66   0.83    0.21   0.37    0.11   0.82   0.40   0.55   0.50

The maxima sit at the smallest shapes ((2, 1), (3, 5), n <= 9), where the unit
is smallest; from m = 64 / n = 130 on, no figure exceeds 0.2.

These tests found one defect: ``tri_inverse_full(A, lower=False)`` of a 1 x 1
complex tile returned 1 / conj(a). The adjoint view of a 1 x 1 tensor is
already contiguous, so ``.mH.contiguous()`` kept the lazy conjugate bit that
the kernel never sees. It reached the stage through ``t_factor`` whenever the
last panel was one column wide (n - band = 1 mod band) and gave sim and bt
figures of 1e4 to 1e15 there.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import red2band_cases as rc  # noqa: E402

from dlaf_amd.ops._ext import get_ext  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of the extension's panel_qr and trtri_lower."""
    ext = get_ext()
    real_qr, real_trtri = ext.panel_qr, ext.trtri_lower
    calls = {"panel_qr": 0, "trtri_lower": 0}

    def panel_qr(P, taus, norms, wraw):
        assert P.is_cuda and taus.is_cuda
        calls["panel_qr"] += 1
        return real_qr(P, taus, norms, wraw)

    def trtri_lower(L, T, n, ldl, ldt, unit_diag):
        assert L.is_cuda and T.is_cuda
        calls["trtri_lower"] += 1
        return real_trtri(L, T, n, ldl, ldt, unit_diag)

    monkeypatch.setattr(ext, "panel_qr", panel_qr)
    monkeypatch.setattr(ext, "trtri_lower", trtri_lower)
    return calls


def trtri_leaves(n: int) -> int:
    """Kernel launches of the recursive split of ``tri_inverse_full``."""
    if n <= 128:
        return 1
    h = min(((n + 1) // 2 + 63) // 64 * 64, n - 1)
    return trtri_leaves(h) + trtri_leaves(n - h)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("kind", rc.PANEL_KINDS)
@pytest.mark.parametrize("m,nb", rc.PANEL_SHAPES)
def test_panel_qr_gpu(m, nb, kind, dtype, spy):
    rc.check_panel(m, nb, dtype, kind, device=DEV, tag="gpu")
    torch.cuda.synchronize()
    assert spy["panel_qr"] == len(rc.LAYOUTS), spy
    assert spy["trtri_lower"] == 0, spy


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("n", rc.TRI_SIZES)
def test_tri_inverse_full_gpu(n, lower, unit, dtype, spy):
    rc.check_tri_inverse(n, lower, unit, dtype, device=DEV, tag="gpu")
    torch.cuda.synchronize()
    assert spy["trtri_lower"] == trtri_leaves(n), spy
    assert spy["panel_qr"] == 0, spy


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("m,k", rc.TFACTOR_SHAPES)
def test_t_factor_gpu(m, k, dtype, spy):
    rc.check_t_factor(m, k, dtype, device=DEV, tag="gpu")
    torch.cuda.synchronize()
    assert spy["trtri_lower"] == trtri_leaves(k), spy
    assert spy["panel_qr"] == 0, spy


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("kind", rc.STAGE_KINDS)
@pytest.mark.parametrize("n,band", rc.STAGE_SHAPES)
def test_red2band_stage_gpu(n, band, kind, dtype, spy):
    rc.check_stage(n, band, dtype, kind, device=DEV, tag="gpu")
    torch.cuda.synchronize()
    panels = rc.expected_panels(n, band)
    assert spy["panel_qr"] == len(panels), spy
    # one T factor per panel in the reduction, one in the back-transform
    assert spy["trtri_lower"] == 2 * sum(trtri_leaves(nrefl)
                                         for _, _, nrefl in panels), spy
