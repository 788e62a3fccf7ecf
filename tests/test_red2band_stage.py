"""Reduction to band (panel QR, triangular inverse, T factor, the whole stage
with its back-transform) on CPU tensors against the inputs and an independent
product of elementary reflectors. Cases, checks and the bound are in
``red2band_cases.py``; ``test_gpu_red2band.py`` runs the same assertions on
the HIP kernels."""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import red2band_cases as rc  # noqa: E402


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("kind", rc.PANEL_KINDS)
@pytest.mark.parametrize("m,nb", rc.PANEL_SHAPES)
def test_panel_qr_cpu(m, nb, kind, dtype):
    rc.check_panel(m, nb, dtype, kind, device="cpu")


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("n", rc.TRI_SIZES)
def test_tri_inverse_full_cpu(n, lower, unit, dtype):
    rc.check_tri_inverse(n, lower, unit, dtype, device="cpu")


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("m,k", rc.TFACTOR_SHAPES)
def test_t_factor_cpu(m, k, dtype):
    rc.check_t_factor(m, k, dtype, device="cpu")


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("kind", rc.STAGE_KINDS)
@pytest.mark.parametrize("n,band", rc.STAGE_SHAPES)
def test_red2band_stage_cpu(n, band, kind, dtype):
    rc.check_stage(n, band, dtype, kind, device="cpu")


def test_holes_panel_has_degenerate_columns():
    """The ``holes`` panel does reach the degenerate branch beyond column 0:
    a third of the taus are exactly zero, none in ``rand``."""
    import torch
    from dlaf_amd.algs.red2band import panel_qr_
    m, nb = 65, 64
    zeros = {}
    for kind in ("rand", "holes"):
        P = rc.panel(m, nb, "float64", kind).clone()
        taus = torch.zeros(nb, dtype=P.dtype)
        panel_qr_(P, taus)
        zeros[kind] = int((taus == 0).sum())
    assert zeros["rand"] == 0 and zeros["holes"] >= len(range(0, nb, 3)), zeros
