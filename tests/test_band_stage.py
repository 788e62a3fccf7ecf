"""Band stage (bulge chase + back-transform) on CPU tensors against the dense
band matrix: the native C++ chase and the torch GEMM chain. Cases, checks and
the bound are in ``band_stage_cases.py``; ``test_gpu_band_stage.py`` runs the
same assertions on the HIP kernels."""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_stage_cases as bc  # noqa: E402


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("n,b", bc.SHAPES)
def test_band_stage_cpu(n, b, kind, dtype):
    bc.check_case(n, b, dtype, kind, device="cpu", expect_gpu_chase=False)


def test_holes_have_zero_reflectors():
    """The ``holes`` kind does produce tau == 0 reflectors beyond the
    trailing length-1 ones every chase ends with."""
    from dlaf_amd.algs.band2tridiag import chase_band
    n, b = 67, 16
    zeros = {}
    for kind in ("rand", "holes"):
        store, _, _ = bc.case(n, b, "float64", kind)
        tri = chase_band(store.clone(), b)
        zeros[kind] = int((tri.vstore[:, 0] == 0).sum())
    assert zeros["holes"] > zeros["rand"], zeros
