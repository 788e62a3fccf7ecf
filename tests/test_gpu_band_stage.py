"""Band stage on the device against the dense band matrix: the persistent
wavefront bulge chase (csrc/chase_gpu.hip) and the whole-group back-transform
kernel (csrc/bt_apply.hip). Cases, checks and the bound C = 8 (units of
n eps scale) are in ``band_stage_cases.py``; the same assertions run on CPU
tensors in ``test_band_stage.py``.

Every case runs in three combinations, so that a failure names its kernel:

    chase   GPU chase + torch GEMM chain
    bt      CPU chase + bt kernel
    both    GPU chase + bt kernel

No combination can pass on a fallback: the chase must leave its reflectors on
the device, warnings are errors (the bounded-spin fallback warns), and a
counting spy on the extension's ``bt_apply_group`` asserts that the kernel ran
once per sweep group exactly where it has an instantiation (n >= 130,
b % 16 == 0, float64 / complex128: ring sizes R = 144, 160 and 192) and
nowhere else. With E = I the column count n is never a multiple of the 64
(f64) / 32 (c128) column slice, so the ragged last slice is always covered.

Measured on an MI355X, maxima over all shapes, kinds and combinations, in
units of n eps scale (bound 8):

                  sim     orth    eig
    float32       0.84    0.50    0.29
    float64       1.55    0.80    0.70
    complex64     0.54    1.07    0.19
    complex128    0.57    0.44    0.64

The maxima sit at (5, 2) and (9, 4), where n eps is smallest; 1.55 is the CPU
chase with the torch chain at (5, 2) and is the same on CPU tensors. With the
GPU chase alone ("chase", "both") the float64 row is 0.78 / 0.70 / 0.60. Over
the cases in which the bt kernel launched: float64 0.08 / 0.11 / 0.24,
complex128 0.08 / 0.08 / 0.22.
"""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_stage_cases as bc  # noqa: E402

from dlaf_amd.ops._ext import get_ext  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# combination -> (DLAF_GPU_CHASE, DLAF_BT_KERNEL); None leaves the default
COMBOS = {
    "chase": ("1", "0"),
    "bt": ("0", None),
    "both": ("1", None),
}


@pytest.fixture
def bt_spy(monkeypatch):
    """Counts the calls of the extension's bt_apply_group by return value."""
    ext = get_ext()
    real = ext.bt_apply_group
    calls = {"launched": 0, "declined": 0, "R": set()}

    def spy(E, V, VTt, base0, b, G, R, nwin):
        ran = real(E, V, VTt, base0, b, G, R, nwin)
        if ran:
            calls["launched"] += 1
            calls["R"].add(int(R))
        else:
            calls["declined"] += 1
        return ran

    monkeypatch.setattr(ext, "bt_apply_group", spy)
    return calls


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("n,b", bc.SHAPES)
def test_band_stage_gpu(n, b, kind, dtype, combo, monkeypatch, bt_spy):
    chase_env, bt_env = COMBOS[combo]
    monkeypatch.setenv("DLAF_GPU_CHASE", chase_env)
    if bt_env is None:
        monkeypatch.delenv("DLAF_BT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("DLAF_BT_KERNEL", bt_env)
    monkeypatch.delenv("DLAF_BT_STREAMS", raising=False)
    bc.check_case(n, b, dtype, kind, device=DEV,
                  expect_gpu_chase=(chase_env == "1"), tag=combo)
    torch.cuda.synchronize()
    if combo != "chase" and bc.bt_kernel_expected(n, b, dtype):
        assert bt_spy["launched"] >= bc.sweep_groups(n), bt_spy
        assert bt_spy["declined"] == 0, bt_spy
        R = -(-(b + bc.BT_GROUP - 1) // b) * b
        assert bt_spy["R"] == {R}, bt_spy
    else:
        assert bt_spy["launched"] == 0, bt_spy
