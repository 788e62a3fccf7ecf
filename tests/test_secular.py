"""Secular-equation roots of the torch path on the CPU against a 50-digit
reference. Inputs, reference and bounds: ``secular_cases.py``;
``test_gpu_secular.py`` runs the same assertions on the HIP kernels."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import secular_cases as sc  # noqa: E402

from dlaf_amd.algs.tridiag_dc import _secular_roots  # noqa: E402


@pytest.mark.parametrize("name", sc.NAMES)
def test_secular_roots_cpu(name):
    d, z, rho = sc.case(name)
    sidx, mu = _secular_roots(torch.from_numpy(d.copy()),
                              torch.from_numpy(z.copy()), rho)
    sc.check(name, sidx.numpy(), mu.numpy(), "cpu")
