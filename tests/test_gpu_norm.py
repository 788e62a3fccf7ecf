"""matrix_norm on the device (csrc/norms.hip): the CPU table (with the
misaligned float32 / complex64 tile bases of nb=17) plus the shapes of
norm_cases.GPU_SHAPES, whose tiles span several 64-row strips and several
column blocks in every dtype, so the strip / block indexing, the row sums
carried across blocks and the mask-free interior path run; device against the
host twin; bitwise repeatability; NaN / inf; Frobenius extremes; one 2-rank
case on one GPU."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as nc  # noqa: E402
from dist_utils import run_distributed  # noqa: E402

from dlaf_amd import UpLo, Diag  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(s, v) for s in nc.SHAPES + nc.GPU_SHAPES
         for v in nc.variants_for(s[0], s[1])]


def _id(case):
    (m, n, mb, nb), (structure, uplo, diag) = case
    u = "" if uplo is None else uplo.value
    d = "unit" if diag == Diag.Unit else ""
    return f"{m}x{n}-{mb}x{nb}-{structure}{u}{d}"


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_norms_against_reference_and_host_twin(case, dtype):
    (m, n, mb, nb), (structure, uplo, diag) = case
    got = nc.check_case(m, n, mb, nb, dtype, structure, uplo, diag, DEV)
    # the host twin, within twice the bound
    a = nc.stored_with_garbage(nc.make_general(m, n, dtype), structure, uplo,
                               diag)
    host = nc.all_norms(nc.to_matrix(a, mb, nb, "cpu"), structure, uplo, diag)
    ref = nc.reference(a, structure, uplo, diag)
    for k in nc.NORMS:
        rel = 2 * nc.bound(k, dtype, ref[k][1])
        assert abs(got[k] - host[k]) <= rel * abs(host[k]), (k, got[k],
                                                              host[k])
    # two device calls on the same data: the same bits
    mat = nc.to_matrix(a, mb, nb, DEV)
    assert (nc.all_norms(mat, structure, uplo, diag)
            == nc.all_norms(mat, structure, uplo, diag) == got)


def test_unaligned_storage_takes_scalar_path():
    """A float32 storage that starts 4 bytes into its allocation cannot use
    16-byte loads; the result is the one of the aligned storage."""
    from dlaf_amd import Matrix
    a = nc.make_general(40, 40, "float32")
    mat = nc.to_matrix(a, 16, 16, DEV)
    want = nc.all_norms(mat, "general", None, Diag.NonUnit)
    flat = torch.zeros(mat.storage.numel() + 1, dtype=torch.float32,
                       device=DEV)
    flat[1:] = mat.storage.reshape(-1)
    shifted = Matrix(mat.dist, mat.dtype, mat.device, None,
                     _storage=flat[1:].view(mat.storage.shape))
    assert shifted.storage.data_ptr() % 16 != 0
    assert nc.all_norms(shifted, "general", None, Diag.NonUnit) == want


def test_more_workgroups_than_one_launch_takes():
    """2900 x 2900 tiles of 1 x 1 are 8.41 million workgroups, above the 2^23
    of one launch: the kernel is launched twice, the second time from a
    workgroup offset."""
    from dlaf_amd.ops._ext import get_ext
    t = 2900
    a = torch.rand(t, t, dtype=torch.float64, device=DEV) - 0.5
    rows, cols, scal = get_ext().matrix_norms(a.view(t, t, 1, 1), t, t, 0, 1,
                                              0, 1, 0, 0, False)
    eps = nc.eps_of("float64")
    assert scal[0].item() == a.abs().max().item()
    for got, dim in ((rows, 1), (cols, 0)):
        want = a.abs().sum(dim=dim)
        assert ((got - want).abs() <= 2 * (t + 2) * eps * want).all()
    assert scal[1].item() == 0.0 and scal[3].item() == 0.0
    want = (a * a).sum().item()
    assert abs(scal[2].item() - want) <= 2 * (t * t + 4) * eps * want


def test_nan_and_inf_propagate():
    nc.check_nan_inf(DEV, "float64")
    nc.check_nan_inf(DEV, "complex64")


def test_frobenius_extremes():
    nc.check_fro_extremes(DEV)


def _worker_two_ranks(rank, ws):
    from dlaf_amd import CommGrid
    torch.cuda.set_device(0)
    grid = CommGrid(1, 2, device=torch.device("cuda", 0))
    a = nc.stored_with_garbage(nc.make_general(96, 96, "float64"),
                               "hermitian", UpLo.Lower, Diag.NonUnit)
    mat = nc.to_matrix(a, 32, 32, "cuda", grid=grid)
    out = nc.all_norms(mat, "hermitian", UpLo.Lower, Diag.NonUnit, grid)
    torch.cuda.synchronize()
    return out


@pytest.mark.timeout(600)
def test_two_ranks_one_gpu():
    outs = run_distributed(_worker_two_ranks, 2)
    assert outs[0] == outs[1]
    a = nc.stored_with_garbage(nc.make_general(96, 96, "float64"),
                               "hermitian", UpLo.Lower, Diag.NonUnit)
    nc.check_against_reference(outs[0], a, "float64", "hermitian", UpLo.Lower,
                               Diag.NonUnit)
