"""The tiled BLAS-3 checks of ``blas3_cases.py`` on CPU tensors: all 24
{side, uplo, op, diag} cases of TRSM and TRMM, HEMM, all op pairs of the local
GEMM, TRTRI, POTRI and HEGST, with NaN in everything that must not be read and
an imaginary part on the Hermitian diagonal. Shapes are restricted to
nb <= 64; ``test_gpu_blas3.py`` runs the same assertions, and the larger tile
sizes, on the device. The measured maxima are in ``blas3_cases.py``.

The complex HEMM and HEGST cases fail without the real-diagonal contract of
``_herm_full``: with the imaginary part read, HEMM is off by the size of the
data and HEGST by about 0.1.
"""

import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blas3_cases as bc  # noqa: E402

TRI_ALL = [(s, u, o, d) for s in bc.SIDES for u in bc.UPLOS for o in bc.OPS
           for d in bc.DIAGS]
TRI_NC = [(s, u, o, d) for s in bc.SIDES for u in bc.UPLOS for o in bc.OPS_NC
          for d in bc.DIAGS]
TRI_CASES = ([(c, s) for c in TRI_ALL for s in bc.TRI_SHAPES_32]
             + [(c, s) for c in TRI_NC for s in bc.cpu_only(bc.TRI_SHAPES_BIG)])
TRI_IDS = [bc._case(*c, *s) for c, s in TRI_CASES]


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("case,shape", TRI_CASES, ids=TRI_IDS)
def test_trsm(case, shape, dtype):
    bc.check_trsm(*case, *shape, dtype)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("case,shape", TRI_CASES, ids=TRI_IDS)
def test_trmm(case, shape, dtype):
    bc.check_trmm(*case, *shape, dtype)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.TRI_SHAPES_32 + bc.cpu_only(bc.TRI_SHAPES_BIG))
@pytest.mark.parametrize("uplo", bc.UPLOS)
@pytest.mark.parametrize("side", bc.SIDES)
def test_hemm(side, uplo, shape, dtype):
    bc.check_hemm(side, uplo, *shape, dtype)


@pytest.mark.parametrize("dtype,opA,opB",
                         [(dt, a, b) for dt in bc.DTYPES for a, b in bc.gemm_ops(dt)])
@pytest.mark.parametrize("shape", bc.cpu_only(bc.GEMM_SHAPES))
def test_gemm(shape, dtype, opA, opB):
    bc.check_gemm(opA, opB, *shape, dtype)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.cpu_only(bc.TRTRI_SHAPES))
@pytest.mark.parametrize("diag", bc.DIAGS)
@pytest.mark.parametrize("uplo", bc.UPLOS)
def test_trtri(uplo, diag, shape, dtype):
    bc.check_trtri(uplo, diag, *shape, dtype)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.cpu_only(bc.POTRI_SHAPES))
@pytest.mark.parametrize("uplo", bc.UPLOS)
def test_potri(uplo, shape, dtype):
    bc.check_potri(uplo, *shape, dtype)


@pytest.mark.parametrize("dtype", bc.DTYPES)
@pytest.mark.parametrize("shape", bc.cpu_only(bc.HEGST_SHAPES))
@pytest.mark.parametrize("uplo", bc.UPLOS)
def test_hegst(uplo, shape, dtype):
    bc.check_hegst(uplo, *shape, dtype)
