"""Build & run the C-ABI test of the norm entry points (dlaf_p{d,z}lange,
dlaf_pdlansy, dlaf_pzlanhe, dlaf_pdlantr) against libdlaf_c.so: 1x1 grid,
n=48, nb=16, the (2,-1) Toeplitz matrix whose norms are known in closed form
(tests/c/test_dlaf_c_norm.c).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_c_abi_norms(tmp_path):
    lib = os.path.join(ROOT, "libdlaf_c.so")
    if not os.path.exists(lib):
        r = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_capi.sh")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    exe = str(tmp_path / "test_dlaf_c_norm")
    r = subprocess.run(
        ["gcc", "-O2",
         os.path.join(ROOT, "tests", "c", "test_dlaf_c_norm.c"),
         "-I", os.path.join(ROOT, "include"),
         "-L", ROOT, "-ldlaf_c", "-lm", f"-Wl,-rpath,{ROOT}", "-o", exe],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=280,
                       env={**os.environ, "DLAF_AMD_PYROOT": ROOT})
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}\n{r.stderr}"
    assert "OK" in r.stdout, r.stdout
