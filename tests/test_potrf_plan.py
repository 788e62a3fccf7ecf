"""Host-side check of the fused tile Cholesky's work decomposition.

Builds tools/check_potrf_plan.cpp (plain C++ over csrc/potrf_plan.h, its own
``main``) with AddressSanitizer and UBSan and runs it on the CPU: which
workgroup writes which block for every launch and every tile size, including
sizes that are no multiple of 64."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_potrf_plan_ownership(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "check_potrf_plan")
    subprocess.run(
        [cxx, "-std=c++17", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csrc"),
         os.path.join(ROOT, "tools", "check_potrf_plan.cpp"), "-o", exe],
        check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "potrf_plan ok" in out.stdout
