"""The host functions of the AR(1) idiosyncratic terms in csrc/dfm_ss_host.h
from a plain C++ compiler: tests/c_harness/ss_ar_host.cpp includes that header
alone and links nothing from the project.  Built with AddressSanitizer + UBSan
and run as its own program.  The limits, the checks of rho, the clamp and the
fallback of the two-step estimate, and the three cases of the fill rule (and
rho = 0) are checked as equalities against hand-worked cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_harness", "ss_ar_host.cpp")
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")


def test_ss_ar_host_functions_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    binp = str(tmp_path / "ss_ar_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", binp],
                   check=True)
    p = subprocess.run([binp], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "OK"
