"""The simulation smoother's host arithmetic in csrc/dfm_ss_host.h from a
plain C++ compiler: tests/c_harness/ss_sim_host.cpp includes that header alone
and links nothing from the project.  Built with AddressSanitizer + UBSan.
ss_psd_cholesky runs on dyadic inputs and is checked as equalities (a rank-one
matrix, a zero matrix, a full-rank one, a zero pivot between two others); then
ss_sim_nz, every rejection of ss_sim_check_args, ss_sim_draws_per_pass with
and without a caller's pass_draws, and ss_panels_per_pass of the smoother and
the EM: M below the caps, the 65535 cap, the half-GB cap, a panel larger than
half a GB, and the two-pass shapes of the GPU tests (7 of 9 panels, 14 of 16)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_harness", "ss_sim_host.cpp")
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")


def test_ss_sim_host_header_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    binp = str(tmp_path / "ss_sim_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", binp],
                   check=True)
    p = subprocess.run([binp], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "OK"
