"""csrc/dfm_fact_ws.h from a plain C++ compiler: tests/c_harness/fact_ws_host.cpp
includes that header alone and links nothing from the project.  Built with
AddressSanitizer + UBSan.  Over T in {1, 15, 16, 17, 120, 121, 500, 2730, 2731,
4096}, nb in {1, 7, 64, 1250}, P in {16, 32} and pz in {2, 12, P} the program
asserts that the factored solver's workspace regions
  - are in ascending order and do not overlap,
  - each hold at least what their consumer indexes (Z: z_rows(T) nb pz doubles,
    HZ: T nb pz, ab: nb 32 P, PF: nb T 16, e2: nb T, FV: nb 16 P, FtF: 256),
  - start on 16-byte boundaries,
  - and that `total` is the closed-form sum fact_workspace_bytes returned
    before the header existed, and the offsets the solver's former pointer
    arithmetic (FV and FtF 8 bytes later where nb T is odd)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_harness", "fact_ws_host.cpp")
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")


def test_fact_ws_header_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    binp = str(tmp_path / "fact_ws_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", binp],
                   check=True)
    p = subprocess.run([binp], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "OK"
