"""The news decomposition's host arithmetic in csrc/dfm_ss_host.h from a plain
C++ compiler: tests/c_harness/ss_news_host.cpp includes that header alone and
links nothing from the project.  Built with AddressSanitizer + UBSan.  Every
refusal of the release list with the entry it names (unsorted, duplicate,
missing one, not a release, outside the panel, old not within new) on a panel
whose leading dimension exceeds T, J = 0, the revised panel, the argument
checks and the releases per pass."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_harness", "ss_news_host.cpp")
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")


def test_ss_news_host_header_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    binp = str(tmp_path / "ss_news_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", binp],
                   check=True)
    p = subprocess.run([binp], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "OK"
