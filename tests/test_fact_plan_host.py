"""csrc/dfm_fact_plan.h from a plain C++ compiler: tests/c_harness/fact_plan_host.cpp
includes that header alone and links nothing from the project.  Built with
AddressSanitizer + UBSan.  The program holds the rule as eig_run_fact2_t
spelled it before the header existed (its chain of booleans, the two ternaries
of its step-0 loop, the Z0 format, the two counters, the pad-row condition) and
asserts that plan_first_filter returns the same for every field, over all 2^6
settings of DFM_FACT_STEP0, DFM_FACT_F32, DFM_FACT_SPLIT, DFM_FACT_SPLIT_LAST,
DFM_FACT_PF and DFM_AP2_PROBE crossed with
  T in {15, 16, 17, 120, 121}, (r, p, P) in {(4, 8, 16), (5, 10, 16),
  (8, 12, 16), (13, 18, 32)}, tol in {-1e-10, 1e-10}, H32 and Hs present or
  absent, hmax in {1, 0, inf}, spread in {0.5, 1.6, 50} (not warm, degree 6,
  degree 3), maxit in {1, 2, 30}, kw below k and at least k (and lamk, fscale
  positive or zero),
that every one of these plans is consistent(), and that three hand-broken
plans are not: a Split product behind an F32 Z, an F64 product behind Split
planes, a last Horner step behind Chunk32 (and a fourth: unwritten pad rows)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_harness", "fact_plan_host.cpp")
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")


def test_fact_plan_header_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    binp = str(tmp_path / "fact_plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", binp],
                   check=True)
    p = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "OK"
