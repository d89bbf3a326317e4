"""The split products' refinement in csrc/dfm_fact_plan.h (terms, z0_planes,
mid_planes, products_split3) from a plain C++ compiler: tests/c_harness/
fact_plan3_host.cpp includes that header alone and links nothing from the
project.  Built with AddressSanitizer + UBSan.  Over test_fact_plan_host's
input sweep crossed with all 2^7 switch settings (split3_off added) it asserts
that every plan is consistent(); that terms is 3 exactly for the Split products
sp <= d0 - 2 with DFM_FACT_SPLIT3 on, 6 for every other split product and 0
elsewhere; that prep and every middle step write the planes the product behind
them reads (2 for three terms, 3 for six); that products_split3 counts the
three-term products and the switch changes no other field; and that plans
broken by hand to three terms behind three planes, or six terms behind two
planes, are inconsistent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_harness", "fact_plan3_host.cpp")
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")


def test_fact_plan3_header_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    binp = str(tmp_path / "fact_plan3_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", binp],
                   check=True)
    p = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == "OK"
