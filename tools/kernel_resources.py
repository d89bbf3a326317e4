#!/usr/bin/env python3
"""The compiler's resource report of one csrc file's kernels as a table:
    tools/kernel_resources.py dfm_ss_em.hip [--raw report.txt] > table.txt
compiles the file for gfx950 (device code only, the Makefile's flags) with
-Rpass-analysis=kernel-resource-usage, or reads a saved report, and prints
per kernel SGPRs, VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block
and the occupancy.  Needs no GPU."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamicfactormodels.jl_amd", "csrc")
FIELDS = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occupancy"))


def report(src):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull],
                       capture_output=True, text=True, check=True)
    return p.stderr


def parse(text):
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return rows


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return [n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for n in out.splitlines()]
    except (OSError, subprocess.CalledProcessError):
        return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", help="a file of csrc/, e.g. dfm_ss_em.hip")
    ap.add_argument("--raw", help="read this saved compiler report instead of compiling")
    a = ap.parse_args()
    rows = parse(open(a.raw).read() if a.raw else report(a.source))
    rows.sort(key=lambda r: r["name"])
    names = demangle([r["name"] for r in rows])
    print(f"# {a.source}: -Rpass-analysis=kernel-resource-usage, gfx950")
    print(f"{'kernel':44s}" + "".join(f"{h:>10s}" for _, h in FIELDS))
    for r, n in zip(rows, names):
        print(f"{n:44s}" + "".join(f"{r.get(k, -1):>10d}" for k, _ in FIELDS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
