#!/usr/bin/env python
"""Timing of dfm_ss_simulate (the simulation smoother) beside the only other
route to the same draws: one dfm_ss_smooth call on M = D pseudo-panels that
share the panel's mask.

Shape: 768 x 128, r = 8, p = 2, 10 % missing at random plus a 6-row ragged
edge on every 5th column; the panel, the pseudo-panels and z resident on the
device; D = 256 and D = 4096 (--draws).  After a warm-up call it reports, per
D, the wall time of a call (a host clock around a call that ends in a stream
synchronise; best and median of --reps) and, from one further call, the
HIP-event time of each kernel through Context.read_timing.

  --route sim     simulation_smoother: collapse (class `stats`), filter +
                  smoother (`misc`), ss_gain_kernel (`ols`), ss_sim_kernel
                  (`factors`), ss_transpose_kernel (`gemm`)
  --route panels  kalman_smoother on the D pseudo-panels: collapse (`stats`),
                  filter + smoother (`misc`).  Building the pseudo-panels is
                  not timed.  DFM_LIB_PATH may name an earlier build of the
                  library (one without dfm_ss_simulate loads too).
  --ratio A B     reads the two routes' --out files and prints panels / sim
                  per D.

One JSON line per D on stdout; --out appends them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, N, R, P = 768, 128, 8, 2


def parameters(rng):
    L = rng.standard_normal((N, R))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    A = np.hstack([0.5 * np.eye(R)] + [0.2 / k * np.eye(R) for k in range(1, P)])
    return L, sigma2, A, np.eye(R)


def panel(seed):
    """(T, N) float64 on the device, column-major, NaN = missing."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((N, T), generator=g, device="cuda", dtype=torch.float64)
    x[torch.rand((N, T), generator=g, device="cuda") < 0.10] = float("nan")
    x[::5, T - 6:] = float("nan")
    return x.t()


def load_library():
    import ctypes
    import dfm_pkg
    D = dfm_pkg.load()
    have = hasattr(ctypes.CDLL(D._lib.LIB_PATH), "dfm_ss_simulate")
    if not have:   # an earlier build: bind what it has
        D._lib.SIGNATURES[:] = [s for s in D._lib.SIGNATURES if s[0] != "dfm_ss_simulate"]
    return D, have


def timed(ctx, call, reps):
    call()   # warm-up
    wall = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.enable_timing(True)
    ctx.reset_timing()
    call()
    tm = ctx.read_timing()
    ctx.enable_timing(False)
    return wall, tm


def ratio(a, b):
    rows = {}
    for path in (a, b):
        for line in open(path):
            rec = json.loads(line)
            rows.setdefault(rec["D"], {})[rec["route"]] = rec["wall_ms_median"]
    for d in sorted(rows):
        if {"sim", "panels"} <= set(rows[d]):
            print(json.dumps({"D": d, "panels_ms": rows[d]["panels"], "sim_ms": rows[d]["sim"],
                              "ratio": rows[d]["panels"] / rows[d]["sim"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("sim", "panels"), default="sim")
    ap.add_argument("--draws", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ratio", nargs=2, metavar=("A", "B"), default=None)
    args = ap.parse_args()
    if args.ratio:
        return ratio(*args.ratio)
    import torch
    D, have_sim = load_library()
    if args.route == "sim" and not have_sim:
        raise SystemExit(f"{D._lib.LIB_PATH} has no dfm_ss_simulate")
    ctx = D.Context(0)
    L, sigma2, A, Q = parameters(np.random.default_rng(1))
    x = panel(seed=T)
    nz = R * P + 2 * R * T
    lines = []
    for nd in args.draws:
        g = torch.Generator(device="cuda").manual_seed(nd)
        if args.route == "sim":
            z = torch.randn((nz, nd), generator=g, device="cuda", dtype=torch.float64).T
            res = []
            call = lambda: res.__setitem__(slice(None), [D.simulation_smoother(x, L, sigma2, A, Q, draws=nd, z=z, ctx=ctx)])  # noqa: E731
            wall, tm = timed(ctx, call, args.reps)
            line = {"gain_ms": tm["ols"][0], "sim_ms": tm["factors"][0], "sim_launches": tm["factors"][1],
                    "transpose_ms": tm["gemm"][0], "finite": bool(np.isfinite(res[0].draws).all())}
            del z
        else:   # pseudo-panels: the panel's mask, other values
            xs = x.t().contiguous()[None] + torch.randn((nd, N, T), generator=g, device="cuda", dtype=torch.float64)
            xs = xs.transpose(1, 2)
            res = []
            call = lambda: res.__setitem__(slice(None), [D.kalman_smoother(xs, L, sigma2, A, Q, ctx=ctx)])  # noqa: E731
            wall, tm = timed(ctx, call, args.reps)
            line = {"finite": bool(np.isfinite(res[0].smoothed).all())}
            del xs
        line = {"route": args.route, "library": os.path.basename(os.path.dirname(D._lib.LIB_PATH)) + "/" +
                os.path.basename(D._lib.LIB_PATH), "T": T, "N": N, "r": R, "p": P, "D": nd,
                "wall_ms_best": min(wall), "wall_ms_median": statistics.median(wall), "wall_ms_all": wall,
                "collapse_ms": tm["stats"][0], "recursion_ms": tm["misc"][0], **line}
        print(json.dumps(line), flush=True)
        lines.append(line)
        res.clear()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
