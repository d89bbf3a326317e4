#!/usr/bin/env python
"""Timing of dfm_ss_smooth_ar (the smoother with AR(1) idiosyncratic terms).

Workload: T x N = 768 x 128, r = 4, p = 2 (the padded state is the plain one,
s = 8), 10 % of the entries missing at random plus a ragged edge (the last
1..12 rows of every fourth series), rho ~ U(-0.8, 0.8); M = 1 and M = --batch
panels resident on the device.  Beside every figure stands the plain
kalman_smoother of the same build on the same panels at the same state size:
the two calls differ by the collapse (four operand images, two half-stages) and
by the update's size, 2r against r.  Per configuration: the wall time of a call
(best and median of --reps) and the HIP-event time per timing class of one call
through Context.read_timing — `stats` the collapse, `misc` the filter and the
smoother.

--plain-only times the plain call alone, and --root loads the package of
another checkout with its own build of the library: the parent commit's plain
call on the same panels is the figure to hold this build's plain call against.

One JSON line per configuration on stdout; --out appends them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, N, R, P = 768, 128, 4, 2


def panels(M, L, sigma2, rho, A, seed):
    """(M, T, N) float64 on the device, each panel column-major, drawn from the
    model with AR(1) idiosyncratic terms, NaN = missing."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = dict(device="cuda", dtype=torch.float64)
    Ad, Ld, sd, rh = (torch.tensor(v, **dev) for v in (A, L, np.sqrt(sigma2), rho))
    burn = 50
    f = torch.zeros((M, T + burn, R), **dev)
    e = torch.zeros((M, T + burn, N), **dev)
    u = torch.randn((M, T + burn, R), generator=g, **dev)
    v = torch.randn((M, T + burn, N), generator=g, **dev)
    for t in range(P, T + burn):
        f[:, t] = sum(f[:, t - 1 - k] @ Ad[:, k * R:(k + 1) * R].T for k in range(P)) + u[:, t]
        e[:, t] = rh * e[:, t - 1] + sd * v[:, t]
    x = (f[:, burn:] @ Ld.T + e[:, burn:]).transpose(1, 2).contiguous()   # (M, N, T)
    x[torch.rand((M, N, T), generator=g, device="cuda") < 0.10] = float("nan")
    for i in range(0, N, 4):
        x[:, i, T - 1 - (i // 4) % 12:] = float("nan")
    return x.transpose(1, 2)


def classes(tm):
    out = {}
    for k in ("stats", "misc"):
        ms, n = tm[k]
        out[k + "_ms"] = ms
        out[k + "_launches"] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and build are timed")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import dfm_pkg
    D = dfm_pkg.load()
    ctx = D.Context(0)
    rng = np.random.default_rng(1)
    L = rng.standard_normal((N, R))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    rho = rng.uniform(-0.8, 0.8, size=N)
    A = np.hstack([0.5 * np.eye(R), 0.2 * np.eye(R)])
    Q = np.eye(R)
    x = panels(args.batch, L, sigma2, rho, A, seed=T)
    calls = {"plain": lambda xs: D.kalman_smoother(xs, L, sigma2, A, Q, ctx=ctx)}
    if not args.plain_only:
        calls["ar"] = lambda xs: D.kalman_smoother(xs, L, sigma2, A, Q, idio_ar=rho, ctx=ctx)
    lines = []
    for M in (1, args.batch):
        xs = x[:M]
        line = {"call": "kalman_smoother", "label": args.label, "T": T, "N": N, "r": R, "p": P, "s": R * max(P, 2), "M": M}
        for name, call in calls.items():
            call(xs)   # warm-up
            wall = []
            for _ in range(args.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                res = call(xs)
                wall.append((time.perf_counter() - t0) * 1e3)
            ctx.enable_timing(True)
            ctx.reset_timing()
            call(xs)
            ev = classes(ctx.read_timing())
            ctx.enable_timing(False)
            line[name] = {"wall_ms": wall, "wall_ms_best": min(wall), "wall_ms_median": statistics.median(wall), **ev,
                          "loglik_mean": float(np.mean(res.loglik))}
        if "ar" in line:
            line["wall_ratio"] = line["ar"]["wall_ms_median"] / line["plain"]["wall_ms_median"]
            line["misc_ratio"] = line["ar"]["misc_ms"] / line["plain"]["misc_ms"]
            line["stats_ratio"] = line["ar"]["stats_ms"] / line["plain"]["stats_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
