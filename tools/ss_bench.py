#!/usr/bin/env python
"""Timing of dfm_ss_smooth (the Kalman smoother of the state-space pass).

Shapes (T, N, r, p): (768, 128, 8, 2), FRED-MD sized, and (500, 2000, 8, 2),
the C3 panel; each at M = 1 and M = 256 panels resident on the device (10 %
missing at random, a 6-row ragged edge on every 5th column).  After a warm-up
call it reports, per configuration, the wall time of a call (best and median
of --reps), the HIP-event time of the collapse kernel (timing class `stats`)
and of the recursion kernels (class `misc`) through Context.read_timing, and
the wall time of M single-panel calls beside the one batched call.

One JSON line per configuration on stdout; --out appends them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((768, 128, 8, 2), (500, 2000, 8, 2))


def parameters(N, r, p, rng):
    L = rng.standard_normal((N, r))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    A = np.hstack([0.5 * np.eye(r)] + [0.2 / k * np.eye(r) for k in range(1, p)])
    return L, sigma2, A, np.eye(r)


def panels(M, T, N, seed):
    """(M, T, N) float64 on the device, each panel column-major, NaN = missing."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((M, N, T), generator=g, device="cuda", dtype=torch.float64)
    x[torch.rand((M, N, T), generator=g, device="cuda") < 0.10] = float("nan")
    x[:, ::5, T - 6:] = float("nan")
    return x.transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dfm_pkg
    D = dfm_pkg.load()
    ctx = D.Context(0)
    rng = np.random.default_rng(1)
    lines = []
    for T, N, r, p in SHAPES:
        L, sigma2, A, Q = parameters(N, r, p, rng)
        x = panels(args.batch, T, N, seed=T)
        for M in (1, args.batch):
            xs = x[:M]
            D.kalman_smoother(xs, L, sigma2, A, Q, ctx=ctx)   # warm-up
            wall = []
            for _ in range(args.reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                res = D.kalman_smoother(xs, L, sigma2, A, Q, ctx=ctx)
                wall.append((time.perf_counter() - t0) * 1e3)
            ctx.enable_timing(True)
            ctx.reset_timing()
            D.kalman_smoother(xs, L, sigma2, A, Q, ctx=ctx)
            tm = ctx.read_timing()
            ctx.enable_timing(False)
            line = {"T": T, "N": N, "r": r, "p": p, "M": M, "wall_ms_best": min(wall),
                    "wall_ms_median": statistics.median(wall), "collapse_ms": tm["stats"][0],
                    "collapse_launches": tm["stats"][1], "recursion_ms": tm["misc"][0],
                    "recursion_launches": tm["misc"][1], "loglik_finite": bool(np.all(np.isfinite(res.loglik)))}
            if M > 1:   # the same panels one call each
                t0 = time.perf_counter()
                for b in range(M):
                    D.kalman_smoother(x[b], L, sigma2, A, Q, ctx=ctx)
                line["wall_ms_single_calls"] = (time.perf_counter() - t0) * 1e3
                line["batch_speedup"] = line["wall_ms_single_calls"] / line["wall_ms_median"]
            print(json.dumps(line), flush=True)
            lines.append(line)
        del x
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
