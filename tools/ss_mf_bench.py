#!/usr/bin/env python
"""Timing of dfm_ss_smooth_mf and dfm_ss_em_mf (the mixed-frequency smoother and EM).

Workload: T x N = 768 x 128, r = 4, p = 2, the flow weights (1, 2, 3, 2, 1) —
the padded state has s = 20 — with the last quarter of the series
low-frequency (observed at t % 3 == 2 only) and 10 % of the rest missing at
random; M = 1 and M = --batch panels resident on the device.  Beside every
figure stands the plain kalman_smoother of the same build on the same panels at
the same state size (r = 4, p = 5, the lags beyond 2 zero): the two calls
differ by the second class's update in one row of three, the wider collapse
operands and the smoothed aggregate.  Per configuration: the wall time of a
call (best and median of --reps) and the HIP-event time per timing class of
one call through Context.read_timing — `stats` the collapse, `misc` the filter
and the smoother.  Then the same for ss_em (--iters M-steps at tol = 0 from the
drawn parameters, mixed against plain at the same state size), with `gemm` the
masked M-step GEMM and `ols` the loadings and transition kernels.

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

T, N, R, P = 768, 128, 4, 2


def panels(M, L, sigma2, A, low, w, seed):
    """(M, T, N) float64 on the device, each panel column-major, drawn from the
    mixed-frequency model, NaN = missing."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = dict(device="cuda", dtype=torch.float64)
    Ad, Ld, sd = torch.tensor(A, **dev), torch.tensor(L, **dev), torch.tensor(np.sqrt(sigma2), **dev)
    burn, nw = 50, len(w)
    f = torch.zeros((M, T + burn, R), **dev)
    u = torch.randn((M, T + burn, R), generator=g, **dev)
    for t in range(P, T + burn):
        f[:, t] = sum(f[:, t - 1 - k] @ Ad[:, k * R:(k + 1) * R].T for k in range(P)) + u[:, t]
    agg = sum(w[k] * f[:, burn - k:T + burn - k] for k in range(nw))
    lowd = torch.tensor(low, device="cuda")
    x = torch.where(lowd, agg @ Ld.T, f[:, burn:] @ Ld.T) + sd * torch.randn((M, T, N), generator=g, **dev)
    x = x.transpose(1, 2).contiguous()   # (M, N, T)
    x[torch.rand((M, N, T), generator=g, device="cuda") < 0.10] = float("nan")
    skip = torch.arange(T, device="cuda") % 3 != 2
    x[:, lowd.nonzero().ravel()[:, None], skip.nonzero().ravel()[None, :]] = float("nan")
    return x.transpose(1, 2)


def classes(tm):
    out = {}
    for k in ("stats", "misc", "gemm", "ols"):
        ms, n = tm[k]
        out[k + "_ms"] = ms
        out[k + "_launches"] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dfm_pkg
    D = dfm_pkg.load()
    ctx = D.Context(0)
    rng = np.random.default_rng(1)
    w = D.AGG_FLOW
    L = rng.standard_normal((N, R))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    A = np.hstack([0.5 * np.eye(R), 0.2 * np.eye(R)])
    Q = np.eye(R)
    low = np.zeros(N, dtype=bool)
    low[N - N // 4:] = True
    Lags = max(P, len(w))
    Aplain = np.hstack([A, np.zeros((R, R * (Lags - P)))])   # the same state size for the plain call
    x = panels(args.batch, L, sigma2, A, low, w, seed=T)
    em = dict(tol=0.0, max_iter=args.iters, ctx=ctx)
    smoother = {"mixed": lambda xs: D.kalman_smoother(xs, L, sigma2, A, Q, low_freq=low, agg_weights=w, ctx=ctx),
                "plain": lambda xs: D.kalman_smoother(xs, L, sigma2, Aplain, Q, ctx=ctx)}
    ss_em = {"mixed": lambda xs: D.ss_em(xs, L, sigma2, A, Q, low_freq=low, agg_weights=w, **em),
             "plain": lambda xs: D.ss_em(xs, L, sigma2, Aplain, Q, **em)}
    lines = []
    runs = [(k, c, m) for k, c in (("kalman_smoother", smoother), ("ss_em", ss_em)) for m in (1, args.batch)]
    for what, calls, M in runs:
        xs = x[:M]
        line = {"call": what, "T": T, "N": N, "r": R, "p": P, "n_w": len(w), "s": R * Lags, "n_low": int(low.sum()),
                "M": M, "iters": args.iters if what == "ss_em" else 0}
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
            line[name] = {"wall_ms_best": min(wall), "wall_ms_median": statistics.median(wall), **ev,
                          "loglik_mean": float(np.mean(res.loglik))}
        line["wall_ratio"] = line["mixed"]["wall_ms_median"] / line["plain"]["wall_ms_median"]
        line["misc_ratio"] = line["mixed"]["misc_ms"] / line["plain"]["misc_ms"]
        line["stats_ratio"] = line["mixed"]["stats_ms"] / line["plain"]["stats_ms"]
        if what == "ss_em":
            line["gemm_ratio"] = line["mixed"]["gemm_ms"] / line["plain"]["gemm_ms"]
            line["ols_ratio"] = line["mixed"]["ols_ms"] / line["plain"]["ols_ms"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
