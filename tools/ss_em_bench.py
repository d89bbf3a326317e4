#!/usr/bin/env python
"""Timing of dfm_ss_em (the quasi-ML EM of the state-space factor model).

Shapes (T, N, r, p) of tools/ss_bench.py: (768, 128, 8, 2) and (500, 2000, 8,
2); panels simulated from drawn parameters (10 % missing at random, a 6-row
ragged edge on every 5th column), resident on the device; every call runs
--iters M-steps at tol = 0 from the drawn parameters.  Per configuration
(M = 1 and M = --batch) it reports the wall time of a call (best and median of
--reps), the HIP-event time per timing class of one call through
Context.read_timing — `stats` the collapse, `misc` the filter and the smoother
with its moments (and a call's one empty-column launch: the recursion per
E-step is misc_ms over stats_launches), `gemm` the masked M-step GEMM, `ols` the loadings and
transition kernels — each also per launch, and beside them the same classes of
one kalman_smoother call at the same shape (the smoother without the moments),
so the table shows what the moments add to a pass.  For the batch it times
--singles single-panel calls against the one batched call.  --numpy times the
NumPy reference (tests/ss_em_reference.py) on the host for --numpy-iters
iterations of one panel.  --blocks B runs the EM with B equal factor blocks
(dfm_ss_em_blocks): block 0 global, series i a member of block 1 + i % (B - 1),
the loadings drawn with the restriction's zeros.

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


def blocks_of(N, r, B):
    """(sizes, N x B membership, N x r free mask) of B equal blocks, the first global."""
    if B < 2 or r % B:
        raise SystemExit(f"--blocks must divide r = {r} into at least two blocks")
    member = np.zeros((N, B), dtype=bool)
    member[:, 0] = True
    member[np.arange(N), 1 + np.arange(N) % (B - 1)] = True
    return (r // B,) * B, member, np.repeat(member, r // B, axis=1)


def panels(M, T, N, L, sigma2, A, seed):
    """(M, T, N) float64 on the device, each panel column-major, drawn from the
    model (so the EM has something to fit), NaN = missing."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, s = A.shape
    dev = dict(device="cuda", dtype=torch.float64)
    Ad, Ld, sd = torch.tensor(A, **dev), torch.tensor(L, **dev), torch.tensor(np.sqrt(sigma2), **dev)
    st = torch.zeros((M, s), **dev)
    f = torch.zeros((M, T + 50, r), **dev)
    u = torch.randn((M, T + 50, r), generator=g, **dev)
    for t in range(T + 50):
        ft = st @ Ad.T + u[:, t]
        st = torch.cat([ft, st[:, :s - r]], dim=1)
        f[:, t] = ft
    x = (f[:, 50:] @ Ld.T + sd * torch.randn((M, T, N), generator=g, **dev)).transpose(1, 2).contiguous()   # (M, N, T)
    x[torch.rand((M, N, T), generator=g, device="cuda") < 0.10] = float("nan")
    x[:, 1::5, T - 6:] = float("nan")
    x[:, 0, :] = torch.nan_to_num(x[:, 0, :])   # no empty column, whatever the draw
    return x.transpose(1, 2)


def classes(tm):
    out = {}
    for k in ("stats", "misc", "gemm", "ols"):
        ms, n = tm[k]
        out[k + "_ms"] = ms
        out[k + "_launches"] = n
        out[k + "_ms_per_launch"] = ms / n if n else 0.0
    return out


def numpy_reference(T, N, r, p, iters, rng):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import ss_em_reference as R
    L, sigma2, A, Q = parameters(N, r, p, rng)
    f = np.zeros((T + 50, r * p))
    for t in range(1, T + 50):
        f[t] = np.concatenate([A @ f[t - 1] + rng.standard_normal(r), f[t - 1, :r * (p - 1)]])
    X = f[50:, :r] @ L.T + np.sqrt(sigma2) * rng.standard_normal((T, N))
    X[rng.uniform(size=X.shape) < 0.10] = np.nan
    X[T - 6:, 1::5] = np.nan
    X[:, 0] = np.nan_to_num(X[:, 0])
    t0 = time.perf_counter()
    res = R.em(X, L, sigma2, A, Q, tol=0.0, max_iter=iters)
    dt = time.perf_counter() - t0
    return {"T": T, "N": N, "r": r, "p": p, "numpy_iters": iters, "numpy_s": dt, "numpy_s_per_iteration": dt / max(iters, 1),
            "numpy_loglik_gain": float(res["path"][-1] - res["path"][0]), "cpus": os.cpu_count()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--singles", type=int, default=None, help="single-panel calls to time (default: the batch)")
    ap.add_argument("--shapes", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--numpy", action="store_true", help="time the NumPy reference instead of the device")
    ap.add_argument("--numpy-iters", type=int, nargs="*", default=[20, 1])
    ap.add_argument("--blocks", type=int, default=0, help="B > 1: the EM with B equal factor blocks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    if args.numpy:
        for k in args.shapes:
            emit(numpy_reference(*SHAPES[k], args.numpy_iters[min(k, len(args.numpy_iters) - 1)], rng))
    else:
        import dfm_pkg
        D = dfm_pkg.load()
        ctx = D.Context(0)
        kw = dict(tol=0.0, max_iter=args.iters, ctx=ctx)
        for k in args.shapes:
            T, N, r, p = SHAPES[k]
            L, sigma2, A, Q = parameters(N, r, p, rng)
            kw.pop("factor_blocks", None), kw.pop("block_members", None)
            if args.blocks:
                sizes, member, free = blocks_of(N, r, args.blocks)
                L = L * free
                kw.update(factor_blocks=sizes, block_members=member)
            x = panels(args.batch, T, N, L, sigma2, A, seed=T)
            for M in (1, args.batch):
                xs = x[:M]
                res = D.ss_em(xs, L, sigma2, A, Q, **kw)   # warm-up
                wall = []
                for _ in range(args.reps):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    res = D.ss_em(xs, L, sigma2, A, Q, **kw)
                    wall.append((time.perf_counter() - t0) * 1e3)
                ctx.enable_timing(True)
                ctx.reset_timing()
                D.ss_em(xs, L, sigma2, A, Q, **kw)
                em = classes(ctx.read_timing())
                ctx.reset_timing()
                D.kalman_smoother(xs, L, sigma2, A, Q, ctx=ctx)
                ks = classes(ctx.read_timing())
                ctx.enable_timing(False)
                gain = res.loglik_path[:, -1] - res.loglik_path[:, 0]
                line = {"T": T, "N": N, "r": r, "p": p, "M": M, "blocks": args.blocks, "iters": args.iters,
                        "wall_ms_best": min(wall),
                        "wall_ms_median": statistics.median(wall),
                        "wall_ms_per_iteration": statistics.median(wall) / args.iters, "em": em,
                        "kalman_smoother": {k2: v for k2, v in ks.items() if k2.startswith(("stats", "misc"))},
                        "iterations": int(res.iterations.min()), "loglik_gain_min": float(gain.min()),
                        "path_rises": bool((np.diff(res.loglik_path, axis=1) > 0).all())}
                if M > 1:   # the same panels one call each
                    n1 = min(args.singles or M, M)
                    t0 = time.perf_counter()
                    for b in range(n1):
                        D.ss_em(x[b], L, sigma2, A, Q, **kw)
                    dt = (time.perf_counter() - t0) * 1e3
                    line["single_calls_timed"] = n1
                    line["wall_ms_single_calls"] = dt * M / n1
                    line["batch_speedup"] = line["wall_ms_single_calls"] / line["wall_ms_median"]
                emit(line)
            del x
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
