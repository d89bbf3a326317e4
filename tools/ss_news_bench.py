#!/usr/bin/env python
"""Timing of dfm_ss_news (the news decomposition) beside the only other route
to the same weights: one dfm_ss_smooth_mf call on M = J impulse panels that
share the new vintage's mask.

Shape: tools/ss_mf_bench.py's panel, 768 x 128, r = 4, p = 2, the flow weights
(1, 2, 3, 2, 1) (s = 20), the last 32 series low-frequency, 10 % of the rest
missing at random.  The releases are J = 32 and J = 256 (--releases) of the
observed entries of the last three rows, evenly spread over them.  After a
warm-up call it reports, per J, the wall time of a call (a host clock around
the call; best and median of --reps) and, from one further call, the HIP-event
time of each kernel class through Context.read_timing.

  --route news    nowcast_news on the two host vintages: three smooths (collapse
                  `stats`, filter + smoother `misc`), ss_gain_kernel
                  (`ols`), ss_news_kernel (`factors`), the transposes (`gemm`)
  --route panels  kalman_smoother on J panels resident on the device, zero on
                  the new mask but for a one at release j, a0 = 0: panel j's
                  smoothed path is release j's weights.  Building the panels is
                  not timed.  DFM_LIB_PATH may name an earlier build of the
                  library (one without dfm_ss_news loads too).
  --ratio A B     reads the two routes' --out files and prints panels / news
                  per J.

One JSON line per J on stdout; --out appends them to a file."""
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
W = (1.0, 2.0, 3.0, 2.0, 1.0)


def model(rng):
    L = rng.standard_normal((N, R))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    A = np.hstack([0.5 * np.eye(R), 0.2 * np.eye(R)])
    low = np.zeros(N, dtype=bool)
    low[N - N // 4:] = True
    return L, sigma2, A, np.eye(R), low


def new_vintage(rng, L, sigma2, A, low):
    """(T, N) host panel drawn from the mixed-frequency model, NaN = missing."""
    burn, nw = 50, len(W)
    f = np.zeros((T + burn, R))
    for t in range(P, T + burn):
        f[t] = sum(A[:, k * R:(k + 1) * R] @ f[t - 1 - k] for k in range(P)) + rng.standard_normal(R)
    agg = sum(W[k] * f[burn - k:T + burn - k] for k in range(nw))
    x = np.where(low, agg @ L.T, f[burn:] @ L.T) + np.sqrt(sigma2) * rng.standard_normal((T, N))
    x[rng.uniform(size=(T, N)) < 0.10] = np.nan
    x[np.ix_(np.arange(T) % 3 != 2, low)] = np.nan
    return x


def old_vintage(xn, J):
    """X_new without J of the observed entries of its last three rows."""
    edge = np.argwhere(~np.isnan(xn[T - 3:]))
    edge[:, 0] += T - 3
    if J > len(edge):
        raise SystemExit(f"only {len(edge)} observed entries in the last three rows")
    xo = xn.copy()
    for t, i in edge[np.linspace(0, len(edge) - 1, J).round().astype(int)]:
        xo[t, i] = np.nan
    return xo


def load_library():
    import ctypes
    import dfm_pkg
    D = dfm_pkg.load()
    have = hasattr(ctypes.CDLL(D._lib.LIB_PATH), "dfm_ss_news")
    if not have:   # an earlier build: bind what it has
        D._lib.SIGNATURES[:] = [s for s in D._lib.SIGNATURES if s[0] != "dfm_ss_news"]
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
            rows.setdefault(rec["J"], {})[rec["route"]] = rec["wall_ms_median"]
    for j in sorted(rows):
        if {"news", "panels"} <= set(rows[j]):
            print(json.dumps({"J": j, "panels_ms": rows[j]["panels"], "news_ms": rows[j]["news"],
                              "ratio": rows[j]["panels"] / rows[j]["news"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("news", "panels"), default="news")
    ap.add_argument("--releases", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ratio", nargs=2, metavar=("A", "B"), default=None)
    args = ap.parse_args()
    if args.ratio:
        return ratio(*args.ratio)
    import torch   # noqa: F401  (before the library: the HIP runtime must come up under torch first)
    D, have_news = load_library()
    if args.route == "news" and not have_news:
        raise SystemExit(f"{D._lib.LIB_PATH} has no dfm_ss_news")
    ctx = D.Context(0)
    rng = np.random.default_rng(1)
    L, sigma2, A, Q, low = model(rng)
    xn = new_vintage(rng, L, sigma2, A, low)
    lines = []
    for J in args.releases:
        xo = old_vintage(xn, J)
        res = []
        if args.route == "news":
            tg = np.array([(T - 1, N - 1), (T - 1, 0)])
            call = lambda: res.__setitem__(slice(None), [D.nowcast_news(xo, xn, L, sigma2, A, Q, targets=tg, low_freq=low, agg_weights=W, ctx=ctx)])  # noqa: E731,E501
            wall, tm = timed(ctx, call, args.reps)
            o = res[0]
            move = o.smoothed_new - o.smoothed_revised
            line = {"gain_ms": tm["ols"][0], "news_ms": tm["factors"][0], "news_launches": tm["factors"][1],
                    "transpose_ms": tm["gemm"][0], "smooth_launches": tm["misc"][1],
                    "identity": float(np.max(np.abs(move - np.einsum("j,jtk->tk", o.news, o.weights_f))) /
                                      np.max(np.abs(o.smoothed_new)))}
        else:
            rel = np.argwhere(~np.isnan(xn) & np.isnan(xo))
            imp = np.where(np.isnan(xn), np.nan, 0.0)[None].repeat(J, axis=0)
            imp[np.arange(J), rel[:, 0], rel[:, 1]] = 1.0
            xs = torch.from_numpy(np.ascontiguousarray(imp.transpose(0, 2, 1))).cuda().transpose(1, 2)
            s = R * max(P, len(W))
            call = lambda: res.__setitem__(slice(None), [D.kalman_smoother(xs, L, sigma2, A, Q, a0=np.zeros(s), low_freq=low, agg_weights=W, ctx=ctx)])  # noqa: E731,E501
            wall, tm = timed(ctx, call, args.reps)
            line = {"finite": bool(np.isfinite(res[0].smoothed).all())}
            del xs
        line = {"route": args.route, "library": os.path.basename(os.path.dirname(D._lib.LIB_PATH)) + "/" +
                os.path.basename(D._lib.LIB_PATH), "T": T, "N": N, "r": R, "p": P, "n_w": len(W), "J": J,
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
