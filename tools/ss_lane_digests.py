#!/usr/bin/env python
"""One SHA-256 per output array of dfm_ss_simulate and dfm_ss_news over the
inputs of their GPU suites: the simulation smoother on every
ss_sim_reference.GPU_SHAPES case (the unit-vector normals) and on the four
synthetic parity cases (70 seeded draws), the news on every
ss_news_reference case; each at the default pass and at pass_draws = 64 /
pass_releases = 64, the news also at t_lo = 5.

Two builds of the library compute the same bits exactly when their outputs of
    DFM_LIB_PATH=<build> python tools/ss_lane_digests.py > digests.txt
are identical files (DFM_LIB_PATH: as tools/ss_news_bench.py documents)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

SIM_FIELDS = ("draws", "smoothed", "smoothed_cov", "loglik")
NEWS_FIELDS = ("news", "release_forecast", "weights_f", "weights_agg", "impacts", "old", "revised", "new",
               "smoothed_old", "smoothed_revised", "smoothed_new", "smoothed_agg_old", "smoothed_agg_revised",
               "smoothed_agg_new")


def digest(label, res, fields):
    for f in fields:
        a = getattr(res, f)
        h = "none" if a is None else hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()).hexdigest()
        print(f"{label} {f} {h}", flush=True)


def main():
    import torch   # noqa: F401  (before the library: the HIP runtime must come up under torch first)
    import dfm_pkg
    import ss_news_reference as NEWS
    import ss_reference as S
    import ss_sim_reference as SIM
    D = dfm_pkg.load()
    ctx = D.Context(0)
    for shape in SIM.GPU_SHAPES:
        X, L, sigma2, A, Q, a0, _, _ = SIM.moment_case(*shape)
        T, N, r, p, h = shape
        n = SIM.nz(T + h, r, r * p)
        for pd in (None, 64):
            res = D.simulation_smoother(X, L, sigma2, A, Q, draws=n + 1, z=SIM.unit_z(n), a0=a0, horizon=h, pass_draws=pd,
                                        ctx=ctx)
            digest(f"sim moments {T}x{N}r{r}p{p}h{h} pass={pd}", res, SIM_FIELDS)
    for i in range(4):
        X, L, sigma2, A, Q, _ = S.synthetic_case(i)
        z = np.random.default_rng(2026).standard_normal((70, SIM.nz(X.shape[0], L.shape[1], A.shape[1])))
        for pd in (None, 64):
            res = D.simulation_smoother(X, L, sigma2, A, Q, draws=70, z=z, pass_draws=pd, ctx=ctx)
            digest(f"sim synthetic {i} pass={pd}", res, SIM_FIELDS)
    for i in range(NEWS.N_CASES):
        Xo, Xn, L, sigma2, A, Q, low, w = NEWS.inputs(i)
        tg = NEWS.targets(Xo.shape[0], Xo.shape[1], low)
        tg = tg[tg[:, 0] >= 5]
        for pr, t_lo in ((None, 0), (64, 0), (64, 5)):
            res = D.nowcast_news(Xo, Xn, L, sigma2, A, Q, low_freq=low, agg_weights=w, targets=tg, horizon=NEWS.HORIZON,
                                 pass_releases=pr, t_lo=t_lo, ctx=ctx)
            digest(f"news {NEWS.CASE_IDS[i]} J={len(res.releases)} pass={pr} t_lo={t_lo}", res, NEWS_FIELDS)


if __name__ == "__main__":
    main()
