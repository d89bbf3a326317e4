#!/usr/bin/env python3
"""Secondary measurements: the BASELINE.json configs other than the headline
C3 (bench.py).  One JSON line per config on stdout; the CPU column is the
reference-faithful oracle (oracle/dfm_oracle.py) on this host, bounded.

    python tools/bench_configs.py [--configs c1,c2,c2s,c4,c5,mc,em] [--cpu] [--reps K]

c1  Simulated DFM T=200 N=100 r=3: fit + Bai-Ng IC sweep k<=8 (all 7 criteria)
c2  FRED-MD-shaped T=600 N=130, r by ICp2 over 1..8, wild bootstrap B=999 with
    LR/LM/Wald for all 130 variables at bp=300 (+ V, ICp2)      [replicates/s]
c2s the sup-Chow sweep at C2's shape and fit: dfm_chow_sweep (LR/LM/Wald, every
    date of the 15 %-trimmed range) against the host loop of dfm_chow_all over
    the same dates, alternating; wild bootstrap B=999 of the sup-LM alone and
    of all three sup statistics beside the single-date C2 job       [ms]
mc  Monte-Carlo batch: M=1000 Bai-Ng panels T=100 N=60 r=3, kmax 8 — selection
    only, and with the sup-LM of every variable at r=3 — monte_carlo (dfm_mc)
    against the per-panel loop it replaces (DynamicFactorModel + chow_sweep),
    alternating, end to end with uploads; per-class kernel split    [x, ms]
em  EM fit of a panel with missing entries (em_factors, dfm_em), r=8: a
    FRED-MD-like T=720 N=128 panel (~5 % missing, ragged edges, late starters)
    and C3's shape T=500 N=2000, against the host loop a caller writes
    without it (NumPy fill + normalize + principal_components per iteration,
    the same iteration count), alternating                           [x, ms]
c4  Targeted predictors T=400 N=5000: hard per-candidate t-stats, soft
    glmnetcv lasso (100 lambdas x 10 folds), then PCA (r=5) on the soft
    selection                                                  [selections/s]
c5  T=2000 N=20000: P=200 expanding windows, IC sweep (ICp2, kmax 8) each
    (src/utils.jl:54-72 refit loop)                               [windows/s]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import dfm_oracle as O
    return O


def cores():
    try:
        from threadpoolctl import threadpool_info
        return max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
    except Exception:
        return os.cpu_count()


def c1(D, ctx, args):
    rng = np.random.default_rng(20261015 + 1)
    y, x, *_ = D.factor_model_DGP(200, 100, 3, rng=rng)
    x = D.normalize(x)
    w = np.ones((200, 1))
    s = timed(lambda: D.DynamicFactorModel(y, w, x, "ICp2", kmax=8, ctx=ctx), args.reps, ctx.synchronize)
    rec = {"config": "c1", "workload": "fit + IC sweep k<=8, T=200 N=100 (host buffers in/out)",
           "value": round(1.0 / s, 3), "unit": "fits/s", "ms": round(s * 1e3, 3)}
    if args.cpu:
        O = oracle()
        t0 = time.perf_counter()
        O.DynamicFactorModel_ic(y, w, x, "ICp2", kmax=8)
        O.ic_sweep_values(y, w, x, 8)
        el = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": round(1 / el, 3), "unit": "fits/s", "cores": cores(), "kind": "port",
                               "sample": "1 oracle IC sweep (8 brute-force refits) + all-criteria table"}
    return rec


def c2_pmc_bytes(prefix):
    """DRAM bytes per launch of the C2 kernel named `prefix` from the latest
    committed C2 PMC passes (profiles/rNN_pmc_traffic_c2.json,
    tools/pmc_traffic.py; one launch = one 500-replicate lane); None when absent."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic_c2.json")))
    if not files:
        return None
    rec = json.load(open(files[-1]))
    for k, v in rec.items():
        if k.startswith(prefix):
            return {"hbm_bytes_per_launch": v.get("hbm_bytes_per_launch"), "source": os.path.basename(files[-1])}
    return None


def c2(D, ctx, args):
    import torch
    rng = np.random.default_rng(20261015 + 2)
    T, N, B, bp = 600, 130, 999, 300
    y, x, *_ = D.factor_model_DGP(T, N, 3, model="Breitung_Eickmeier_2011", b=0.5, rng=rng)
    x = D.normalize(x)
    w = np.ones((T, 1))
    model = D.DynamicFactorModel(y, w, x, "ICp2", kmax=8, ctx=ctx)
    S = D.Stat
    stats = [S.V(), S.criterion(), S.LR_all(bp), S.LM_all(bp), S.Wald_all(bp)]
    arr = D.api._stat_array(stats)
    width = int(ctx.lib.dfm_stats_width(model.handle, arr, len(stats)))
    idx, eta = D.draw_wild_fast(7, B, T)
    dev = torch.device("cuda", 0)
    di, de = torch.from_numpy(idx).to(dev), torch.from_numpy(eta).to(dev)
    out = torch.empty((B, width), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def run():
        ctx.check(ctx.lib.dfm_bootstrap_dev(model.handle, 0, B, di.data_ptr(), de.data_ptr(), arr, len(stats),
                                            out.data_ptr()))
    run()
    ctx.synchronize()
    ctx.reset_timing()
    ctx.enable_timing(True)
    s = timed(run, args.reps, ctx.synchronize)
    ctx.enable_timing(False)
    tm = ctx.read_timing()
    rec = {"config": "c2", "workload": f"wild bootstrap B={B}, T={T} N={N} r={model.number_of_factors}, "
                                       f"LR/LM/Wald all variables at bp={bp} + V + ICp2 (inputs resident)",
           "value": round(B / s, 1), "unit": "replicates/s", "ms_per_job": round(s * 1e3, 3),
           "kernels_ms_per_job": {k: round(v[0] / (args.reps + 1), 4) for k, v in tm.items() if v[1]}}
    es = ctx.eig_stats()
    rec["eig_iterations"] = dict(es, rayleigh_ritz_steps_per_replicate=round(
        es["replicate_iterations"] / (B * (args.reps + 1)), 3))
    # Gram roofline: the replicate Grams X*'X* (130 x 130 over T = 600), SYRK
    # count N (N + 1) T per replicate (the weighted GEMM Q = W K
    # of the gram_wk path does 2 T N (N + 1) / 2, the same count), over the
    # HIP-event time of the whole Gram phase (prep + GEMM + combine)
    gms, gn = tm.get("gram", (0.0, 0))
    if gn:
        flop = B * (args.reps + 1) * N * (N + 1) * T
        rec["roofline_gram"] = {"kernel": "gram_wk: prep (w, B = F'DPE) + ONE batch GEMM Q = W K on gemmh_kernel "
                                          "(v_mfma_f64_4x4x4_4b) + tiled symmetric combine",
                                "bound": "mfma", "achieved": round(flop / (gms * 1e-3) / 1e12, 3), "peak": 78.6,
                                "unit": "TFLOP/s", "frac": round(flop / (gms * 1e-3) / 1e12 / 78.6, 4),
                                "avg_launch_ms": round(gms / gn, 4), "flop_per_replicate": N * (N + 1) * T}
    # Chow pass, labelled by its measured bound: fp64 VALU.  Per
    # (replicate, variable) and row t, pass A forms e = x - F_t l (r FMA), ||e||^2
    # (1) and F_t'x (r); pass B the subperiod residuals u, rs (2 r), ssr (1),
    # u^2 z_t (r) and the HC0 block's r (r + 1) / 2 sums: 5 r + 2 + r (r + 1) / 2
    # FMA = 2 x that in flop.  Its DRAM traffic (PMC FETCH_SIZE / WRITE_SIZE,
    # profiles/*_pmc_traffic_c2.json) is far below HBM peak: the gathered x rows
    # come from the L2-resident C and E panels.
    # Fused direct eigensolver (eig_fused_kernel, class eig_gq): MFMA products
    # G S of the replicate's m x m Gram with the 16-column block, 2 m^2 16 flop
    # each; dfm_ctx_gemm_products counts them exactly (a[i] replicates at
    # Rayleigh-Ritz step i, dg(i) products each).  A per-replicate latency
    # chain (one workgroup per replicate): the frac says how far from the MFMA
    # peak that chain runs, the PMC bytes that it is not HBM-bound either.
    ems, en = tm.get("eig_gq", (0.0, 0))
    if en and es.get("gemm_products"):
        m = min(T, N)
        fl = 2.0 * m * m * 16 * es["gemm_products"]
        tf = fl / (ems * 1e-3) / 1e12
        rec["roofline_eig_fused"] = {"kernel": "eig_fused_kernel (one workgroup per replicate, Q and Y in LDS, "
                                               "G streamed from L2/MALL, v_mfma_f64_4x4x4_4b)",
                                     "bound": "mfma (latency chain)", "achieved": round(tf, 3), "peak": 78.6,
                                     "unit": "TFLOP/s", "frac": round(tf / 78.6, 4),
                                     "products_per_replicate": round(es["gemm_products"] / (B * (args.reps + 1)), 2),
                                     "flop_per_product": 2 * m * m * 16,
                                     "traffic": c2_pmc_bytes("eig_fused_kernel")}
    cms, cn = tm.get("chow", (0.0, 0))
    if cn:
        r = model.number_of_factors
        fl = B * (args.reps + 1) * N * T * 2 * (5 * r + 2 + r * (r + 1) // 2)
        tf = fl / (cms * 1e-3) / 1e12
        rec["roofline_chow"] = {"kernel": "chow_prep + chow_all_kernel", "bound": "valu (fp64)",
                                "achieved": round(tf, 3), "peak": 78.6, "unit": "TFLOP/s",
                                "frac": round(tf / 78.6, 4),
                                "flop_per_replicate": N * T * 2 * (5 * r + 2 + r * (r + 1) // 2),
                                "traffic": c2_pmc_bytes("chow_all_kernel")}
    if args.cpu:
        O = oracle()
        o = O.DynamicFactorModel_ic(y, w, x, "ICp2", kmax=8)
        C, E = o.common_component, o.factor_residuals
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.cpu_seconds or n < 1:
            d = O.DynamicFactorModel(y, w, C + eta[n][:, None] * E[idx[n]], o.number_of_factors, "ICp2")
            for i in range(N):
                O.LR_test(d, bp, i), O.LM_test(d, bp, i), O.Wald_test(d, bp, i)
            n += 1
        el = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": round(n / el, 4), "unit": "replicates/s", "cores": cores(), "kind": "port",
                               "sample": f"{n} oracle replicates (refit + 3 x {N} Chow tests) in {el:.1f} s"}
    return rec


def c4(D, ctx, args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    rng = np.random.default_rng(20261015 + 4)
    T, N = 400, 5000
    y, x, *_ = D.factor_model_DGP(T, N, 5, rng=rng)
    x = D.normalize(x)
    w = np.ones((T, 1))
    folds = D.glmnet_default_folds(T, np.random.default_rng(404))
    parts = {}

    def run():
        t0 = time.perf_counter()
        hard = D.targeted_predictors(y, w, x, "hard", "per_candidate", ctx=ctx)
        t1 = time.perf_counter()
        soft = D.targeted_predictors(y, w, x, "soft", folds=folds, ctx=ctx)
        t2 = time.perf_counter()
        D.principal_components(x[:, soft], 5, ctx=ctx)
        t3 = time.perf_counter()
        parts.update(hard_ms=(t1 - t0) * 1e3, soft_ms=(t2 - t1) * 1e3, pca_ms=(t3 - t2) * 1e3,
                     n_hard=int(hard.sum()), n_soft=int(soft.sum()))
    s = timed(run, args.reps, ctx.synchronize)
    rec = {"config": "c4", "workload": "hard per-candidate t-stats + soft glmnetcv (100 lambdas, 10 folds) "
                                       "+ PCA r=5 on the soft selection, T=400 N=5000 (host buffers in/out)",
           "value": round(1.0 / s, 3), "unit": "selections/s", "ms": round(s * 1e3, 2),
           "parts_ms": {k: round(v, 2) for k, v in parts.items() if k.endswith("ms")},
           "selected": {"hard": parts["n_hard"], "soft": parts["n_soft"]}}
    if args.cpu:
        O = oracle()
        t0 = time.perf_counter()
        O.targeted_predictors_hard(y, w, x, "per_candidate")
        t1 = time.perf_counter()
        m, _ = O.targeted_predictors_soft(y, w, x, folds)
        t2 = time.perf_counter()
        O.principal_components(x[:, m], T, int(m.sum()))
        el = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": round(1 / el, 5), "unit": "selections/s", "cores": cores(), "kind": "port",
                               "sample": f"1 oracle selection: hard {t1 - t0:.1f} s, soft {t2 - t1:.1f} s"}
    return rec


def c5(D, ctx, args):
    rng = np.random.default_rng(20261015 + 5)
    T, N, P = 2000, 20000, 200
    y, x, *_ = D.factor_model_DGP(T, N, 8, rng=rng)
    # column-major host panel, as a Julia caller hands it over (no harness
    # transpose inside the timed region; the PCIe upload stays in)
    x = np.asfortranarray(D.normalize(x))
    w = np.asfortranarray(np.ones((T, 1)))
    out = {}
    s = timed(lambda: out.update(D.pseudo_out_of_sample_refits(y, w, x, "ICp2", num_predictions=P, kmax=8,
                                                                ctx=ctx)), max(1, args.reps // 2), ctx.synchronize)
    rec = {"config": "c5", "workload": f"{P} expanding windows (rows 1..t-1, t = T-P+1..T) x IC sweep ICp2 "
                                       f"kmax 8, T={T} N={N} (host panel in, per-window results out)",
           "value": round(P / s, 2), "unit": "windows/s", "ms_per_job": round(s * 1e3, 1),
           "r_selected": sorted(set(int(v) for v in out["number_of_factors"]))}
    if args.cpu:
        O = oracle()
        t0 = time.perf_counter()
        O.DynamicFactorModel_ic(y[:T - 1], w[:T - 1], x[:T - 1], "ICp2", kmax=8)
        el = time.perf_counter() - t0
        rec["cpu_baseline"] = {"value": round(1 / el, 5), "unit": "windows/s", "cores": cores(), "kind": "port",
                               "sample": f"1 oracle window (T-1 rows, 8 brute-force refits) in {el:.1f} s"}
    return rec


def c2s(D, ctx, args):
    import torch
    rng = np.random.default_rng(20261015 + 2)
    T, N, B, bp = 600, 130, 999, 300
    y, x, *_ = D.factor_model_DGP(T, N, 3, model="Breitung_Eickmeier_2011", b=0.5, rng=rng)
    x = D.normalize(x)
    w = np.ones((T, 1))
    model = D.DynamicFactorModel(y, w, x, "ICp2", kmax=8, ctx=ctx)
    r = model.number_of_factors
    lo, hi = D.sup_chow_range(T, r)

    def loop():
        return np.array([D.chow_all(model, b) for b in range(lo, hi + 1)])   # (dates, 3, N)
    res, ref = D.chow_sweep(model, lo, hi), loop()
    agree = max(float(np.max(np.abs(res.sup[n] - ref[:, k].max(axis=0)) / ref[:, k].max(axis=0)))
                for k, n in enumerate(D.api.SUP_CHOW_STATS))
    dates_equal = all(np.array_equal(res.argsup[n], lo + ref[:, k].argmax(axis=0))
                      for k, n in enumerate(D.api.SUP_CHOW_STATS))
    # the two alternate, each timed by the host clock around calls that end in a stream synchronise
    ts, tl = [], []
    for _ in range(max(args.reps, 5) * 4):
        t0 = time.perf_counter()
        for _ in range(20):
            D.chow_sweep(model, lo, hi)
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        ts.append((t1 - t0) / 20)
        tl.append(t2 - t1)
    ctx.reset_timing()
    ctx.enable_timing(True)
    D.chow_sweep(model, lo, hi)
    ctx.enable_timing(False)
    sweep_kernels_ms = ctx.read_timing()["chow"][0]
    S = D.Stat
    idx, eta = D.draw_wild_fast(7, B, T)
    dev = torch.device("cuda", 0)
    di, de = torch.from_numpy(idx).to(dev), torch.from_numpy(eta).to(dev)
    jobs = {"single_date_lr_lm_wald": [S.LR_all(bp), S.LM_all(bp), S.Wald_all(bp)],
            "sup_lm": [S.supLM_all(lo, hi)],
            "sup_lr_lm_wald": [S.supLR_all(lo, hi), S.supLM_all(lo, hi), S.supWald_all(lo, hi)]}
    boot = {}
    for name, stats in jobs.items():
        arr = D.api._stat_array(stats)
        width = int(ctx.lib.dfm_stats_width(model.handle, arr, len(stats)))
        out = torch.empty((B, width), dtype=torch.float64, device=dev)

        def run():
            ctx.check(ctx.lib.dfm_bootstrap_dev(model.handle, 0, B, di.data_ptr(), de.data_ptr(), arr, len(stats),
                                                out.data_ptr()))
        run()
        ctx.synchronize()
        ctx.reset_timing()
        ctx.enable_timing(True)
        sec = timed(run, max(args.reps, 5), ctx.synchronize)
        ctx.enable_timing(False)
        tm = ctx.read_timing()
        boot[name] = {"ms_per_job": round(sec * 1e3, 3),
                      "chow_kernels_ms_per_job": round(tm["chow"][0] / (max(args.reps, 5) + 1), 3)}
    med = lambda v: float(np.median(v))   # noqa: E731
    return {"config": "c2s", "workload": f"sup-Chow sweep, T={T} N={N} r={r}, dates {lo}..{hi} ({hi - lo + 1}), "
                                         "LR/LM/Wald with sup and arg-max (host buffers out)",
            "sweep_ms": round(med(ts) * 1e3, 4), "sweep_ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)],
            "chow_all_loop_ms": round(med(tl) * 1e3, 3),
            "chow_all_loop_ms_min_max": [round(min(tl) * 1e3, 3), round(max(tl) * 1e3, 3)],
            "value": round(med(tl) / med(ts), 1), "unit": "x (loop time / sweep time)",
            "sweep_kernels_ms": round(sweep_kernels_ms, 4), "sup_max_rel_diff_vs_loop": agree,
            "argsup_equal_loop": dates_equal, "bootstrap_B999": boot}


def mc(D, ctx, args):
    M, T, N, r, kmax = 1000, 100, 60, 3, 8
    xs = np.array([D.factor_model_DGP(T, N, r, rng=np.random.default_rng(20261019 + b))[1] for b in range(M)])
    y, w = np.zeros(T), np.ones((T, 1))
    lo, hi = D.sup_chow_range(T, r)
    sup = [D.Stat.supLM_all(lo, hi)]

    def batch_sel():
        return D.monte_carlo(xs, kmax=kmax, ctx=ctx)

    def batch_sup():
        return D.monte_carlo(xs, r, kmax=kmax, stats=sup, ctx=ctx)

    # the panels already resident in HBM in dfm_mc's layout: no host repack, no upload
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(xs.transpose(0, 2, 1))).to(torch.device("cuda", 0)).permute(0, 2, 1)

    def batch_sel_dev():
        return D.monte_carlo(xd, kmax=kmax, ctx=ctx)

    def batch_sup_dev():
        return D.monte_carlo(xd, r, kmax=kmax, stats=sup, ctx=ctx)

    def loop_sel():
        return [D.DynamicFactorModel(y, w, D.normalize(x, ctx=ctx), "ICp2", kmax=kmax, ctx=ctx) for x in xs]

    def loop_sup():
        out = []
        for x in xs:
            g = D.DynamicFactorModel(y, w, D.normalize(x, ctx=ctx), "ICp2", kmax=kmax, ctx=ctx)
            out.append((g.number_of_factors, D.chow_sweep(g, lo, hi, stats=["LM"]).sup["LM"]))
        return out
    # the same numbers: r^ of every panel, and the sup-LM rows of the panels the loop fitted at r
    a, b = batch_sel(), loop_sel()
    assert np.array_equal(a.criteria, batch_sel_dev().criteria)
    rhat_equal = bool(np.array_equal(a.rhat["ICp2"], [g.number_of_factors for g in b]))
    a2, b2 = batch_sup(), loop_sup()
    at_r = [i for i, (k, _) in enumerate(b2) if k == r]
    sup_diff = max(float(np.max(np.abs(a2.rows[i] - b2[i][1]) / np.abs(b2[i][1]))) for i in at_r)
    del b, b2
    # alternating, each call ending in a stream synchronise (host clock, uploads and read-backs in)
    reps = max(args.reps, 5)
    t = {"batch_sel": [], "loop_sel": [], "batch_sup": [], "loop_sup": [], "batch_sel_dev": [], "batch_sup_dev": []}
    for _ in range(reps):
        for name, fn, inner in (("batch_sel", batch_sel, 10), ("loop_sel", loop_sel, 1), ("batch_sup", batch_sup, 10),
                                ("loop_sup", loop_sup, 1), ("batch_sel_dev", batch_sel_dev, 10),
                                ("batch_sup_dev", batch_sup_dev, 10)):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            t[name].append((time.perf_counter() - t0) / inner)
    split = {}
    for name, fn in (("selection", batch_sel), ("sup_lm", batch_sup)):
        ctx.reset_timing()
        ctx.enable_timing(True)
        fn()
        ctx.enable_timing(False)
        split[name] = {k: [round(v[0], 4), int(v[1])] for k, v in ctx.read_timing().items() if v[1]}
    ms = lambda v: {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3),   # noqa: E731
                    "max": round(max(v) * 1e3, 3)}
    med = lambda k: float(np.median(t[k]))   # noqa: E731
    return {"config": "mc", "workload": f"Monte-Carlo batch M={M}, T={T} N={N} r={r}, kmax {kmax}: selection (all 7 "
                                        f"criteria), and + sup-LM of every variable over dates {lo}..{hi} at r={r}; "
                                        "host panels in, results out",
            "value": round(med("loop_sel") / med("batch_sel"), 1), "unit": "x (per-panel loop time / monte_carlo time)",
            "selection_ms": {"monte_carlo": ms(t["batch_sel"]), "loop": ms(t["loop_sel"]),
                             "monte_carlo_resident_input": ms(t["batch_sel_dev"])},
            "sup_lm_ms": {"monte_carlo": ms(t["batch_sup"]), "loop": ms(t["loop_sup"]),
                          "monte_carlo_resident_input": ms(t["batch_sup_dev"])},
            "sup_lm_ratio": round(med("loop_sup") / med("batch_sup"), 1),
            "kernel_ms_and_launches_by_class": split,
            "classes": "misc = layout + z-score (+ relocation lists), gram, eig_other = trace + spectrum, "
                       "stats = criterion sweep / arg-min (+ V etc.), eig_* / factors / chow = fit stage",
            "rhat_equal_loop": rhat_equal, "sup_lm_max_rel_diff_vs_loop": sup_diff, "panels_compared": len(at_r)}


def em_panel(D, T, N, r, seed):
    """A FRED-MD-like panel: r factors + noise, columns on their own scales; ~3 %
    missing at random, ragged last 1-3 rows on a third of the columns, late
    starters (first 24-240 rows missing) on a tenth — about 5 % missing in all."""
    rng = np.random.default_rng(seed)
    x = D.factor_model_DGP(T, N, r, rng=rng)[1]
    x = x * rng.uniform(0.5, 3.0, size=N) + rng.uniform(-2.0, 2.0, size=N)
    miss = rng.uniform(size=(T, N)) < 0.03
    for j in rng.choice(N, N // 3, replace=False):
        miss[T - int(rng.integers(1, 4)):, j] = True
    for j in rng.choice(N, N // 10, replace=False):
        miss[:int(rng.integers(T // 30, T // 3)), j] = True
    x[miss] = np.nan
    return x


def em(D, ctx, args):
    r = 8
    out = {"config": "em", "workload": f"EM fit with missing entries at r={r}, tol 1e-6: em_factors (device loop) vs the "
                                       "host loop (NumPy fill + normalize + principal_components per iteration, same "
                                       "iteration count); host panel in, completed panels / factors / loadings out",
           "unit": "x (host loop time / em_factors time)", "shapes": {}}
    for name, T, N in (("fred_md_like", 720, 128), ("c3_shape", 500, 2000)):
        x = em_panel(D, T, N, r, 20261020 + N)
        obs = ~np.isnan(x)
        res = D.em_factors(x, r, ctx=ctx)
        iters = res.iterations

        def device():
            return D.em_factors(x, r, ctx=ctx)

        def host_loop():
            x2 = np.where(obs, x, np.nanmean(x, axis=0))
            for it in range(iters + 1):
                mu, sd = x2.mean(axis=0), x2.std(axis=0, ddof=1)
                z = D.normalize(x2, ctx=ctx)
                ev, F, L, _ = D.principal_components(z, r, ctx=ctx)
                c = F @ L.T
                if it < iters:
                    x2 = np.where(obs, x, c * sd + mu)
            return z, c
        zl, cl = host_loop()
        cd = res.factors @ res.loadings.T
        agree = {"z_max_abs_diff": float(np.max(np.abs(zl - res.x_standardized))),
                 "common_rel_diff": float(np.linalg.norm(cl - cd) / np.linalg.norm(cd))}
        reps = max(args.reps, 5)
        td, th = [], []
        for _ in range(reps):   # alternating; every call ends in a stream synchronise (host clock)
            t0 = time.perf_counter()
            for _ in range(5):
                device()
            t1 = time.perf_counter()
            host_loop()
            t2 = time.perf_counter()
            td.append((t1 - t0) / 5)
            th.append(t2 - t1)
        ctx.reset_timing()
        ctx.enable_timing(True)
        device()
        ctx.enable_timing(False)
        split = {k: [round(v[0], 4), int(v[1])] for k, v in ctx.read_timing().items() if v[1]}
        ms = lambda v: {"median": round(float(np.median(v)) * 1e3, 3), "min": round(min(v) * 1e3, 3),   # noqa: E731
                        "max": round(max(v) * 1e3, 3)}
        out["shapes"][name] = {"T": T, "N": N, "missing_share": round(float((~obs).mean()), 4), "iterations": iters,
                               "converged": res.converged, "em_factors_ms": ms(td), "host_loop_ms": ms(th),
                               "ratio": round(float(np.median(th) / np.median(td)), 2),
                               "kernel_ms_and_launches_by_class": split, "agreement": agree}
    out["value"] = out["shapes"]["fred_md_like"]["ratio"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c2,c4,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time the CPU oracle (bounded samples)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--dump-maps", default="", help="copy /proc/self/maps here at interpreter exit (names the "
                                                      "libraries behind addresses in an exit-time stack trace)")
    args = ap.parse_args()
    if args.dump_maps:
        import atexit
        import shutil
        atexit.register(lambda: shutil.copyfile("/proc/self/maps", args.dump_maps))
    import torch  # noqa: F401  (before libdfm: one HIP runtime in the process, as bench.py)
    torch.cuda.init()
    import dfm_pkg
    D = dfm_pkg.load()
    ctx = D.Context(0)
    for name in args.configs.split(","):
        rec = globals()[name](D, ctx, args)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
