"""Monte-Carlo batches (dfm_mc / monte_carlo): M independent panels of one
shape — z-score, Gram, spectrum, the criterion sweep with its arg-mins and,
when statistics are asked for, the fit at each panel's r with the Chow tests —
in one pass, against

* the oracle's brute-force sweep (ic_sweep_values) and numpy's eigvalsh:
  criteria and eigenvalues 1e-10 relative, arg-mins exactly (over all panels of
  these inputs the smallest relative gap between the best and second-best k of
  any criterion is 2.9e-4, BIC at (50, 20): no tie exemption);
* the single fits the batch replaces (DynamicFactorModel, chow_all,
  chow_sweep, criterion_value): |a - b| <= max(1e-10 |b|, T 1e-14), the rule
  of tests/test_gpu_chow_sweep.py;
* itself: pre-normalised input, another chunk size, a strided layout and
  device-resident input give the same bits.

Shapes (T, N, r, kmax): both branches (T >= N: X'X, N > T: XX'), no dimension
a multiple of 16, Gram sizes 20 (Jacobi spectrum), 40 / 45 (tridiagonal +
bisection) and 90 (more than one 64 x 64 Gram tile).  At (50, 20, 2, 6) ICp3
selects every r in 2..6 across the 24 panels: the per-r^ grouping's input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(50, 20, 2, 6), (72, 45, 3, 8), (40, 70, 3, 8), (90, 130, 3, 8), (130, 90, 3, 8)]
M = 24
RTOL = 1e-10
NAMES = ("LR", "LM", "Wald")
_cache = {}


def raw(oracle, shape):
    """The shape's M raw panels (and their y)."""
    if ("raw", shape) not in _cache:
        T, N, r, _ = shape
        ys, xs = [], []
        for b in range(M):
            y, x, *_ = oracle.factor_model_DGP(T, N, r, np.random.default_rng(20261019 + 1000 * T + N + 7919 * b))
            ys.append(y)
            xs.append(x)
        _cache["raw", shape] = (ys, xs)
    return _cache["raw", shape]


def ref(oracle, shape):
    """The oracle's sweep of every panel: criteria (M, 7, kmax), arg-mins (M, 7), eigenvalues (M, kmax)."""
    if ("ref", shape) not in _cache:
        T, N, _, kmax = shape
        ys, xs = raw(oracle, shape)
        ic, ev = [], []
        for y, x in zip(ys, xs):
            xn = oracle.normalize(x)
            ic.append(oracle.ic_sweep_values(y, np.ones((T, 1)), xn, kmax))
            g = xn.T @ xn if T >= N else xn @ xn.T
            ev.append(np.linalg.eigvalsh(g)[::-1][:kmax])
        ic = np.array(ic)
        _cache["ref", shape] = (ic, ic.argmin(axis=2) + 1, np.array(ev))
    return _cache["ref", shape]


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.abs(b))


def near(a, b, T):
    """|a - b| <= max(1e-10 |b|, T 1e-14): the floor of a near-zero LR."""
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= np.maximum(RTOL * np.abs(b), T * 1e-14))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_selection_matches_oracle(dfm, oracle, shape):
    T, N, _, kmax = shape
    ic, rhat, ev = ref(oracle, shape)
    res = dfm.monte_carlo(raw(oracle, shape)[1], kmax=kmax, normalize=True)
    assert res.criteria.shape == (M, 7, kmax) and res.eigenvalues.shape == (M, kmax) and res.rows.shape == (M, 0)
    for c, name in enumerate(dfm.CRITERIA):
        assert np.array_equal(res.rhat[name], rhat[:, c]), (name, res.rhat[name], rhat[:, c])
    print(f"{shape}: criteria max rel err {np.max(np.abs(res.criteria - ic) / np.abs(ic)):.2e}, "
          f"eigenvalues {np.max(np.abs(res.eigenvalues - ev) / np.abs(ev)):.2e}")
    assert close(res.criteria, ic)
    assert close(res.eigenvalues, ev)
    assert np.array_equal(res.r, rhat[:, dfm.CRITERIA.index("ICp2")])


@pytest.mark.parametrize("shape", SHAPES)
def test_selection_matches_single_fits(dfm, oracle, shape):
    T, N, _, kmax = shape
    ys, xs = raw(oracle, shape)
    res = dfm.monte_carlo(xs, kmax=kmax)
    w = np.ones((T, 1))
    for crit in ("ICp2", "PCp1", "BIC"):
        c = dfm.CRITERIA.index(crit)
        for b in range(M):
            g = dfm.DynamicFactorModel(ys[b], w, oracle.normalize(xs[b]), crit, kmax=kmax)
            assert g.number_of_factors == res.rhat[crit][b], (crit, b)
            got = res.criteria[b, c, g.number_of_factors - 1]
            assert close(got, g.number_of_factors_criterion_value), (crit, b, got)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_normalize_is_the_existing_normalize(dfm, oracle, shape):
    T, N, r, kmax = shape
    xs = raw(oracle, shape)[1]
    S = dfm.Stat
    lo, hi = dfm.sup_chow_range(T, r)
    stats = [S.V(), S.criterion("PCp2"), S.LM_all(T // 2), S.supLM_all(lo, hi)]
    a = dfm.monte_carlo(xs, r, kmax=kmax, stats=stats, normalize=True)
    b = dfm.monte_carlo([dfm.normalize(x) for x in xs], r, kmax=kmax, stats=stats, normalize=False)
    assert same(a.criteria, b.criteria) and same(a.eigenvalues, b.eigenvalues) and same(a.rows, b.rows)
    assert np.all(np.isfinite(a.rows)) and a.rows.shape == (M, 2 + 2 * N)


def single_fit_rows(dfm, oracle, shape, rs, bp, lo, hi):
    """Per panel, the single fit at its r: V, the criteria, eigenvalue 1, trace, chow_all(bp), chow_sweep(lo..hi)."""
    key = ("single", shape, tuple(int(v) for v in rs), bp, lo, hi)
    if key not in _cache:
        T = shape[0]
        ys, xs = raw(oracle, shape)
        out = []
        for b in range(M):
            g = dfm.DynamicFactorModel(ys[b], np.ones((T, 1)), oracle.normalize(xs[b]), int(rs[b]))
            sw = dfm.chow_sweep(g, lo, hi)
            out.append(dict(V=dfm.factor_residual_variance(g), ICp2=dfm.criterion_value("ICp2", g),
                            PCp2=dfm.criterion_value("PCp2", g), ev1=g.eigenvalues[0], trace=g.trace_G,
                            chow=dfm.chow_all(g, bp), sup=[sw.sup[n] for n in NAMES]))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_stats_at_fixed_r_match_single_fits(dfm, oracle, shape):
    T, N, r, kmax = shape
    xs = raw(oracle, shape)[1]
    S = dfm.Stat
    bp = T // 2
    lo, hi = dfm.sup_chow_range(T, r)
    stats = [S.V(), S.criterion("ICp2"), S.criterion("PCp2"), S.eigenvalue(1), S.trace(), S.LR_all(bp), S.LM_all(bp),
             S.Wald_all(bp), S.LR(bp, 2), S.supLR_all(lo, hi), S.supLM_all(lo, hi), S.supWald_all(lo, hi)]
    res = dfm.monte_carlo(xs, r, kmax=kmax, stats=stats)
    assert res.rows.shape == (M, 6 + 6 * N) and np.all(res.r == r)
    want = single_fit_rows(dfm, oracle, shape, [r] * M, bp, lo, hi)
    for b in range(M):
        w = want[b]
        for st, key in zip(stats[:5], ("V", "ICp2", "PCp2", "ev1", "trace")):
            assert near(res.columns(st)[b], w[key], T), (b, key, res.columns(st)[b], w[key])
        for s in range(3):
            assert near(res.columns(stats[5 + s])[b], w["chow"][s], T), (b, NAMES[s])
            assert near(res.columns(stats[9 + s])[b], w["sup"][s], T), (b, "sup" + NAMES[s])
        assert near(res.columns(stats[8])[b], w["chow"][0][1], T), b   # LR(bp, variable 2)
    if shape == SHAPES[1]:   # the first panels against the oracle's own tests and their maxima over the range
        tests = (oracle.LR_test, oracle.LM_test, oracle.Wald_test)
        ys = raw(oracle, shape)[0]
        for b in range(4):
            o = oracle.DynamicFactorModel(ys[b], np.ones((T, 1)), oracle.normalize(xs[b]), r)
            cur = np.array([[[f(o, d, i) for i in range(N)] for d in range(lo, hi + 1)] for f in tests])
            for s in range(3):
                assert near(res.columns(stats[5 + s])[b], cur[s][bp - lo], T), (b, NAMES[s])
                assert near(res.columns(stats[9 + s])[b], cur[s].max(axis=0), T), (b, "sup" + NAMES[s])


def test_per_panel_rhat_groups(dfm, oracle):
    shape = SHAPES[0]
    T, N, _, kmax = shape
    xs = raw(oracle, shape)[1]
    rhat = ref(oracle, shape)[1][:, dfm.CRITERIA.index("ICp3")]
    assert len(set(rhat)) >= 3   # a silent single-group path cannot pass
    S = dfm.Stat
    bp = T // 2
    lo, hi = dfm.sup_chow_range(T, kmax)
    stats = [S.V(), S.LM_all(bp), S.supLM_all(lo, hi)]
    res = dfm.monte_carlo(xs, None, "ICp3", kmax=kmax, stats=stats)
    assert np.array_equal(res.r, rhat)
    want = single_fit_rows(dfm, oracle, shape, rhat, bp, lo, hi)
    for b in range(M):   # rows in panel order, each at its own r^
        assert near(res.columns(stats[0])[b], want[b]["V"], T), (b, rhat[b])
        assert near(res.columns(stats[1])[b], want[b]["chow"][1], T), (b, rhat[b])
        assert near(res.columns(stats[2])[b], want[b]["sup"][1], T), (b, rhat[b])


@pytest.mark.parametrize("shape,r,crit", [(SHAPES[1], 3, "ICp2"), (SHAPES[2], 3, "ICp2"), (SHAPES[1], None, "ICp3"),
                                          (SHAPES[2], None, "ICp3"), (SHAPES[0], None, "ICp3")])
def test_chunk_independence(dfm, oracle, shape, r, crit):
    T, N, _, kmax = shape
    xs = raw(oracle, shape)[1]
    S = dfm.Stat
    lo, hi = dfm.sup_chow_range(T, kmax)
    stats = [S.V(), S.criterion("PCp1"), S.LR_all(T // 2), S.Wald(T // 2, N), S.supLM_all(lo, hi),
             S.supWald_all(lo, hi)]
    a = dfm.monte_carlo(xs, r, crit, kmax=kmax, stats=stats, batch=5)   # 5 does not divide 24
    b = dfm.monte_carlo(xs, r, crit, kmax=kmax, stats=stats, batch=M)
    c = dfm.monte_carlo(xs, r, crit, kmax=kmax, stats=stats)
    for o in (b, c):
        assert same(a.rows, o.rows) and same(a.criteria, o.criteria) and same(a.eigenvalues, o.eigenvalues)
        assert all(np.array_equal(a.rhat[n], o.rhat[n]) for n in dfm.CRITERIA)
    assert np.all(np.isfinite(a.rows))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_layout_and_device_input(dfm, oracle, shape):
    import torch
    T, N, r, kmax = shape
    xs = np.array(raw(oracle, shape)[1])
    S = dfm.Stat
    lo, hi = dfm.sup_chow_range(T, kmax)
    stats = [S.V(), S.LM_all(T // 2), S.supLR_all(lo, hi)]
    packed = dfm.monte_carlo(xs, None, "ICp3", kmax=kmax, stats=stats)
    # ldx = T + 3, stride = ldx N + 5, NaN in every gap
    ldx, stride = T + 3, (T + 3) * N + 5
    buf = np.full(M * stride, np.nan)
    view = np.lib.stride_tricks.as_strided(buf, (M, T, N), (8 * stride, 8, 8 * ldx))
    view[...] = xs
    assert np.isnan(buf).sum() == M * stride - M * T * N
    for res in (dfm.monte_carlo(view, None, "ICp3", kmax=kmax, stats=stats),
                # device-resident: the packed layout, and the strided one
                dfm.monte_carlo(torch.from_numpy(np.ascontiguousarray(xs.transpose(0, 2, 1))).cuda().permute(0, 2, 1),
                                None, "ICp3", kmax=kmax, stats=stats),
                dfm.monte_carlo(torch.as_strided(torch.from_numpy(buf).cuda(), (M, T, N), (stride, 1, ldx)),
                                None, "ICp3", kmax=kmax, stats=stats)):
        assert same(res.rows, packed.rows) and same(res.criteria, packed.criteria)
        assert same(res.eigenvalues, packed.eigenvalues) and np.array_equal(res.r, packed.r)
    assert np.all(np.isfinite(packed.rows))


def test_arguments(dfm, oracle):
    shape = SHAPES[1]
    T, N, r, kmax = shape
    xs = np.array(raw(oracle, shape)[1])
    S = dfm.Stat
    for st in (S.coefficient(1), S.factors(), S.iterations(), S.t_stat(1), S.loadings()):
        with pytest.raises(dfm.DFMError) as e:
            dfm.monte_carlo(xs, r, stats=[st])
        assert e.value.code < 0

    def rejected(job, sentinel):
        """-7, a message, and no output row written (the C ABI directly)."""
        with pytest.raises(dfm.DFMError) as e:
            job()
        assert e.value.code == -7 and len(str(e.value).split(":", 1)[1].strip()) > 0
        assert np.all(sentinel == -99.0)

    ctx = dfm.default_context()
    xc = np.ascontiguousarray(xs.transpose(0, 2, 1))

    def call(rr, km, stats):
        arr = dfm.api._stat_array(stats)
        width = int(ctx.lib.dfm_mc_stats_width(N, arr, len(stats)))
        out = np.full((M, width), -99.0)
        rh = np.full((M, 7), -99, dtype=np.int64)
        spec = dfm._lib.dfm_mc_spec(rr, 4, km, 1, 0, 0)
        import ctypes as C
        return (lambda: ctx.check(ctx.lib.dfm_mc(ctx.h, C.c_void_p(xc.ctypes.data), M, T, N, T, T * N, C.byref(spec),
                                                 arr, len(stats), rh.ctypes.data_as(dfm._lib.c_int64_p), None, None,
                                                 dfm._lib.ptr(out))),
                np.concatenate([out.ravel(), rh.ravel().astype(float)]))
    # a break period outside r..T-r at a fixed r; outside kmax..T-kmax when r^ is per panel
    for rr, km, bad in [(r, kmax, r - 1), (r, kmax, T - r + 1), (0, kmax, kmax - 1), (0, kmax, T - kmax + 1)]:
        rejected(*call(rr, km, [S.LM_all(bad)]))
        rejected(*call(rr, km, [S.supLM_all(bad, bad) if bad < T // 2 else S.supLM_all(T // 2, bad)]))
    # the same dates are fine where the bound is the fixed r, not kmax
    ok = dfm.monte_carlo(xs, r, kmax=kmax, stats=[S.LM_all(kmax - 1)])
    assert np.all(np.isfinite(ok.rows))
    rejected(*call(17, kmax, [S.supLM_all(20, 40)]))            # the sweep's r <= 16
    assert np.all(np.isfinite(dfm.monte_carlo(xs[:2], 17, stats=[S.LM_all(30)]).rows))   # (single dates: any r <= 32)
    rejected(*call(r, kmax, [S.LM_all(30), S.LR_all(31)]))      # one break period per call
    # M = 0: empty arrays
    for empty in (xs[:0], []):
        res = dfm.monte_carlo(empty, kmax=kmax, stats=[S.V()])
        assert res.rows.shape == (0, 1) and res.r.shape == (0,) and res.criteria.shape[:2] == (0, 7)
        assert all(v.shape == (0,) for v in res.rhat.values())
    # the context still works
    assert np.array_equal(dfm.monte_carlo(xs[:3], kmax=kmax).rhat["ICp2"], ref(oracle, shape)[1][:3, 4])
