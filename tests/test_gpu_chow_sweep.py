"""sup-Chow tests (Breitung–Eickmeier 2011 with an unknown break date): LR / LM /
Wald of src/chowtest.jl:19-42 for every variable at every candidate break
period in one device pass (dfm_chow_sweep, DFM_STAT_SUP*_ALL), against

* the oracle's LR_test / LM_test / Wald_test maximised over the range, on the
  oracle's own fit and on its bootstrap replicates (1e-10 relative, arg-max
  dates equal: the smallest relative gap between the top two dates of any
  variable of these inputs is 5.9e-5, so no tie exemption);
* the single-date path dfm_chow_all at every date of the curve
  (|a - b| <= max(1e-10 |b|, T 1e-14), the floor of a near-zero LR).

Shapes (T, N, r, seed): no dimension a multiple of a tile; r = 1, 3 run the
4-wide kernels (four dates per thread in the Wald pass, eight in the LR / LM
pass), r = 5 the 8-wide, r = 10 the 16-wide;
(50, 70) is N > T (factored and direct bootstrap), the others T >= N."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(83, 13, 1, 1), (90, 21, 3, 2), (50, 70, 5, 3), (70, 24, 10, 4)]
NAMES = ("LR", "LM", "Wald")
RTOL = 1e-10
_cache = {}


def data(oracle, shape):
    if ("data", shape) not in _cache:
        T, N, r, seed = shape
        y, x, *_ = oracle.factor_model_DGP(T, N, r, np.random.default_rng(seed))
        _cache["data", shape] = (y, oracle.normalize(x), np.ones((T, 1)))
    return _cache["data", shape]


def oracle_tests(oracle):
    return (oracle.LR_test, oracle.LM_test, oracle.Wald_test)


def oracle_curves(oracle, d, lo, hi):
    """(3, hi - lo + 1, N): the oracle's three tests of fit d at every date and variable."""
    N = d.x.shape[1]
    return np.array([[[f(d, bp, i) for i in range(N)] for bp in range(lo, hi + 1)] for f in oracle_tests(oracle)])


def base(dfm, oracle, shape):
    """The shape's inputs, default range, oracle fit and oracle curves (computed once)."""
    if ("base", shape) not in _cache:
        T, N, r, _ = shape
        y, x, w = data(oracle, shape)
        lo, hi = dfm.sup_chow_range(T, r)
        o = oracle.DynamicFactorModel(y, w, x, r)
        _cache["base", shape] = (lo, hi, o, oracle_curves(oracle, o, lo, hi))
    return _cache["base", shape]


def fit(dfm, oracle, shape, ctx=None):
    y, x, w = data(oracle, shape)
    return dfm.DynamicFactorModel(y, w, x, shape[2], ctx=ctx)


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    return np.all(np.abs(a - b) <= rtol * np.abs(b))


@pytest.mark.parametrize("shape", SHAPES)
def test_sup_matches_oracle(dfm, oracle, shape):
    lo, hi, _, oc = base(dfm, oracle, shape)
    res = dfm.chow_sweep(fit(dfm, oracle, shape))
    assert (res.lo, res.hi) == (lo, hi) and res.curves is None
    for s, name in enumerate(NAMES):
        want = oc[s].max(axis=0)
        err = np.max(np.abs(res.sup[name] - want) / np.abs(want))
        print(f"{shape} sup-{name}: max rel err {err:.2e}")
        assert close(res.sup[name], want), (name, err)
        assert np.array_equal(res.argsup[name], lo + oc[s].argmax(axis=0)), name


@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_curves_match_single_date_path(dfm, oracle, shape, short):
    T = shape[0]
    lo, hi = dfm.sup_chow_range(T, shape[2])
    if short:   # fewer dates than one thread of the 4-wide kernels carries
        lo, hi = lo + 1, lo + 3
    g = fit(dfm, oracle, shape)
    res = dfm.chow_sweep(g, lo, hi, curves=True)
    assert (res.lo, res.hi) == (lo, hi)
    for name in NAMES:
        assert res.curves[name].shape == (hi - lo + 1, shape[1])
    for k, bp in enumerate(range(lo, hi + 1)):
        for name, b in zip(NAMES, dfm.chow_all(g, bp)):
            a = res.curves[name][k]
            bad = np.abs(a - b) > np.maximum(RTOL * np.abs(b), T * 1e-14)
            assert not bad.any(), (name, bp, a[bad], b[bad])
    for name in NAMES:
        c = res.curves[name]
        assert np.array_equal(res.sup[name], c.max(axis=0)), name
        assert np.array_equal(res.argsup[name], lo + c.argmax(axis=0)), name


def oracle_boot(oracle, shape, o, kind, idx, eta, lo, hi):
    """(B, 3 N): sup-LR | sup-LM | sup-Wald of every replicate by the oracle's own
    bootstrap loop, under a closure that maximises the oracle's tests over the range."""
    key = ("boot", shape, kind)
    if key not in _cache:
        rows = []

        def stat(d):
            rows.append(oracle_curves(oracle, d, lo, hi).max(axis=1).ravel())
            return 0.0
        if kind == "wild":
            oracle.wild_bootstrap(o, len(idx), stat, idx, eta)
        else:
            oracle.residual_bootstrap(o, len(idx), stat, idx)
        _cache[key] = np.array(rows)
    return _cache[key]


@pytest.mark.parametrize("kind", ["wild", "residual"])
@pytest.mark.parametrize("shape,mode", [(SHAPES[1], "auto"), (SHAPES[2], "direct"), (SHAPES[2], "factored")])
def test_bootstrap_sup_rows(dfm, oracle, shape, mode, kind):
    T, N, r, seed = shape
    lo, hi, o, _ = base(dfm, oracle, shape)
    B = 5
    idx, eta = oracle.draw_wild(np.random.default_rng(100 + seed), B, T)
    if kind == "residual":
        idx, eta = oracle.draw_residual(np.random.default_rng(200 + seed), B, T), None
    want = oracle_boot(oracle, shape, o, kind, idx, eta, lo, hi)
    g = fit(dfm, oracle, shape)
    g.set_bootstrap_mode(mode)
    S = dfm.Stat
    sups = [S.supLR_all(lo, hi), S.supLM_all(lo, hi), S.supWald_all(lo, hi)]

    def run(model, stats):
        if kind == "wild":
            return dfm.wild_bootstrap(model, B, stats, idx=idx, eta=eta)
        return dfm.residual_bootstrap(model, B, stats, idx=idx)
    got = run(g, sups)
    assert got.shape == (B, 3 * N)
    for s, name in enumerate(NAMES):
        a, b = got[:, s * N:(s + 1) * N], want[:, s * N:(s + 1) * N]
        err = np.max(np.abs(a - b) / np.abs(b))
        print(f"{shape} {mode} {kind} sup-{name}: max rel err {err:.2e}")
        assert close(a, b), (name, err)
    # batch-invariant to the bit, and over two models on one device
    for batch in (1, 2):
        g.set_batch(batch)
        assert np.array_equal(run(g, sups), got), batch
    g.set_batch(0)
    c = dfm.clone_model(g, dfm.Context(0))
    c.set_bootstrap_mode(mode)
    assert np.array_equal(run([g, c], sups), got)
    # beside a single-date stat: the same values as the two asked for separately
    bp0 = (lo + hi) // 2
    both = run(g, [S.supLM_all(lo, hi), S.LM_all(bp0)])
    assert np.array_equal(both[:, :N], run(g, S.supLM_all(lo, hi)))
    assert np.array_equal(both[:, :N], got[:, N:2 * N])
    assert np.array_equal(both[:, N:], run(g, S.LM_all(bp0)))


def chow_launches(ctx, job):
    ctx.reset_timing()
    ctx.enable_timing(True)
    try:
        job()
    finally:
        ctx.enable_timing(False)
    return ctx.read_timing()["chow"][1]


def test_sup_lm_alone_launches_no_wald_pass(dfm, oracle):
    """Every step of a sweep is one timed DFM_KC_CHOW launch (residuals, inverses, the
    LR / LM pass, the Wald pass, the reduction; one chunk of replicates here):
    asking for the sup-LM alone drops exactly the Wald pass."""
    shape = SHAPES[1]
    T, N, r, _ = shape
    ctx = dfm.Context(0)
    g = fit(dfm, oracle, shape, ctx=ctx)
    lo, hi = dfm.sup_chow_range(T, r)
    S = dfm.Stat
    B = 5
    idx, eta = oracle.draw_wild(np.random.default_rng(9), B, T)
    n_lm = chow_launches(ctx, lambda: dfm.wild_bootstrap(g, B, S.supLM_all(lo, hi), idx=idx, eta=eta))
    n_lr_lm = chow_launches(ctx, lambda: dfm.wild_bootstrap(g, B, [S.supLR_all(lo, hi), S.supLM_all(lo, hi)],
                                                            idx=idx, eta=eta))
    n_wald = chow_launches(ctx, lambda: dfm.wild_bootstrap(g, B, S.supWald_all(lo, hi), idx=idx, eta=eta))
    n_all = chow_launches(ctx, lambda: dfm.wild_bootstrap(
        g, B, [S.supLR_all(lo, hi), S.supLM_all(lo, hi), S.supWald_all(lo, hi)], idx=idx, eta=eta))
    assert (n_lm, n_lr_lm, n_wald, n_all) == (4, 4, 4, 5)
    # the fitted model: the LM curve and sup alone, against everything
    f_lm = chow_launches(ctx, lambda: dfm.chow_sweep(g, stats=["LM"], curves=True))
    f_all = chow_launches(ctx, lambda: dfm.chow_sweep(g, curves=True))
    assert (f_lm, f_all) == (4, 5)
    res = dfm.chow_sweep(g, stats=["LM"])
    assert list(res.sup) == ["LM"] and np.array_equal(res.sup["LM"], dfm.chow_sweep(g).sup["LM"])
    # the C ABI with only the LM curve pointer: one pass, no reduction, no Wald
    cur = np.zeros((hi - lo + 1, N))
    n_ptr = chow_launches(ctx, lambda: ctx.check(ctx.lib.dfm_chow_sweep(
        g.handle, lo, hi, 0, None, dfm._lib.ptr(cur), None, None, None)))
    assert n_ptr == 3
    assert np.array_equal(cur, dfm.chow_sweep(g, curves=True).curves["LM"])
    # rows of statistics left out: NaN / -1
    sup, arg = np.zeros((3, N)), np.zeros((3, N), dtype=np.int64)
    ctx.check(ctx.lib.dfm_chow_sweep(g.handle, lo, hi, 2, None, None, None, dfm._lib.ptr(sup),
                                     arg.ctypes.data_as(dfm._lib.c_int64_p)))
    assert np.all(np.isnan(sup[[0, 2]])) and np.all(arg[[0, 2]] == -1)
    assert np.array_equal(sup[1], res.sup["LM"]) and np.array_equal(arg[1], res.argsup["LM"])


def test_errors_leave_the_context_usable(dfm, oracle):
    shape = SHAPES[1]
    T, N, r, _ = shape
    y, x, w = data(oracle, shape)
    ctx = dfm.Context(0)
    g = fit(dfm, oracle, shape, ctx=ctx)
    lo, hi = dfm.sup_chow_range(T, r)
    S = dfm.Stat
    idx, eta = oracle.draw_wild(np.random.default_rng(3), 2, T)

    def rejected(job):
        with pytest.raises(dfm.DFMError) as e:
            job()
        assert e.value.code == -7
        assert len(str(e.value).split(":", 1)[1].strip()) > 0

    for a, b in [(hi, lo), (r - 1, hi), (lo, T - r + 1)]:
        rejected(lambda: dfm.chow_sweep(g, a, b))
        rejected(lambda: dfm.wild_bootstrap(g, 2, S.supLM_all(a, b), idx=idx, eta=eta))
    rejected(lambda: dfm.wild_bootstrap(g, 2, [S.supLM_all(lo, hi), S.supLR_all(lo, hi - 1)], idx=idx, eta=eta))
    gb = dfm.DynamicFactorModel(y, w, x, r, break_indices=[T // 2], ctx=ctx)
    rejected(lambda: dfm.chow_sweep(gb, lo, hi))
    rejected(lambda: dfm.wild_bootstrap(gb, 2, S.supLM_all(lo, hi), idx=idx, eta=eta))
    y2, x2, *_ = oracle.factor_model_DGP(60, 40, 17, np.random.default_rng(5))
    g17 = dfm.DynamicFactorModel(y2, np.ones((60, 1)), oracle.normalize(x2), 17, ctx=ctx)
    idx2, eta2 = oracle.draw_wild(np.random.default_rng(4), 2, 60)
    rejected(lambda: dfm.chow_sweep(g17, 20, 30))
    rejected(lambda: dfm.wild_bootstrap(g17, 2, S.supWald_all(20, 30), idx=idx2, eta=eta2))
    # the context and the models still work
    res = dfm.chow_sweep(g)
    assert np.all(np.isfinite(res.sup["LR"])) and np.all(res.sup["Wald"] > 0)
    out = dfm.wild_bootstrap(g, 2, S.supLM_all(lo, hi), idx=idx, eta=eta)
    assert out.shape == (2, N) and np.all(np.isfinite(out))
    assert np.all(np.isfinite(dfm.chow_all(g17, 25)[0]))
