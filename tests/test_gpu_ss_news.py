"""The news decomposition on the device (dfm_ss_news through nowcast_news)
against route (a) of tests/ss_news_reference.py, which conditions the joint
Gaussian densely and uses no Kalman recursion.

Shapes: the six ss_mf_reference.CASES (s = 1, odd s, s = 32, r = 16, two K
chunks of the collapse) and three plain panels (one at r = 16, p = 2, where
the lane kernel's LDS passes 64 KB and its staging registers are exactly
filled; 120 releases, so a second wave starts at a later row, 36), two
forecast rows.  Releases:
every second observed entry of the last six rows (J from 12 to 492: partial
waves, several waves, low-frequency releases), a release at row 0, one that is
the only observed entry of its row, one in the row that holds low-frequency
entries only; two old values are revised; and a J = 1 call.

Bars: every array within 1e-10 of the reference array's largest magnitude,
the bar of test_gpu_ss.py and test_gpu_ss_sim.py (the reference's two routes
agree to 1e-13, tests/test_ss_news_host.py).  What the header promises bit for
bit is checked bit for bit: the three smoothed paths, independence of the
pass, of t_lo and of what else is released, and repeatability."""
import numpy as np
import pytest

import ss_news_reference as R
import ss_sim_reference as SIM

pytestmark = pytest.mark.gpu

RTOL = 1e-10


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def report(label, fig):
    """Print every figure, then assert each against the bar."""
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < RTOL, (label, k, v)


def run(dfm, ctx, inp, **kw):
    Xo, Xn, L, sigma2, A, Q, low, w = inp
    kw.setdefault("targets", R.targets(Xo.shape[0], Xo.shape[1], low))
    kw.setdefault("horizon", R.HORIZON)
    return dfm.nowcast_news(Xo, Xn, L, sigma2, A, Q, low_freq=low, agg_weights=w, ctx=ctx, **kw)


def figures(res, ref, inp):
    L, low = inp[2], inp[6]
    r = ref["r"]
    fig = {k: big(getattr(res, k) - ref[k]) / big(ref[k]) for k in ("news", "release_forecast", "weights_f")}
    if ref["weights_agg"] is not None:
        fig["weights_agg"] = big(res.weights_agg - ref["weights_agg"]) / big(ref["weights_agg"])
    else:
        assert res.weights_agg is None
    old, rev, new, imp = R.target_values(ref, L, low, res.targets)
    fig["old"], fig["revised"], fig["new"] = (big(a - b) / big(b) for a, b in
                                               ((res.old, old), (res.revised, rev), (res.new, new)))
    fig["impacts"] = big(res.impacts - imp) / big(imp)
    # the identity on the device's own numbers: every row, the forecast rows included
    move = res.smoothed_new - res.smoothed_revised
    fig["identity"] = big(move - np.einsum("j,jtk->tk", res.news, res.weights_f)) / big(res.smoothed_new)
    if res.weights_agg is not None:
        amove = res.smoothed_agg_new - res.smoothed_agg_revised
        fig["identity_agg"] = big(amove - np.einsum("j,jtk->tk", res.news, res.weights_agg)) / big(res.smoothed_agg_new)
    fig["targets"] = big(res.new - res.revised - res.impacts.sum(axis=1)) / big(res.new)
    fig["smoothed_new"] = big(res.smoothed_new - ref["state_new"][:, :r]) / big(ref["state_new"][:, :r])
    return fig


# -------------------------------------------------------------------- parity
@pytest.mark.parametrize("i", range(R.N_CASES), ids=R.CASE_IDS)
def test_parity_with_the_joint_gaussian(dfm, ctx, i):
    inp, ref = R.case(i)
    res = run(dfm, ctx, inp)
    J = len(ref["releases"])
    assert np.array_equal(res.releases, ref["releases"]) and J >= 9
    assert res.weights_f.shape == (J, inp[0].shape[0] + R.HORIZON, ref["r"])
    rows = set(res.releases[:, 0].tolist())
    assert 0 in rows and (inp[6] is None or 5 in rows)
    report(f"news {R.CASE_IDS[i]} J={J}", figures(res, ref, inp))
    by = np.zeros_like(res.by_series)
    for j, (_, s) in enumerate(res.releases):
        by[:, s] += res.impacts[:, j]
    assert big(res.by_series - by) <= 1e-15 * big(res.impacts) * J
    assert big(res.revision_effect - (res.revised - res.old)) == 0.0 and big(res.revision_effect) > 0.0


@pytest.mark.parametrize("i", (0, R.N_CASES - 1), ids=("mixed", "plain"))
def test_a_single_release(dfm, ctx, i):
    inp, ref = R.case(i, True)
    res = run(dfm, ctx, inp)
    assert res.releases.tolist() == ref["releases"].tolist() and len(res.news) == 1
    report(f"single {R.CASE_IDS[i]}", figures(res, ref, inp))


def test_standardised_vintages_report_original_units(dfm, ctx):
    """mean / std: the model sees (x - mean) / std; the targets come back in x's units."""
    inp, ref = R.case(1)
    Xo, Xn, L, sigma2, A, Q, low, w = inp
    rng = np.random.default_rng(5)
    mu, sd = rng.uniform(-2.0, 2.0, size=Xo.shape[1]), rng.uniform(0.5, 3.0, size=Xo.shape[1])
    res = run(dfm, ctx, (Xo * sd + mu, Xn * sd + mu) + inp[2:], mean=mu, std=sd)
    old, rev, new, imp = R.target_values(ref, L, low, res.targets)
    k = res.targets[:, 1]
    report("standardised", {"news": big(res.news - ref["news"]) / big(ref["news"]),
                            "new": big(res.new - (new * sd[k] + mu[k])) / big(new * sd[k] + mu[k]),
                            "revised": big(res.revised - (rev * sd[k] + mu[k])) / big(rev * sd[k] + mu[k]),
                            "impacts": big(res.impacts - imp * sd[k][:, None]) / big(imp * sd[k][:, None]),
                            "targets": big(res.new - res.revised - res.impacts.sum(axis=1)) / big(res.new)})


# --------------------------------------------------------------- bit for bit
@pytest.fixture(scope="module")
def base(dfm, ctx):
    """70 x 300 with 492 releases (eight waves, the last partial) and the
    plain 60 x 40, r = 5, p = 3 with 65."""
    return {i: (R.case(i)[0], run(dfm, ctx, R.case(i)[0])) for i in (5, R.N_CASES - 1)}


@pytest.mark.parametrize("i", (5, R.N_CASES - 1), ids=("mixed", "plain"))
def test_smoothed_paths_are_kalman_smoothers(dfm, ctx, base, i):
    inp, res = base[i]
    Xo, Xn, L, sigma2, A, Q, low, w = inp
    for X, sm, agg in ((Xo, res.smoothed_old, res.smoothed_agg_old),
                       (R.revised(Xo, Xn), res.smoothed_revised, res.smoothed_agg_revised),
                       (Xn, res.smoothed_new, res.smoothed_agg_new)):
        ks = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=R.HORIZON, low_freq=low, agg_weights=w, ctx=ctx)
        assert np.array_equal(sm, ks.smoothed)
        assert (agg is None and ks.smoothed_agg is None) or np.array_equal(agg, ks.smoothed_agg)


FIELDS = ("news", "release_forecast", "weights_f", "weights_agg", "impacts", "smoothed_new", "new")


def same(a, b, fields=FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None) or np.array_equal(x, y), f


@pytest.mark.parametrize("i", (5, R.N_CASES - 1), ids=("mixed", "plain"))
def test_pass_size_and_repeats_change_nothing(dfm, ctx, base, i):
    inp, res = base[i]
    same(run(dfm, ctx, inp, pass_releases=64), res)   # 492 = 7 x 64 + 44; 65 = 64 + 1
    same(run(dfm, ctx, inp), res)


@pytest.mark.parametrize("i", (5, R.N_CASES - 1), ids=("mixed", "plain"))
def test_t_lo_is_a_slice(dfm, ctx, base, i):
    inp, res = base[i]
    T = inp[0].shape[0]
    tg = res.targets[res.targets[:, 0] >= 5]
    lo = run(dfm, ctx, inp, t_lo=5, targets=tg)
    assert lo.weights_f.shape[1] == T + R.HORIZON - 5 and np.array_equal(lo.weights_f, res.weights_f[:, 5:])
    assert (res.weights_agg is None and lo.weights_agg is None) or np.array_equal(lo.weights_agg, res.weights_agg[:, 5:])
    assert np.array_equal(lo.news, res.news) and np.array_equal(lo.smoothed_new, res.smoothed_new)
    last = run(dfm, ctx, inp, t_lo=T + R.HORIZON - 1, targets=tg[-1:])   # the backward loop does not run
    assert np.array_equal(last.weights_f, res.weights_f[:, -1:])


@pytest.mark.parametrize("i", (5, R.N_CASES - 1), ids=("mixed", "plain"))
def test_weights_depend_on_the_new_mask_only(dfm, ctx, base, i):
    """Every third release moves into X_old with X_new's value: the others
    keep their weights, now at other lanes of other waves."""
    inp, res = base[i]
    Xo = inp[0].copy()
    J = len(res.releases)
    moved = np.arange(J) % 3 == 1
    for t, s in res.releases[moved]:
        Xo[t, s] = inp[1][t, s]
    sub = run(dfm, ctx, (Xo,) + inp[1:])
    assert np.array_equal(sub.releases, res.releases[~moved])
    assert np.array_equal(sub.weights_f, res.weights_f[~moved])
    assert (res.weights_agg is None) or np.array_equal(sub.weights_agg, res.weights_agg[~moved])
    assert np.array_equal(sub.smoothed_new, res.smoothed_new)


def test_simulation_smoother_repeats_beside_the_news(dfm, ctx):
    """The two features run one gain kernel, one lane core and one pass driver
    (dfm_ss_lane.h / .hip).  The simulation smoother's own suite pins its
    values; this guards that in a process that has run the news on the same
    context (its records, its constants, its raised LDS cap) the draws still
    repeat whatever the pass."""
    X, L, sigma2, A, Q, a0, _, _ = SIM.moment_case(*SIM.GPU_SHAPES[0])
    T, N, r, p, h = SIM.GPU_SHAPES[0]
    z = np.random.default_rng(1).standard_normal((70, SIM.nz(T + h, r, r * p)))
    a = dfm.simulation_smoother(X, L, sigma2, A, Q, draws=70, z=z, a0=a0, horizon=h, ctx=ctx)
    b = dfm.simulation_smoother(X, L, sigma2, A, Q, draws=70, z=z, a0=a0, horizon=h, pass_draws=64, ctx=ctx)
    assert np.array_equal(a.draws, b.draws) and np.isfinite(a.draws).all()


def _smallest_sim_shape():
    X, L, sigma2, A, Q, a0, _, _ = SIM.moment_case(*SIM.GPU_SHAPES[0])   # 9 x 7: a one-entry row, an empty row
    return X, L, sigma2, A, Q, a0, SIM.GPU_SHAPES[0][4]


def _smallest_mixed_case():
    _, Xn, L, sigma2, A, Q, _, _ = R.inputs(4)   # 30 x 6
    return Xn, L, sigma2, A, Q, None, R.HORIZON


@pytest.mark.parametrize("make", (_smallest_sim_shape, _smallest_mixed_case), ids=("sim9x7", "mixed30x6"))
def test_both_features_take_over_the_same_smoother(dfm, ctx, make):
    """Both features start from the same smoother's launches, which the shared
    driver takes over.  This checks the smoothed paths only, which exist
    before the driver runs; the gain record itself is checked by the parity
    tests of both suites.  On the same parameters and the same (new-vintage)
    panel the simulation smoother's smoothed path, the news' smoothed_new and
    kalman_smoother's are the same bits, and both features' own outputs are
    finite.  The simulation smoother has no mixed-frequency model, so on
    the mixed case's parameters and panel the three run the plain model, and
    the mixed model's hand-over is the news' against kalman_smoother's."""
    Xn, L, sigma2, A, Q, a0, h = make()
    T, N = Xn.shape
    r, s = np.atleast_2d(L).shape[1], np.atleast_2d(A).shape[1]
    Xo = Xn.copy()
    seen = np.argwhere(~np.isnan(Xn))
    for t, i in seen[seen[:, 0] >= T - 2][::2]:   # releases on the ragged edge ...
        Xo[t, i] = np.nan
    t1, i1 = seen[seen[:, 0] > 0][0]              # ... and the first observed entry after row 0
    Xo[t1, i1] = np.nan
    tg = np.array([(T - 1, 0), (T + h - 1, N - 1)], dtype=np.int64)
    ks = dfm.kalman_smoother(Xn, L, sigma2, A, Q, a0=a0, horizon=h, ctx=ctx)
    sim = dfm.simulation_smoother(Xn, L, sigma2, A, Q, draws=2, z=np.zeros((2, SIM.nz(T + h, r, s))), a0=a0, horizon=h,
                                  ctx=ctx)
    news = dfm.nowcast_news(Xo, Xn, L, sigma2, A, Q, targets=tg, a0=a0, horizon=h, ctx=ctx)
    assert len(news.releases) >= 2 and np.isfinite(sim.draws).all() and np.isfinite(news.weights_f).all()
    assert np.array_equal(sim.smoothed, ks.smoothed) and np.array_equal(news.smoothed_new, ks.smoothed)
    assert np.array_equal(sim.smoothed, news.smoothed_new)
    if make is _smallest_mixed_case:
        low, w = R.inputs(4)[6:]
        ksm = dfm.kalman_smoother(Xn, L, sigma2, A, Q, horizon=h, low_freq=low, agg_weights=w, ctx=ctx)
        mixed = dfm.nowcast_news(Xo, Xn, L, sigma2, A, Q, targets=tg, horizon=h, low_freq=low, agg_weights=w, ctx=ctx)
        assert np.array_equal(mixed.smoothed_new, ksm.smoothed) and np.array_equal(mixed.smoothed_agg_new, ksm.smoothed_agg)


# ------------------------------------------------------------------ refusals
def test_no_release_is_valid(dfm, ctx):
    inp, _ = R.case(0)
    Xn = inp[1]
    Xo = Xn.copy()
    t, k = np.argwhere(~np.isnan(Xn))[7]
    Xo[t, k] += 0.5   # a revision alone
    res = run(dfm, ctx, (Xo,) + inp[1:])
    assert res.releases.shape == (0, 2) and res.weights_f.shape[0] == 0 and res.impacts.shape[1] == 0
    ks = dfm.kalman_smoother(Xo, *inp[2:6], horizon=R.HORIZON, low_freq=inp[6], agg_weights=inp[7], ctx=ctx)
    assert np.array_equal(res.smoothed_old, ks.smoothed) and np.array_equal(res.smoothed_revised, res.smoothed_new)
    assert big(res.new - res.revised) == 0.0 and big(res.revision_effect) > 0.0


def test_refusals(dfm, ctx, base):
    inp, good = base[R.N_CASES - 1]
    rel = good.releases

    def refused(word, entry, Xo=inp[0], **kw):
        with pytest.raises(dfm.DFMError) as e:
            run(dfm, ctx, (Xo,) + inp[1:], **kw)
        assert e.value.code == -2 and word in str(e.value), str(e.value)
        assert f"(t = {entry[0]}, i = {entry[1]})" in str(e.value), str(e.value)

    swapped = rel.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    refused("sorted", rel[3], releases=swapped)
    refused("twice", rel[7], releases=np.vstack([rel[:8], rel[7:]]))
    refused("leaves out", rel[10], releases=np.delete(rel, 10, axis=0))
    both = np.argwhere(~np.isnan(inp[0]))[5]
    extra = np.vstack([rel, both[None]])
    refused("no release", both, releases=extra[np.lexsort((extra[:, 1], extra[:, 0]))])
    refused("outside", (inp[0].shape[0], 0), releases=np.vstack([rel, [[inp[0].shape[0], 0]]]))
    Xd = inp[0].copy()
    gone = np.argwhere(np.isnan(inp[1]))[0]
    Xd[gone[0], gone[1]] = 1.0   # observed in the old vintage only
    refused("old observed set", gone, Xo=Xd)
    for bad in (dict(t_lo=inp[0].shape[0] + R.HORIZON), dict(horizon=-1)):
        with pytest.raises((dfm.DFMError, ValueError)):
            run(dfm, ctx, inp, **bad)
    same(run(dfm, ctx, inp), good)   # the context still serves a good call
