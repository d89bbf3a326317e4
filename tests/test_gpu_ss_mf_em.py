"""The mixed-frequency quasi-ML EM on the device (dfm_ss_em_mf through
ss_em(low_freq=, agg_weights=)) against tests/ss_mf_reference.py: the dense
filter, ss_em_reference's lag-one covariances and the restricted M-step solved
with numpy.linalg.solve.

Bars as tests/test_gpu_ss_em.py: every parameter and output within 1e-10 of
the reference array's largest magnitude after 4-5 M-steps at tol = 0 from a
perturbed start, every log-likelihood of the path 1e-10 relative, the path
strictly increasing.  The reference's path rises on every case (smallest gain
0.16); its stopping times of the batch have margins |c_j - tol| / tol >= 0.028,
far above the bar, so they are reproduced exactly."""
import numpy as np
import pytest

import ss_mf_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
IDS = R.CASE_IDS + ["270x8r2p1w3"]
PARAMS = ("loadings", "sigma2", "A", "Q", "a0", "P0")
OUTPUTS = ("filtered", "smoothed", "smoothed_cov", "smoothed_agg")
REF = dict(loadings="L")
ALL = PARAMS + OUTPUTS + ("loglik", "n_observed", "loglik_path", "iterations", "converged", "criterion")


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def figures(res, ref):
    # an all-zero reference array (a0 left at the start's zero) must be met exactly
    fig = {k: big(getattr(res, k) - ref[REF.get(k, k)]) / (big(ref[REF.get(k, k)]) or 1.0) for k in PARAMS + OUTPUTS}
    n = len(ref["path"])
    fig["path"] = float(np.max(np.abs(res.loglik_path[:n] - ref["path"]) / np.abs(ref["path"])))
    return fig


def report(label, fig, bar):
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < bar, (label, k, v)


def same(a, b):
    for f in ALL:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


def iters(i):
    return 4 if i in (3, 5) else 5


@pytest.mark.parametrize("i", range(len(IDS)), ids=IDS)
def test_em_parity(dfm, ctx, i):
    X, start, low, w, ref = R.em_case(i, iters(i))
    res = dfm.ss_em(X, *start, tol=0.0, max_iter=iters(i), horizon=2, low_freq=low, agg_weights=w, ctx=ctx)
    assert res.iterations == ref["iterations"] == iters(i) and not res.converged
    assert res.n_observed == ref["nobs"] and res.loglik == res.loglik_path[-1]
    assert res.A.shape == ref["A"].shape and res.P0.shape == ref["P0"].shape
    assert (np.diff(res.loglik_path) > 0).all()
    report(f"em {IDS[i]}", figures(res, ref), RTOL)


def test_em_without_update_init(dfm, ctx):
    X, L, sigma2, A, Q, low = R.make_case(*R.CASES[1])
    w = R.CASES[1][4]
    start = R.perturbed_start(L, sigma2, A, Q)
    ref = R.em(X, *start, low, w, tol=0.0, max_iter=3, update_init=False)
    res = dfm.ss_em(X, *start, tol=0.0, max_iter=3, update_init=False, low_freq=low, agg_weights=w, ctx=ctx)
    report("no update_init", figures(res, ref), RTOL)


def test_batch_stopping_times_and_single_calls(dfm, ctx):
    cases = [R.em_batch_case(k) for k in range(6)]
    low, w = cases[0][2], cases[0][3]
    panels = np.stack([c[0] for c in cases])
    starts = [np.stack([c[1][j] for c in cases]) for j in range(4)]
    kw = dict(tol=R.BATCH_TOL, max_iter=40, low_freq=low, agg_weights=w, ctx=ctx)
    res = dfm.ss_em(panels, *starts, **kw)
    want = [c[4]["iterations"] for c in cases]
    print("stopping times", res.iterations.tolist(), "reference", want)
    assert res.iterations.tolist() == want and res.converged.all() and len(set(want)) > 1
    for k, c in enumerate(cases):
        one = dfm.ss_em(c[0], *c[1], **kw)
        for f in ALL:
            assert np.array_equal(getattr(res, f)[k], getattr(one, f), equal_nan=True), (k, f)
        report(f"batch panel {k}", figures(one, c[4]), RTOL)


def test_repeat_device_input_and_horizon(dfm, ctx):
    import torch
    X, start, low, w, _ = R.em_case(1)
    kw = dict(tol=0.0, max_iter=3, low_freq=low, agg_weights=w, ctx=ctx)
    a = dfm.ss_em(X, *start, horizon=2, **kw)
    same(a, dfm.ss_em(X, *start, horizon=2, **kw))
    xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    same(a, dfm.ss_em(xd, *start, horizon=2, **kw))
    app = dfm.ss_em(np.vstack([X, np.full((2, X.shape[1]), np.nan)]), *start, **kw)
    # appended rows are sample rows to the M-step's transition sums, so only the first E-step is comparable
    h0 = dfm.ss_em(X, *start, horizon=2, tol=0.0, max_iter=0, low_freq=low, agg_weights=w, ctx=ctx)
    a0 = dfm.ss_em(np.vstack([X, np.full((2, X.shape[1]), np.nan)]), *start, tol=0.0, max_iter=0, low_freq=low,
                   agg_weights=w, ctx=ctx)
    for f in ("smoothed", "smoothed_cov", "smoothed_agg", "loglik"):
        assert np.array_equal(getattr(h0, f), getattr(a0, f)), f
    assert np.isfinite(app.loglik)


def test_no_low_series_is_the_plain_em(dfm, ctx):
    X, start, low, w, _ = R.em_case(1)
    plain = dfm.ss_em(X, *start, tol=0.0, max_iter=3, horizon=1, ctx=ctx)
    none = dfm.ss_em(X, *start, tol=0.0, max_iter=3, horizon=1, low_freq=np.zeros_like(low), agg_weights=w, ctx=ctx)
    for f in ALL:
        if f != "smoothed_agg":
            assert np.array_equal(getattr(plain, f), getattr(none, f), equal_nan=True), f
    assert none.smoothed_agg is None


def test_unit_weight_is_the_plain_em(dfm, ctx):
    X, start, low, _, _ = R.em_case(1)
    plain = dfm.ss_em(X, *start, tol=0.0, max_iter=4, ctx=ctx)
    one = dfm.ss_em(X, *start, tol=0.0, max_iter=4, low_freq=low, agg_weights=(1.0,), ctx=ctx)
    ref = {k: getattr(plain, k) for k in PARAMS + OUTPUTS[:3]}
    ref.update(L=plain.loadings, smoothed_agg=plain.smoothed, path=plain.loglik_path)
    report("unit weight", figures(one, ref), RTOL)


def test_errors(dfm, ctx):
    X, start, low, w, _ = R.em_case(0)
    L, sigma2, A, Q = start
    rng = np.random.default_rng(5)
    with pytest.raises(dfm.DFMError) as e:   # r = 8, n_w = 5
        dfm.ss_em(X, rng.standard_normal((10, 8)), sigma2, 0.5 * np.eye(8), np.eye(8), low_freq=low,
                  agg_weights=R.AGG_FLOW, ctx=ctx)
    assert e.value.code == -7
    for bad in ((1.0, np.nan), (0.0, 1.0)):
        with pytest.raises(dfm.DFMError) as e:
            dfm.ss_em(X, *start, low_freq=low, agg_weights=bad, ctx=ctx)
        assert e.value.code == -2
    with pytest.raises(dfm.DFMError) as e:
        dfm.ss_em(X, *start, low_freq=low[:-1], agg_weights=w, ctx=ctx)
    assert e.value.code == -2
    Xe = X.copy()
    Xe[:, 8] = np.nan
    with pytest.raises(dfm.DFMError) as e:   # an empty column is named before the first pass
        dfm.ss_em(Xe, *start, low_freq=low, agg_weights=w, ctx=ctx)
    assert e.value.code == -2 and "column 8" in str(e.value)
    assert np.isfinite(dfm.ss_em(X, *start, max_iter=1, low_freq=low, agg_weights=w, ctx=ctx).loglik)
