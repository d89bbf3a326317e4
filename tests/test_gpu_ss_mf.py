"""The mixed-frequency smoother on the device (dfm_ss_smooth_mf through
kalman_smoother(low_freq=, agg_weights=)) against tests/ss_mf_reference.py,
whose reference filter is the textbook one on explicit N x s loading rows.

Bars: loglik 1e-10 relative, every array within 1e-10 of the reference
array's largest magnitude (the project's fp64 bar); the reference's two
arrangements agree to 5e-14, and every case's reference outputs move by less
than 1e-11 when its inputs are perturbed by 1e-12 (both asserted in
tests/test_ss_mf_host.py).  Repeated runs, device input, horizon against appended rows, batch
against single calls and an all-False mask against the plain call are bit for
bit."""
import numpy as np
import pytest

import ss_mf_reference as R
import ss_reference as S

pytestmark = pytest.mark.gpu

RTOL = 1e-10
FIELDS = ("filtered", "smoothed", "smoothed_cov", "smoothed_agg", "loglik", "n_observed")


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def figures(res, ref):
    fig = {"loglik": abs(res.loglik - ref["loglik"]) / abs(ref["loglik"])}
    for k in ("filtered", "smoothed", "smoothed_cov", "smoothed_agg"):
        fig[k] = big(getattr(res, k) - ref[k]) / big(ref[k])
    return fig


def report(label, fig, bar):
    """Print every figure, then assert each against its bar."""
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < bar, (label, k, v)


def same(a, b, fields=FIELDS):
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


# -------------------------------------------------------------------- parity
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_smoother_parity(dfm, ctx, i):
    """P0 is left to the library: the doubling iteration at the padded
    companion form against the Kronecker solve."""
    X, L, sigma2, A, Q, low, w, ref = R.case(i)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, low_freq=low, agg_weights=w, ctx=ctx)
    assert res.n_observed == ref["nobs"] == int((~np.isnan(X)).sum())
    for k in ("filtered", "smoothed", "smoothed_cov", "smoothed_agg"):
        assert getattr(res, k).shape == ref[k].shape, k
    report(f"parity {R.CASE_IDS[i]}", figures(res, ref), RTOL)


def test_smoother_with_a0_and_horizon(dfm, ctx):
    """A caller's a0 and P0 at the padded state (s = 10 for r = 2, p = 1, five weights)."""
    X, L, sigma2, A, Q, low, w, _ = R.case(0)
    s = 10
    a0 = np.linspace(-1.0, 1.0, s)
    P0 = 2.0 * np.eye(s) + 0.5
    ref = R.smooth(X, L, sigma2, A, Q, low, w, a0, P0, horizon=3)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, a0=a0, P0=P0, horizon=3, low_freq=low, agg_weights=w, ctx=ctx)
    report("a0/P0", figures(res, ref), RTOL)
    with pytest.raises(ValueError):   # a0 of the unpadded state
        dfm.kalman_smoother(X, L, sigma2, A, Q, a0=a0[:2], low_freq=low, agg_weights=w, ctx=ctx)


# -------------------------------------------------------------- bit-identity
def test_repeat_device_input_horizon_and_batch(dfm, ctx):
    import torch
    T, N, r, p, w = R.CASES[1]
    X0, L, sigma2, A, Q, low = R.make_case(T, N, r, p, w)
    X1 = R.make_case(T, N, r, p, w, seed=1)[0]
    X2 = X0.copy()
    X2[:, low] = np.nan            # a panel whose low-frequency class is never observed
    panels = np.stack([X0, X1, X2])
    kw = dict(low_freq=low, agg_weights=w, ctx=ctx)
    a = dfm.kalman_smoother(panels, L, sigma2, A, Q, horizon=2, **kw)
    b = dfm.kalman_smoother(panels, L, sigma2, A, Q, horizon=2, **kw)
    xd = torch.from_numpy(np.ascontiguousarray(panels.transpose(0, 2, 1))).cuda().transpose(1, 2)
    d = dfm.kalman_smoother(xd, L, sigma2, A, Q, horizon=2, **kw)
    same(a, b)
    same(a, d)
    assert a.smoothed_agg.shape == (3, T + 2, r)
    for k in range(3):
        one = dfm.kalman_smoother(panels[k], L, sigma2, A, Q, horizon=2, **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(a, f)[k], getattr(one, f)), (k, f)
        report(f"batch panel {k}", figures(one, R.smooth(panels[k], L, sigma2, A, Q, low, w, horizon=2)), RTOL)
    app = dfm.kalman_smoother(np.vstack([X0, np.full((2, N), np.nan)]), L, sigma2, A, Q, **kw)
    for f in ("smoothed", "smoothed_cov", "smoothed_agg"):
        assert np.array_equal(getattr(a, f)[0], getattr(app, f)), f
    assert np.array_equal(a.filtered[0], app.filtered[:T]) and a.loglik[0] == app.loglik


def test_no_low_series_is_the_plain_call(dfm, ctx):
    X, L, sigma2, A, Q, low, w, _ = R.case(1)
    plain = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=2, ctx=ctx)
    none = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=2, low_freq=np.zeros_like(low), agg_weights=w, ctx=ctx)
    same(plain, none, FIELDS[:3] + FIELDS[4:])
    assert none.smoothed_agg is None and plain.smoothed_agg is None


def test_unit_weight_is_the_plain_model(dfm, ctx):
    """agg_weights = (1,): any mask gives the plain model, by the two-update route."""
    X, L, sigma2, A, Q, low, _, _ = R.case(1)
    plain = dfm.kalman_smoother(X, L, sigma2, A, Q, ctx=ctx)
    mask = low.copy()
    mask[::2] = True
    one = dfm.kalman_smoother(X, L, sigma2, A, Q, low_freq=mask, agg_weights=(1.0,), ctx=ctx)
    ref = dict(loglik=plain.loglik, filtered=plain.filtered, smoothed=plain.smoothed, smoothed_cov=plain.smoothed_cov,
               smoothed_agg=plain.smoothed)
    assert one.n_observed == plain.n_observed
    report("unit weight", figures(one, ref), RTOL)


# -------------------------------------------------------------------- errors
def test_errors(dfm, ctx):
    X, L, sigma2, A, Q, low, w, _ = R.case(0)
    kw = dict(low_freq=low, ctx=ctx)
    rng = np.random.default_rng(5)
    with pytest.raises(dfm.DFMError) as e:   # r = 8, n_w = 5: s = 40
        dfm.kalman_smoother(X, rng.standard_normal((10, 8)), sigma2, 0.5 * np.eye(8), np.eye(8), agg_weights=R.AGG_FLOW,
                            **kw)
    assert e.value.code == -7
    with pytest.raises(dfm.DFMError) as e:   # nine weights
        dfm.kalman_smoother(X, L, sigma2, A, Q, agg_weights=np.ones(9), **kw)
    assert e.value.code == -7
    for bad in ((1.0, np.nan, 1.0), (0.0, 1.0), (np.inf,)):
        with pytest.raises(dfm.DFMError) as e:
            dfm.kalman_smoother(X, L, sigma2, A, Q, agg_weights=bad, **kw)
        assert e.value.code == -2, bad
    with pytest.raises(dfm.DFMError) as e:
        dfm.kalman_smoother(X, L, sigma2, A, Q, low_freq=low[:-1], agg_weights=w, ctx=ctx)
    assert e.value.code == -2
    sz = sigma2.copy()
    sz[9] = 0.0
    with pytest.raises(dfm.DFMError) as e:   # the plain checks still hold
        dfm.kalman_smoother(X, L, sz, A, Q, agg_weights=w, **kw)
    assert e.value.code == -10 and "column 9" in str(e.value)
    with pytest.raises(dfm.DFMError) as e:   # an explosive A, P0 left to the library
        dfm.kalman_smoother(X, L, sigma2, 2.5 * A, Q, agg_weights=w, **kw)
    assert e.value.code == 6
    ok = dfm.kalman_smoother(X, L, sigma2, A, Q, agg_weights=w, **kw)   # the context still serves a good call
    assert np.isfinite(ok.loglik)
