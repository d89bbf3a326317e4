"""The mixed-frequency fit on the device (dfm_ss_fit_mf through
DynamicFactorModel_ss(low_freq=, agg_weights=)) against the NumPy chain of
tests/ss_mf_reference.py (em_reference.em -> ss_reference.estimate ->
start_values -> the dense smoother or the restricted EM), on a 60 x 14 panel
with r = 2, p = 1 and the flow weights.

The device's own static EM runs underneath, so the bar is the project's end to
end one: 1e-8 of the largest magnitude on quantities that do not depend on the
factors' signs (log-likelihood, the three panels); observed entries of
x_completed are bit-equal to x."""
import numpy as np
import pytest

import ss_mf_reference as R

pytestmark = pytest.mark.gpu

E2E = 1e-8
T, N, r, p, W = R.FIT_SHAPE
H = R.FIT_HORIZON


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def run(dfm, ctx, X, low, method, **kw):
    return dfm.DynamicFactorModel_ss(X, r, lags=p, horizon=H, tol=0.0, max_iter=6, method=method, ml_tol=0.0,
                                     ml_max_iter=4, low_freq=low, agg_weights=W, ctx=ctx, **kw)


@pytest.mark.parametrize("method", ["two-step", "ml"])
def test_fit_against_the_numpy_chain(dfm, ctx, method):
    ref = R.fit_case(method)
    X, low = ref["X"], ref["low"]
    fit = run(dfm, ctx, X, low, method)
    obs = ~np.isnan(X)
    hole = ~obs[:, low]
    fig = {"loglik": abs(fit.loglik - ref["loglik"]) / abs(ref["loglik"]),
           "x_smoothed": big(fit.x_smoothed - ref["x_smoothed"]) / big(ref["x_smoothed"]),
           "x_completed": big(fit.x_completed - ref["x_completed"]) / big(ref["x_completed"]),
           "low months": big((fit.x_completed[:, low] - ref["x_completed"][:, low])[hole]) / big(ref["x_completed"][:, low]),
           "forecast": big(fit.forecast - ref["forecast"]) / big(ref["forecast"]),
           "sigma2": big(fit.sigma2 - ref["res"]["sigma2"]) / big(ref["res"]["sigma2"]) if method == "ml" else 0.0}
    print(method, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert np.array_equal(fit.x_completed[obs], X[obs])
    assert not np.isnan(fit.x_completed).any() and not np.isnan(fit.forecast).any()
    assert fit.forecast.shape == (H, N) and fit.smoothed_agg.shape == (T + H, r) and fit.P0.shape == (10, 10)
    assert fit.A.shape == (r, r * p)
    if method == "ml":
        assert fit.ml_iterations == 4 and (np.diff(fit.loglik_path) > 0).all() and fit.a0.shape == (10,)
    for k, v in fig.items():
        assert v < E2E, (method, k, v)


def test_fit_is_repeatable_and_takes_device_input(dfm, ctx):
    import torch
    X, low = R.make_fit_panel()
    a = run(dfm, ctx, X, low, "ml")
    b = run(dfm, ctx, X, low, "ml")
    d = run(dfm, ctx, torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), low, "ml")
    for o in (b, d):
        for f in ("sigma2", "A", "Q", "P0", "a0", "loadings", "filtered", "smoothed", "smoothed_cov", "smoothed_agg",
                  "x_smoothed", "x_completed", "forecast", "loglik_path"):
            assert np.array_equal(getattr(a, f), getattr(o, f)), f


@pytest.mark.parametrize("method", ["two-step", "ml"])
def test_no_low_series_is_the_plain_fit(dfm, ctx, method):
    X, low = R.make_fit_panel()
    kw = dict(lags=p, horizon=H, tol=0.0, max_iter=6, method=method, ml_tol=0.0, ml_max_iter=3, ctx=ctx)
    plain = dfm.DynamicFactorModel_ss(X, r, **kw)
    none = dfm.DynamicFactorModel_ss(X, r, low_freq=np.zeros_like(low), agg_weights=W, **kw)
    for f in ("sigma2", "A", "Q", "P0", "loadings", "filtered", "smoothed", "smoothed_cov", "x_smoothed", "x_completed",
              "forecast"):
        assert np.array_equal(getattr(plain, f), getattr(none, f)), f
    assert plain.loglik == none.loglik and none.smoothed_agg is None


def test_errors(dfm, ctx):
    X, low = R.make_fit_panel()
    Xf = X.copy()
    col = int(np.flatnonzero(low)[1])
    Xf[:, col] = np.nan
    Xf[8, col], Xf[11, col] = 1.0, -0.5
    with pytest.raises(dfm.DFMError) as e:   # two usable rows for r = 2
        run(dfm, ctx, Xf, low, "two-step")
    assert e.value.code == -11 and f"column {col}" in str(e.value)
    with pytest.raises(dfm.DFMError) as e:   # r = 8, n_w = 5
        dfm.DynamicFactorModel_ss(X, 8, low_freq=low, agg_weights=W, ctx=ctx)
    assert e.value.code == -7
    with pytest.raises(dfm.DFMError) as e:
        dfm.DynamicFactorModel_ss(X, r, low_freq=low, agg_weights=(0.0, 1.0), ctx=ctx)
    assert e.value.code == -2
    with pytest.raises(dfm.DFMError) as e:
        dfm.DynamicFactorModel_ss(X, r, low_freq=low[:-1], agg_weights=W, ctx=ctx)
    assert e.value.code == -2
