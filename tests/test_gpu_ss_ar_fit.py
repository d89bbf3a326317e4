"""The two-step fit with AR(1) idiosyncratic terms on the device
(dfm_ss_fit_ar through DynamicFactorModel_ss(idiosyncratic_ar1=True)) on a
60 x 14 panel drawn with AR(1) idiosyncratic terms (rho up to 0.8), late
starters, a ragged edge and two holes (tests/ss_ar_reference.py::fit_panel).

The fit is the chain em_factors -> ss_parameters(idio_ar1=True) ->
kalman_smoother(idio_ar=) -> idio_fill bit for bit (the conversion to the
panel's units is one fma in the library and two roundings in NumPy: one ulp).
Against the NumPy chain: 1e-8 of the largest magnitude on quantities that do not
depend on the factors' signs, the project's end-to-end bar, and the smoothed
factors by principal angle below 1e-8.  Observed entries of x_completed are
bit-equal to x.  At the ragged edge the forecast carries rho^(k + gap) ehat."""
import numpy as np
import pytest

import em_reference as E
import ss_ar_reference as AR

pytestmark = pytest.mark.gpu

E2E = 1e-8
ANGLE = 1e-8
KW = dict(lags=AR.FIT_P, horizon=AR.FIT_H, tol=0.0, max_iter=6)


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


@pytest.fixture(scope="module")
def fit(dfm, ctx):
    return dfm.DynamicFactorModel_ss(AR.fit_panel(), AR.FIT_R, idiosyncratic_ar1=True, ctx=ctx, **KW)


def big(a):
    return float(np.max(np.abs(a)))


def test_panel_is_what_the_issue_asks():
    X = AR.fit_panel()
    assert X.shape == (60, 14)
    m = ~np.isnan(X)
    assert not m[:5, 1].any() and not m[:9, 9].any()                       # late starters
    assert all(not m[60 - g:, i].any() and m[60 - g - 1, i] for i, g in zip(AR.FIT_RAGGED, AR.FIT_GAP))
    assert not m[20:23, 5].any() and m[19, 5] and m[23, 5] and not m[40, 11] and m[39, 11] and m[41, 11]   # two holes


def test_fit_is_the_chain_of_its_steps(dfm, ctx, fit):
    X = AR.fit_panel()
    T, N = X.shape
    r, p, h = AR.FIT_R, AR.FIT_P, AR.FIT_H
    em = dfm.em_factors(X, r, tol=0.0, max_iter=6, ctx=ctx)
    for f in ("x_standardized", "x_completed", "mean", "std", "factors", "loadings", "eigenvalues"):
        assert np.array_equal(getattr(fit.em, f), getattr(em, f)), f
    zm = np.where(np.isnan(X), np.nan, em.x_standardized)
    sg, A, Q, P0, rho = dfm.ss_parameters(zm, em.factors, em.loadings, p, idio_ar1=True, ctx=ctx)
    assert P0.shape == (r * max(p, 2), r * max(p, 2)) and rho.shape == (N,)
    for name, a, b in (("sigma2", fit.sigma2, sg), ("A", fit.A, A), ("Q", fit.Q, Q), ("P0", fit.P0, P0),
                       ("idio_ar", fit.idio_ar, rho), ("loadings", fit.loadings, em.loadings)):
        assert np.array_equal(a, b), name
    ks = dfm.kalman_smoother(zm, em.loadings, sg, A, Q, P0=P0, horizon=h, idio_ar=rho, ctx=ctx)
    assert np.array_equal(fit.filtered, ks.filtered) and np.array_equal(fit.smoothed, ks.smoothed)
    assert np.array_equal(fit.smoothed_cov, ks.smoothed_cov) and fit.loglik == ks.loglik
    z = dfm.idio_fill(zm, em.loadings, rho, ks.smoothed)
    assert z.shape == (T + h, N)
    assert np.array_equal(fit.x_smoothed, z[:T])
    miss = np.isnan(X)
    units = z * em.std + em.mean
    ulp = np.spacing(np.abs(z * em.std) + np.abs(em.mean))
    assert np.all(np.abs(fit.x_completed[miss] - units[:T][miss]) <= ulp[:T][miss])
    assert np.all(np.abs(fit.forecast - units[T:]) <= ulp[T:])


def test_fit_against_the_numpy_chain(fit):
    X, ts = AR.fit_panel(), AR.fit_reference()
    T, N = X.shape
    h = AR.FIT_H
    obs = ~np.isnan(X)
    Lr, cr = ts["em"]["L"], ts["smooth"]["smoothed_cov"]
    fig = {"loglik": abs(fit.loglik - ts["loglik"]) / abs(ts["loglik"]),
           "rho": big(fit.idio_ar - ts["rho"]) / big(ts["rho"]),
           "sigma2": big(fit.sigma2 - ts["sigma2"]) / big(ts["sigma2"]),
           "x_smoothed": big(fit.x_smoothed - ts["x_smoothed"]) / big(ts["x_smoothed"]),
           "x_completed": big(fit.x_completed - ts["x_completed"]) / big(ts["x_completed"]),
           "forecast": big(fit.forecast - ts["forecast"]) / big(ts["forecast"]),
           "angle": E.max_principal_angle(fit.smoothed, ts["smooth"]["smoothed"])}
    for t, a, b in ((0, 0, 0), (T // 2, 1, N - 1), (T + h - 1, 2, 5)):   # Lambda P_t|T Lambda' at three fixed entries
        g = fit.loadings @ fit.smoothed_cov[t] @ fit.loadings.T
        w = Lr @ cr[t] @ Lr.T
        fig[f"LPL[{t},{a},{b}]"] = abs(g[a, b] - w[a, b]) / big(w)
    print("end to end", " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fit.forecast.shape == (h, N) and fit.smoothed.shape == (T + h, AR.FIT_R)
    assert np.array_equal(fit.x_completed[obs], X[obs])
    assert np.array_equal(fit.x_smoothed[obs], fit.em.x_standardized[obs])
    assert not np.isnan(fit.x_completed).any() and not np.isnan(fit.x_smoothed).any()
    for k, v in fig.items():
        assert v < (ANGLE if k == "angle" else E2E), (k, v)


def test_forecast_carries_the_last_idiosyncratic_deviation(fit):
    """forecast - (Lambda f_{T+k|T}) sd - mu = rho^(k + gap) ehat sd for the ragged series, k = 1..h."""
    X = AR.fit_panel()
    T = X.shape[0]
    zm = np.where(np.isnan(X), np.nan, fit.em.x_standardized)
    common = fit.smoothed @ fit.loadings.T
    for i, gap in zip(AR.FIT_RAGGED, AR.FIT_GAP):
        u = T - gap - 1
        ehat = zm[u, i] - common[u, i]
        assert abs(ehat) > 1e-3 and abs(fit.idio_ar[i]) > 0.1   # the reference chain gives 0.3 and 0.6
        for k in range(1, AR.FIT_H + 1):
            got = fit.forecast[k - 1, i] - common[T + k - 1, i] * fit.std[i] - fit.mean[i]
            want = fit.idio_ar[i] ** (k + gap) * ehat * fit.std[i]
            assert abs(got - want) <= 1e-10 * max(1.0, abs(fit.forecast[k - 1, i])), (i, k, got, want)
        for t in range(u + 1, T):   # the ragged edge itself
            got = fit.x_smoothed[t, i] - common[t, i]
            assert abs(got - fit.idio_ar[i] ** (t - u) * ehat) <= 1e-10


def test_repeatable(dfm, ctx, fit):
    again = dfm.DynamicFactorModel_ss(AR.fit_panel(), AR.FIT_R, idiosyncratic_ar1=True, ctx=ctx, **KW)
    assert again.loglik == fit.loglik
    for f in ("sigma2", "A", "Q", "P0", "idio_ar", "filtered", "smoothed", "smoothed_cov", "x_smoothed", "x_completed",
              "forecast"):
        assert np.array_equal(getattr(again, f), getattr(fit, f)), f
