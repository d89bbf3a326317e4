"""The state-space pass on the device (dfm_ss_smooth / dfm_ss_estimate /
dfm_ss_fit through kalman_smoother, ss_parameters, DynamicFactorModel_ss)
against the NumPy reference tests/ss_reference.py, whose reference filter is
the textbook one on the dense innovation covariance.

Bars.  Smoother and parameter layers (inputs taken from the reference, so
nothing upstream blurs the comparison): loglik 1e-10 relative, every array
within 1e-10 of the reference array's largest magnitude — the project's fp64
bar; the reference's two filters agree four orders below it
(tests/test_ss_host.py).  End to end (the device's own EM underneath): 1e-8 of
the largest magnitude on quantities that do not depend on the factors' signs,
the project's bar for factor-derived quantities; smoothed factors by principal
angle below 1e-8; observed entries of x_completed bit-equal to x.  Composition,
horizon, batch, device input and repeatability are bit-for-bit."""
import numpy as np
import pytest

import em_reference as E
import ss_reference as S

pytestmark = pytest.mark.gpu

RTOL = 1e-10
E2E = 1e-8
ANGLE = 1e-8
FIT_IDS = [f"{T}x{N}" for T, N in S.SHAPES]
SYN_IDS = [f"{T}x{N}r{r}p{p}" for T, N, r, p in S.SYNTHETIC]


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def report(label, fig, bar):
    """Print every figure, then assert each against its bar."""
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < (ANGLE if k == "angle" else bar), (label, k, v)


def smoother_figures(res, ref):
    return {"loglik": abs(res.loglik - ref["loglik"]) / abs(ref["loglik"]),
            "filtered": big(res.filtered - ref["filtered"]) / big(ref["filtered"]),
            "smoothed": big(res.smoothed - ref["smoothed"]) / big(ref["smoothed"]),
            "cov": big(res.smoothed_cov - ref["smoothed_cov"]) / big(ref["smoothed_cov"])}


# ------------------------------------------------------------ smoother layer
@pytest.mark.parametrize("i", range(4), ids=FIT_IDS)
def test_smoother_on_fitted_parameters(dfm, ctx, i):
    """The reference's Zm and fitted (Lambda, sigma^2, A, Q, P0), HORIZON forecast rows."""
    _, ts = S.two_step_case(i)
    ref = ts["smooth"]
    res = dfm.kalman_smoother(ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], P0=ts["P0"],
                              horizon=S.HORIZON, ctx=ctx)
    assert res.n_observed == ref["nobs"] == int((~np.isnan(ts["Zm"])).sum())
    assert res.smoothed.shape == ref["smoothed"].shape and res.filtered.shape == ref["filtered"].shape
    report(f"fitted {FIT_IDS[i]}", smoother_figures(res, ref), RTOL)


@pytest.mark.parametrize("i", range(4), ids=SYN_IDS)
def test_smoother_on_synthetic_parameters(dfm, ctx, i):
    """Drawn parameters at the limits (s = 32, r = 16, the scalar case, s = 15);
    P0 is left to the library: the doubling iteration against the Kronecker solve."""
    X, L, sigma2, A, Q, ref = S.synthetic_case(i)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, ctx=ctx)
    assert res.n_observed == ref["nobs"]
    report(f"synthetic {SYN_IDS[i]}", smoother_figures(res, ref), RTOL)


def test_smoother_with_a0(dfm, ctx):
    """A caller's a0 and P0 (not the stationary ones)."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(3)
    s = A.shape[1]
    a0 = np.linspace(-1.0, 1.0, s)
    P0 = 2.0 * np.eye(s) + 0.5
    ref = S.smooth(X, L, sigma2, A, Q, a0, P0)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, a0=a0, P0=P0, ctx=ctx)
    report("a0/P0", smoother_figures(res, ref), RTOL)


# ----------------------------------------------------------- parameter layer
@pytest.mark.parametrize("i", range(4), ids=FIT_IDS)
def test_parameters(dfm, ctx, i):
    _, ts = S.two_step_case(i)
    p = S.TWO_STEP_RP[i][1]
    sg, A, Q, P0 = dfm.ss_parameters(ts["Zm"], ts["em"]["F"], ts["em"]["L"], p, ctx=ctx)
    fig = {k: big(g - ts[k]) / big(ts[k]) for k, g in (("sigma2", sg), ("A", A), ("Q", Q), ("P0", P0))}
    report(f"parameters {FIT_IDS[i]}", fig, RTOL)


# --------------------------------------------------------------- composition
@pytest.mark.parametrize("i", range(4), ids=FIT_IDS)
def test_fit_is_the_chain_of_its_steps(dfm, ctx, i):
    """DynamicFactorModel_ss == em_factors -> ss_parameters -> kalman_smoother, bit for bit."""
    X, _ = S.two_step_case(i)
    r, p = S.TWO_STEP_RP[i]
    fit = dfm.DynamicFactorModel_ss(X, r, lags=p, horizon=S.HORIZON, tol=0.0, max_iter=6, ctx=ctx)
    em = dfm.em_factors(X, r, tol=0.0, max_iter=6, ctx=ctx)
    for f in ("x_standardized", "x_completed", "mean", "std", "factors", "loadings", "eigenvalues"):
        assert np.array_equal(getattr(fit.em, f), getattr(em, f)), f
    assert (fit.em.iterations, fit.em.error, fit.em.n_missing) == (em.iterations, em.error, em.n_missing) and \
        em.iterations == 6
    zm = np.where(np.isnan(X), np.nan, em.x_standardized)
    sg, A, Q, P0 = dfm.ss_parameters(zm, em.factors, em.loadings, p, ctx=ctx)
    for a, b in ((fit.sigma2, sg), (fit.A, A), (fit.Q, Q), (fit.P0, P0), (fit.loadings, em.loadings)):
        assert np.array_equal(a, b)
    ks = dfm.kalman_smoother(zm, em.loadings, sg, A, Q, P0=P0, horizon=S.HORIZON, ctx=ctx)
    assert np.array_equal(fit.filtered, ks.filtered) and np.array_equal(fit.smoothed, ks.smoothed)
    assert np.array_equal(fit.smoothed_cov, ks.smoothed_cov) and fit.loglik == ks.loglik
    assert (fit.number_of_factors, fit.lags) == (r, p)


def test_fit_device_input_and_repeatability(dfm, ctx):
    import torch
    X, _ = S.two_step_case(3)
    r, p = S.TWO_STEP_RP[3]
    kw = dict(lags=p, horizon=2, tol=0.0, max_iter=6, ctx=ctx)
    a = dfm.DynamicFactorModel_ss(X, r, **kw)
    b = dfm.DynamicFactorModel_ss(X, r, **kw)
    xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()   # column-major in HBM
    d = dfm.DynamicFactorModel_ss(xd, r, **kw)
    assert a.em.iterations == b.em.iterations == d.em.iterations == 6
    for o in (b, d):
        assert o.loglik == a.loglik
        for f in ("sigma2", "A", "Q", "P0", "filtered", "smoothed", "smoothed_cov", "x_smoothed", "x_completed",
                  "forecast", "mean", "std", "loadings"):
            assert np.array_equal(getattr(a, f), getattr(o, f)), f


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("i", range(4), ids=FIT_IDS)
def test_fit_against_the_numpy_two_step_fit(dfm, ctx, i):
    X, ts = S.two_step_case(i)
    T, N = X.shape
    r, p = S.TWO_STEP_RP[i]
    h = S.HORIZON
    fit = dfm.DynamicFactorModel_ss(X, r, lags=p, horizon=h, tol=0.0, max_iter=6, ctx=ctx)
    obs = ~np.isnan(X)
    Lr, cr = ts["em"]["L"], ts["smooth"]["smoothed_cov"]
    fig = {"loglik": abs(fit.loglik - ts["loglik"]) / abs(ts["loglik"]),
           "x_smoothed": big(fit.x_smoothed - ts["x_smoothed"]) / big(ts["x_smoothed"]),
           "x_completed": big(fit.x_completed - ts["x_completed"]) / big(ts["x_completed"]),
           "forecast": big(fit.forecast - ts["forecast"]) / big(ts["forecast"]),
           "angle": E.max_principal_angle(fit.smoothed, ts["smooth"]["smoothed"])}
    for t, a, b in ((0, 0, 0), (T // 2, 1, N - 1), (T + h - 1, 2, 5)):   # Lambda P_t|T Lambda' at three fixed entries
        g = fit.loadings @ fit.smoothed_cov[t] @ fit.loadings.T
        w = Lr @ cr[t] @ Lr.T
        fig[f"LPL[{t},{a},{b}]"] = abs(g[a, b] - w[a, b]) / big(w)
    assert fit.forecast.shape == (h, N) and fit.smoothed.shape == (T + h, r)
    assert np.array_equal(fit.x_completed[obs], X[obs])
    assert np.array_equal(fit.x_smoothed[obs], fit.em.x_standardized[obs])
    assert not np.isnan(fit.x_completed).any() and not np.isnan(fit.x_smoothed).any()
    report(f"end to end {FIT_IDS[i]}", fig, E2E)


# ------------------------------------------------------------------- horizon
def test_horizon_is_appended_missing_rows(dfm, ctx):
    X, L, sigma2, A, Q, _ = S.synthetic_case(0)
    T, N = X.shape
    base = dfm.kalman_smoother(X, L, sigma2, A, Q, ctx=ctx)
    hor = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=4, ctx=ctx)
    app = dfm.kalman_smoother(np.vstack([X, np.full((4, N), np.nan)]), L, sigma2, A, Q, ctx=ctx)
    assert np.array_equal(hor.smoothed, app.smoothed) and np.array_equal(hor.smoothed_cov, app.smoothed_cov)
    assert np.array_equal(hor.filtered, app.filtered[:T]) and hor.loglik == app.loglik
    assert hor.n_observed == app.n_observed == base.n_observed
    assert np.array_equal(hor.smoothed[:T], base.smoothed) and np.array_equal(hor.smoothed_cov[:T], base.smoothed_cov)
    assert np.array_equal(hor.filtered, base.filtered) and hor.loglik == base.loglik


# --------------------------------------------------------------------- batch
def test_batch_device_input_and_repeatability(dfm, ctx):
    import torch
    shape = S.SYNTHETIC[3]   # 60 x 40, r = 5, p = 3
    X0, L, sigma2, A, Q = S.make_synthetic(*shape)
    full = S.make_synthetic(*shape, complete=True)[0]
    X1 = full.copy()
    X1[np.random.default_rng(11).uniform(size=full.shape) < 0.35] = np.nan
    X1[7, :] = np.nan
    panels = np.stack([X0, X1, full])
    a = dfm.kalman_smoother(panels, L, sigma2, A, Q, horizon=2, ctx=ctx)
    b = dfm.kalman_smoother(panels, L, sigma2, A, Q, horizon=2, ctx=ctx)
    xd = torch.from_numpy(np.ascontiguousarray(panels.transpose(0, 2, 1))).cuda().transpose(1, 2)
    d = dfm.kalman_smoother(xd, L, sigma2, A, Q, horizon=2, ctx=ctx)
    fields = ("filtered", "smoothed", "smoothed_cov", "loglik", "n_observed")
    for o in (b, d):
        for f in fields:
            assert np.array_equal(getattr(a, f), getattr(o, f)), f
    assert a.smoothed.shape == (3, 62, 5) and a.n_observed[2] == 60 * 40
    for k in range(3):
        one = dfm.kalman_smoother(panels[k], L, sigma2, A, Q, horizon=2, ctx=ctx)
        for f in fields:
            assert np.array_equal(getattr(a, f)[k], getattr(one, f)), (k, f)
        ref = S.smooth(panels[k], L, sigma2, A, Q, horizon=2)
        report(f"batch panel {k}", smoother_figures(one, ref), RTOL)
    one_d = dfm.kalman_smoother(xd[1], L, sigma2, A, Q, horizon=2, ctx=ctx)   # a single column-major device panel
    assert np.array_equal(one_d.smoothed, a.smoothed[1]) and one_d.loglik == a.loglik[1]


def test_pass_loop_taken_twice(dfm, ctx):
    """S.two_pass_case: a panel of the smoother keeps 4096 (collapsed rows) + 4096 x 2112 (workspace) + 64 + 32768
    + 262144 + 2 (outputs) doubles = 71598608 B: ss_panels_per_pass gives 7 per half GB
    (tests/c_harness/ss_sim_host.cpp), so M = 9 runs as a pass of 7 and a pass of 2.  The first and last panel of
    each pass against a call on that panel alone, bit for bit."""
    panels, L, sigma2, A, Q, h = S.two_pass_case()
    a = dfm.kalman_smoother(panels, L, sigma2, A, Q, horizon=h, ctx=ctx)
    assert a.smoothed.shape == (9, 8 + h, 8) and a.n_observed[8] == 28
    for k in (0, 6, 7, 8):
        one = dfm.kalman_smoother(panels[k], L, sigma2, A, Q, horizon=h, ctx=ctx)
        for f in ("filtered", "smoothed", "smoothed_cov", "loglik", "n_observed"):
            assert np.array_equal(getattr(a, f)[k], getattr(one, f)), (k, f)


# -------------------------------------------------------------------- errors
def test_errors(dfm, ctx):
    """Every new return code from a minimal input; all are argument checks made before any device work."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(3)
    bad = L.copy()
    bad[3, 1] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.kalman_smoother(X, bad, sigma2, A, Q, ctx=ctx)
    assert e.value.code == -12
    sz = sigma2.copy()
    sz[9] = 0.0
    with pytest.raises(dfm.DFMError) as e:
        dfm.kalman_smoother(X, L, sz, A, Q, ctx=ctx)
    assert e.value.code == -10 and "column 9" in str(e.value)
    with pytest.raises(dfm.DFMError) as e:   # r p = 36
        dfm.kalman_smoother(X, np.ones((40, 12)), sigma2, np.hstack([0.1 * np.eye(12)] * 3), np.eye(12), ctx=ctx)
    assert e.value.code == -7
    with pytest.raises(dfm.DFMError) as e:   # r = 17
        dfm.kalman_smoother(X, np.ones((40, 17)), sigma2, 0.1 * np.eye(17), np.eye(17), ctx=ctx)
    assert e.value.code == -7
    Ax = 2.0 * A
    assert S.spectral_radius(Ax) > 1.0
    with pytest.raises(dfm.DFMError) as e:   # an explosive A, P0 left to the library
        dfm.kalman_smoother(X, L, sigma2, Ax, Q, ctx=ctx)
    assert e.value.code == 6
    rng = np.random.default_rng(2)
    with pytest.raises(dfm.DFMError) as e:   # T - p = 6 <= r p = 6
        dfm.ss_parameters(rng.standard_normal((8, 6)), rng.standard_normal((8, 3)), rng.standard_normal((6, 3)), 2,
                          ctx=ctx)
    assert e.value.code == -11
    with pytest.raises(dfm.DFMError) as e:
        dfm.DynamicFactorModel_ss(S.make_two_step_panel(60, 40), 3, lags=9, ctx=ctx)
    assert e.value.code == -7
    with pytest.raises(dfm.DFMError) as e:   # 10 rows, r = 3, p = 3: T - p = 7 <= 9
        dfm.DynamicFactorModel_ss(np.random.default_rng(4).standard_normal((10, 12)), 3, lags=3, ctx=ctx)
    assert e.value.code == -11
    ok = dfm.kalman_smoother(X, L, sigma2, A, Q, ctx=ctx)   # the context still serves a good call
    assert np.isfinite(ok.loglik)
