"""The quasi-ML EM of the state-space factor model on the device (dfm_ss_em /
dfm_ss_fit_ml through ss_em and DynamicFactorModel_ss(method="ml")) against the
NumPy reference tests/ss_em_reference.py, whose E-step is the textbook filter
on the dense innovation covariance and whose M-step uses numpy.linalg.solve.

Bars.  Layers fed from the reference (the starts are the reference's, so
nothing upstream blurs the comparison): every array within RTOL = 1e-10 of the
reference array's largest magnitude, the loglik path 1e-10 relative — the
project's fp64 bar (tests/test_gpu_ss.py); a 1e-12 relative perturbation of the
starting loadings moves every reference output by at most 1.2e-12 after 4-8
iterations, so the iteration does not amplify rounding towards the bar.  End
to end (the device's own static EM underneath): E2E = 1e-8 on quantities that
do not depend on the factors' signs.  Batch against single calls, repeated
runs, device input and the horizon are bit-for-bit."""
import numpy as np
import pytest

import ss_em_reference as R
import ss_reference as S

pytestmark = pytest.mark.gpu

RTOL = 1e-10
E2E = 1e-8
FIT_IDS = [f"{T}x{N}" for T, N in S.SHAPES]
SYN_IDS = [f"{T}x{N}r{r}p{p}" for T, N, r, p in S.SYNTHETIC]
PARAMS = (("loadings", "L"), ("sigma2", "sigma2"), ("A", "A"), ("Q", "Q"), ("a0", "a0"), ("P0", "P0"))
OUTPUTS = ("filtered", "smoothed", "smoothed_cov")
FIELD_ORDER = ("loadings", "sigma2", "A", "Q", "a0", "P0", "filtered", "smoothed", "smoothed_cov", "loglik", "n_observed",
               "loglik_path", "iterations", "converged", "criterion")   # of StateSpaceEMResult
FIELDS = tuple(k for k, _ in PARAMS) + OUTPUTS + ("loglik", "n_observed", "loglik_path", "iterations", "converged",
                                                  "criterion")


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def report(label, fig, bar):
    """Print every figure, then assert each against its bar."""
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < bar, (label, k, v)


def em_figures(res, ref):
    fig = {k: big(getattr(res, k) - ref[rk]) / big(ref[rk]) for k, rk in PARAMS if k != "a0"}
    if big(ref["a0"]) == 0.0:   # a0 is not re-estimated and none was given: it stays exactly zero
        assert np.array_equal(res.a0, np.zeros_like(ref["a0"]))
    else:
        fig["a0"] = big(res.a0 - ref["a0"]) / big(ref["a0"])
    n = len(ref["path"])
    fig["path"] = float(np.max(np.abs(res.loglik_path[:n] - ref["path"]) / np.abs(ref["path"])))
    for k in OUTPUTS:
        fig[k] = big(getattr(res, k) - ref[k]) / big(ref[k])
    return fig


def same(a, b, fields=FIELDS):
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


def smoother_consistency(dfm, ctx, label, X, res, horizon):
    """The returned outputs are kalman_smoother's at the returned parameters."""
    ks = dfm.kalman_smoother(X, res.loadings, res.sigma2, res.A, res.Q, a0=res.a0, P0=res.P0, horizon=horizon, ctx=ctx)
    fig = {k: big(getattr(res, k) - getattr(ks, k)) / big(getattr(ks, k)) for k in OUTPUTS}
    fig["loglik"] = abs(res.loglik - ks.loglik) / abs(ks.loglik)
    print(label, "bit-equal to kalman_smoother:",
          all(np.array_equal(getattr(res, k), getattr(ks, k)) for k in OUTPUTS) and res.loglik == ks.loglik)
    assert res.n_observed == ks.n_observed
    report(label + " vs kalman_smoother", fig, RTOL)


def monotone(label, res):
    steps = np.diff(res.loglik_path[:res.iterations + 1])
    print(label, "smallest increment", steps.min())
    assert len(steps) == res.iterations and (steps > 0).all(), (label, steps)


# ------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("update_init", (True, False), ids=("init", "fixed"))
@pytest.mark.parametrize("i", range(4), ids=FIT_IDS)
def test_em_on_fitted_panels(dfm, ctx, i, update_init):
    """From the reference's Zm and two-step parameters: tol = 0, 8 iterations, HORIZON forecast rows."""
    _, ts = S.two_step_case(i)
    ref = R.fitted_em(i, update_init)
    res = dfm.ss_em(ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], P0=ts["P0"], tol=0.0, max_iter=8,
                    update_init=update_init, horizon=S.HORIZON, ctx=ctx)
    label = f"fitted {FIT_IDS[i]} update_init={update_init}"
    assert res.iterations == ref["iterations"] == 8 and not res.converged
    assert res.n_observed == ref["nobs"] and res.loglik == res.loglik_path[8]
    assert res.smoothed.shape == ref["smoothed"].shape and res.loglik_path.shape == (9,)
    report(label, em_figures(res, ref), RTOL)
    monotone(label, res)
    smoother_consistency(dfm, ctx, label, ts["Zm"], res, S.HORIZON)


@pytest.mark.parametrize("i", range(4), ids=SYN_IDS)
def test_em_at_the_limits(dfm, ctx, i):
    """The synthetic sets (s = 32, r = 16, the scalar case, s = 15) from their true parameters: tol = 0, 4 iterations."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(i)
    ref = R.synthetic_em(i)
    res = dfm.ss_em(X, L, sigma2, A, Q, tol=0.0, max_iter=4, ctx=ctx)
    label = f"synthetic {SYN_IDS[i]}"
    assert res.iterations == 4 and res.n_observed == ref["nobs"]
    report(label, em_figures(res, ref), RTOL)
    monotone(label, res)
    smoother_consistency(dfm, ctx, label, X, res, 0)


def test_max_iter_zero_is_one_e_step(dfm, ctx):
    X, L, sigma2, A, Q, ref = S.synthetic_case(3)
    s = A.shape[1]
    a0 = np.linspace(-1.0, 1.0, s)
    P0 = 2.0 * np.eye(s) + 0.5
    res = dfm.ss_em(X, L, sigma2, A, Q, a0=a0, P0=P0, max_iter=0, ctx=ctx)
    assert res.iterations == 0 and not res.converged and res.loglik_path.shape == (1,) and np.isnan(res.criterion)
    for got, want in ((res.loadings, L), (res.sigma2, sigma2), (res.A, A), (res.Q, Q), (res.a0, a0), (res.P0, P0)):
        assert np.array_equal(got, want)
    smoother_consistency(dfm, ctx, "max_iter=0", X, res, 0)
    rs = S.smooth(X, L, sigma2, A, Q, a0, P0)
    report("max_iter=0 vs reference", {k: big(getattr(res, k) - rs[k]) / big(rs[k]) for k in OUTPUTS}, RTOL)


# ---------------------------------------------------------------------- batch
@pytest.fixture(scope="module")
def batch(dfm, ctx):
    cases = [R.batch_case(k) for k in range(5)]
    X = np.stack([c[0]["Zm"] for c in cases])
    st = {k: np.stack([c[0][k] for c in cases]) for k in ("L", "sigma2", "A", "Q", "P0")}
    res = dfm.ss_em(X, st["L"], st["sigma2"], st["A"], st["Q"], P0=st["P0"], tol=1e-4, max_iter=60, ctx=ctx)
    return cases, X, st, res


def test_batch_panels_stop_on_their_own(dfm, ctx, batch):
    """Five panels, each from its own two-step start: the reference's stopping
    times, each panel bit-equal to its own single call, NaN beyond its path."""
    cases, X, st, res = batch
    print("iterations", res.iterations, "reference", [c[1]["iterations"] for c in cases])
    assert tuple(res.iterations) == tuple(c[1]["iterations"] for c in cases) == R.BATCH_ITERATIONS
    assert res.converged.all() and res.loglik_path.shape == (5, 61)
    for k, (start, ref) in enumerate(cases):
        one = dfm.ss_em(X[k], start["L"], start["sigma2"], start["A"], start["Q"], P0=start["P0"], tol=1e-4,
                        max_iter=60, ctx=ctx)
        for f in FIELDS:
            assert np.array_equal(getattr(res, f)[k], getattr(one, f), equal_nan=True), (k, f)
        j = ref["iterations"]
        assert np.isfinite(res.loglik_path[k, :j + 1]).all() and np.isnan(res.loglik_path[k, j + 1:]).all()
        assert res.loglik[k] == res.loglik_path[k, j]
        report(f"batch panel {k}", em_figures(one, ref), RTOL)


def test_em_across_k_chunks_and_row_tiles(dfm, ctx):
    """T = 270 takes two K chunks of the M-step GEMM (the second partial, T no
    multiple of 16), N = 70 two row tiles: two panels, each from its own start."""
    cases = [R.chunk_case(k) for k in range(2)]
    X = np.stack([c[0]["Zm"] for c in cases])
    st = {k: np.stack([c[0][k] for c in cases]) for k in ("L", "sigma2", "A", "Q", "P0")}
    assert X.shape[1:] == R.CHUNK_SHAPE
    res = dfm.ss_em(X, st["L"], st["sigma2"], st["A"], st["Q"], P0=st["P0"], tol=0.0, max_iter=3, ctx=ctx)
    assert tuple(res.iterations) == (3, 3)
    for k, (_, ref) in enumerate(cases):
        one = dfm.StateSpaceEMResult(*(getattr(res, f)[k] for f in FIELD_ORDER))
        report(f"chunks panel {k}", em_figures(one, ref), RTOL)
        monotone(f"chunks panel {k}", one)


def test_batch_with_a_shared_start(dfm, ctx, batch):
    cases, X, st, _ = batch
    start = cases[2][0]
    args = (start["L"], start["sigma2"], start["A"], start["Q"])
    res = dfm.ss_em(X, *args, P0=start["P0"], tol=1e-4, max_iter=60, ctx=ctx)
    print("iterations from the shared start", res.iterations)
    for k in range(5):
        one = dfm.ss_em(X[k], *args, P0=start["P0"], tol=1e-4, max_iter=60, ctx=ctx)
        for f in FIELDS:
            assert np.array_equal(getattr(res, f)[k], getattr(one, f), equal_nan=True), (k, f)


def test_pass_loop_taken_twice(dfm, ctx):
    """S.two_pass_case under the EM, max_iter = 1 (two E-steps) from a shared start.  At the smoother's Tt = 4096
    and M = 9 a panel keeps the smoother's 8949826 doubles, the M-step's rows (4096), the operand rows (512), the
    moments (2848), its parameter block (4244) and 8 ints: 71692240 B, 7 per pass as for the smoother
    (tests/c_harness/ss_sim_host.cpp) — but the five calls' ten serial recursions take 5 s.  So half the rows and
    twice the panels: horizon 2040 (Tt = 2048), 4096 + 2048 x 2112 + 64 + 16384 + 131072 + 2 + 11700 doubles and 32
    B = 35909584 B a panel, 2^29 / 35909584 = 14 per pass, and M = 16 runs as passes of 14 and 2.  The first and
    last panel of each pass against a call on that panel alone, bit for bit."""
    panels, L, sigma2, A, Q, h = S.two_pass_case(M=16, horizon=2040)
    kw = dict(tol=0.0, max_iter=1, horizon=h, ctx=ctx)
    res = dfm.ss_em(panels, L, sigma2, A, Q, **kw)
    assert tuple(res.iterations) == (1,) * 16 and res.smoothed.shape == (16, 8 + h, 8)
    for k in (0, 13, 14, 15):
        one = dfm.ss_em(panels[k], L, sigma2, A, Q, **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(res, f)[k], getattr(one, f), equal_nan=True), (k, f)


# ---------------------------------------------------------------- bit for bit
def test_repeat_device_input_and_horizon(dfm, ctx, batch):
    import torch
    cases, X, st, a = batch
    kw = dict(P0=st["P0"], tol=1e-4, max_iter=60, ctx=ctx)
    b = dfm.ss_em(X, st["L"], st["sigma2"], st["A"], st["Q"], **kw)
    xd = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).cuda().transpose(1, 2)
    d = dfm.ss_em(xd, st["L"], st["sigma2"], st["A"], st["Q"], **kw)
    same(a, b)
    same(a, d)
    hz = dfm.ss_em(X, st["L"], st["sigma2"], st["A"], st["Q"], horizon=4, **kw)
    T = X.shape[1]
    same(a, hz, tuple(k for k, _ in PARAMS) + ("filtered", "loglik", "n_observed", "loglik_path", "iterations",
                                               "converged", "criterion"))
    assert hz.smoothed.shape == (5, T + 4, 2)
    assert np.array_equal(hz.smoothed[:, :T], a.smoothed) and np.array_equal(hz.smoothed_cov[:, :T], a.smoothed_cov)
    one_d = dfm.ss_em(xd[1], st["L"][1], st["sigma2"][1], st["A"][1], st["Q"][1], P0=st["P0"][1], tol=1e-4, max_iter=60,
                      ctx=ctx)   # a single column-major device panel
    for f in FIELDS:
        assert np.array_equal(getattr(a, f)[1], getattr(one_d, f), equal_nan=True), f


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("i", (0, 3), ids=(FIT_IDS[0], FIT_IDS[3]))
def test_ml_fit_end_to_end(dfm, ctx, i):
    X, ts = S.two_step_case(i)
    T, N = X.shape
    r, p = S.TWO_STEP_RP[i]
    h = S.HORIZON
    kw = dict(lags=p, tol=0.0, max_iter=6, horizon=h, ctx=ctx)
    ml = dfm.DynamicFactorModel_ss(X, r, method="ml", ml_tol=0.0, ml_max_iter=5, **kw)
    two = dfm.DynamicFactorModel_ss(X, r, method="two-step", **kw)
    plain = dfm.DynamicFactorModel_ss(X, r, **kw)
    for f in ("sigma2", "A", "Q", "P0", "loadings", "filtered", "smoothed", "smoothed_cov", "x_smoothed",
              "x_completed", "forecast", "mean", "std"):
        assert np.array_equal(getattr(two, f), getattr(plain, f)), f
    assert two.loglik == plain.loglik and plain.method == "two-step" and plain.loglik_path is None
    zm = np.where(np.isnan(X), np.nan, two.em.x_standardized)
    em = dfm.ss_em(zm, two.loadings, two.sigma2, two.A, two.Q, P0=two.P0, tol=0.0, max_iter=5, horizon=h, ctx=ctx)
    for f in ("loadings", "sigma2", "A", "Q", "a0", "P0", "filtered", "smoothed", "smoothed_cov", "loglik_path"):
        assert np.array_equal(getattr(ml, f), getattr(em, f)), f
    assert ml.loglik == em.loglik and ml.ml_iterations == em.iterations == 5 and not ml.ml_converged
    assert np.array_equal(ml.mean, two.mean) and np.array_equal(ml.std, two.std)
    print(f"end to end {FIT_IDS[i]}: loglik two-step {two.loglik:.6f} ml {ml.loglik:.6f}")
    assert ml.loglik > two.loglik and ml.loglik_path[0] == two.loglik
    obs = ~np.isnan(X)
    assert np.array_equal(ml.x_completed[obs], X[obs]) and not np.isnan(ml.x_completed).any()
    assert ml.forecast.shape == (h, N) and ml.smoothed.shape == (T + h, r)
    ref = R.ml_chain(i, max_iter=5)
    fig = {"x_completed": big(ml.x_completed - ref["x_completed"]) / big(ref["x_completed"]),
           "forecast": big(ml.forecast - ref["forecast"]) / big(ref["forecast"])}
    report(f"end to end {FIT_IDS[i]}", fig, E2E)


# -------------------------------------------------------------------- errors
def test_errors(dfm, ctx):
    """Argument checks made before any device work."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(3)
    bad = L.copy()
    bad[3, 1] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.ss_em(X, bad, sigma2, A, Q, ctx=ctx)
    assert e.value.code == -12
    sz = sigma2.copy()
    sz[9] = 0.0
    with pytest.raises(dfm.DFMError) as e:
        dfm.ss_em(X, L, sz, A, Q, ctx=ctx)
    assert e.value.code == -10 and "column 9" in str(e.value)
    with pytest.raises(dfm.DFMError) as e:   # r = 17
        dfm.ss_em(X, np.ones((40, 17)), sigma2, 0.1 * np.eye(17), np.eye(17), ctx=ctx)
    assert e.value.code == -7
    Xe = X.copy()
    Xe[:, 5] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.ss_em(Xe, L, sigma2, A, Q, ctx=ctx)
    assert e.value.code == -2 and "column 5" in str(e.value)
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(Xe.T)).cuda().t()   # column-major in HBM: found before the first pass
    for mi in (0, 3):
        with pytest.raises(dfm.DFMError) as e:
            dfm.ss_em(xd, L, sigma2, A, Q, max_iter=mi, ctx=ctx)
        assert e.value.code == -2 and "column 5" in str(e.value)
    with pytest.raises(ValueError):   # per-panel starts of differing r
        dfm.ss_em(np.stack([X, X]), [L, L[:, :3]], sigma2, A, Q, ctx=ctx)
    ok = dfm.ss_em(X, L, sigma2, A, Q, max_iter=1, ctx=ctx)   # the context still serves a good call
    assert np.isfinite(ok.loglik) and ok.iterations == 1
