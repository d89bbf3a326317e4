"""Principal components with missing observations (dfm_em / em_factors /
DynamicFactorModel_em) against the NumPy restatement tests/em_reference.py
(the oracle's PCA, scipy eigh "evr") on the four panels of its generator:

  60 x 40   T >= N, N not a multiple of 16 (three strips, the last half full)
  40 x 72   N > T (XX'), five strips
  33 x 33   the T == N branch, odd sizes; ICp2 picks r^ = 2
  67 x 19   two strips, the second partial; more than one 64-row tile

Bars: eigenvalues, V and err 1e-10 relative; factors to a principal angle
below 1e-8; Z, X2, mu, sd within 1e-10 of the panel's largest magnitude;
observed entries of X2 bit-equal to X.  The reference itself: six forced
iterations in float64 and in long double differ by ~2e-15 relative in C, and
at tol = 1e-6 its final err is 22 %, 23 %, 3.5 % and 6.3 % clear of tol on the
four panels (18, 19, 31, 13 iterations), so the iteration counts are compared
exactly."""
import ctypes as C

import numpy as np
import pytest

import em_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
ANGLE = 1e-8
IDS = [f"{T}x{N}" for T, N in R.SHAPES]


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def check(res, ref, X, label):
    """The bars of the module docstring; prints every figure before it asserts."""
    T, N = X.shape
    obs = ~np.isnan(X)
    big = float(np.max(np.abs(X[obs])))
    r = ref["r"]
    assert res.number_of_factors == r
    Vg = float(np.sum((res.x_standardized - res.factors @ res.loadings.T) ** 2)) / (N * T)
    Vr = float(np.sum((ref["Z"] - ref["F"] @ ref["L"].T) ** 2)) / (N * T)
    fig = {
        "eig": rel(res.eigenvalues, ref["ev"]),
        "V": abs(Vg - Vr) / Vr,
        "err": abs(res.error - ref["err"]) / ref["err"] if ref["err"] > 0 else abs(res.error),
        "angle": R.max_principal_angle(res.factors, ref["F"]),
        "Z": float(np.max(np.abs(res.x_standardized - ref["Z"]))) / big,
        "X2": float(np.max(np.abs(res.x_completed - ref["X2"]))) / big,
        "mu": float(np.max(np.abs(res.mean - ref["mu"]))) / big,
        "sd": float(np.max(np.abs(res.std - ref["sd"]))) / big,
    }
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert np.array_equal(res.x_completed[obs], X[obs])
    assert res.n_missing == ref["n_missing"] == int((~obs).sum())
    assert not np.isnan(res.x_completed).any() and not np.isnan(res.x_standardized).any()
    for k, v in fig.items():
        assert v < (ANGLE if k == "angle" else RTOL), (label, k, v)
    return fig


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_fixed_iteration_count(dfm, ctx, shape):
    """tol = 0, max_iter = 6, r = 3: six iterations, no early stop."""
    X, _ = R.make_panel(*shape)
    ref = R.cached(*shape, tol=0.0, max_iter=6)
    res = dfm.em_factors(X, 3, tol=0.0, max_iter=6, ctx=ctx)
    assert res.iterations == 6 and not res.converged
    check(res, ref, X, f"fixed {shape}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_convergence(dfm, ctx, shape):
    """tol = 1e-6: converged after the reference's iteration count, and one more
    reference step from the device's fixed point moves C by at most tol."""
    X, _ = R.make_panel(*shape)
    ref = R.cached(*shape)
    res = dfm.em_factors(X, 3, ctx=ctx)
    print("iterations", res.iterations, ref["iterations"], "err", res.error, ref["err"])
    assert res.converged and ref["converged"]
    assert res.iterations == ref["iterations"]
    assert res.error <= 1e-6
    check(res, ref, X, f"converged {shape}")
    nxt = R.em_step(X, res.factors @ res.loadings.T, res.mean, res.std, 3)
    print("next step err", nxt["err"])
    assert nxt["err"] <= 1e-6


def test_max_iter_reached(dfm, ctx):
    X, _ = R.make_panel(60, 40)
    res = dfm.em_factors(X, 3, max_iter=3, ctx=ctx)   # a DFMError would be a non-zero return code
    assert not res.converged and res.iterations == 3
    assert res.error == pytest.approx(R.cached(60, 40)["errs"][2], rel=RTOL)


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_selection(dfm, ctx, shape):
    """r re-selected every iteration by ICp2 over 1..8: r^ = 3, 3, 2, 3."""
    X, _ = R.make_panel(*shape)
    ref = R.cached(*shape, r=None)
    assert len(set(ref["rs"])) == 1
    assert ref["r"] == (2 if shape == (33, 33) else 3)
    res = dfm.em_factors(X, None, "ICp2", kmax=8, ctx=ctx)
    assert res.number_of_factors == ref["r"]
    assert res.iterations == ref["iterations"] and res.converged
    check(res, ref, X, f"selected {shape}")


def test_selection_rejects_pcp_and_wide_kmax(dfm, ctx):
    X, _ = R.make_panel(60, 40)
    for name in ("PCp1", "PCp2", "PCp3"):
        with pytest.raises(dfm.DFMError) as e:
            dfm.em_factors(X, None, name, kmax=8, ctx=ctx)
        assert e.value.code == -3
    wide = np.random.default_rng(5).standard_normal((60, 56))   # ceil(m/2) = 28 >= 26: a 34-column block
    wide[3, 4] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.em_factors(wide, None, "ICp2", kmax=26, ctx=ctx)
    assert e.value.code == -7


def test_standardize_false(dfm, ctx):
    X, _ = R.make_panel(60, 40)
    ref = R.cached(60, 40, standardize=False)
    res = dfm.em_factors(X, 3, standardize=False, ctx=ctx)
    assert res.iterations == ref["iterations"] and res.converged
    assert np.all(res.mean == 0.0) and np.all(res.std == 1.0)
    assert np.array_equal(res.x_standardized, res.x_completed)
    check(res, ref, X, "standardize=False")


def test_no_missing_entry(dfm, ctx):
    """A complete panel: one iteration that changes nothing, the plain z-score
    and the plain fit bit for bit."""
    _, full = R.make_panel(60, 40)
    y, w = R.regression_inputs(60)
    res = dfm.em_factors(full, 3, ctx=ctx)
    assert res.iterations == 1 and res.error == 0.0 and res.converged and res.n_missing == 0
    Z = dfm.normalize(full, ctx=ctx)
    assert np.array_equal(res.x_standardized, Z)
    assert np.array_equal(res.x_completed, full)
    m = dfm.DynamicFactorModel_em(y, w, full, 3, ctx=ctx)
    p = dfm.DynamicFactorModel(y, w, Z, 3, "ICp2", ctx=ctx)
    assert np.array_equal(m.em.x_standardized, Z)
    for a, b in ((m.eigenvalues, p.eigenvalues), (m.F, p.F), (m.loadings[0], p.loadings[0]),
                 (m.coefficients, p.coefficients), (m.t_stats, p.t_stats)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", [(60, 40), (40, 72)], ids=["60x40", "40x72"])
def test_model_contract(dfm, ctx, shape):
    """DynamicFactorModel_em is the plain fit of its completed panel, and the
    bootstrap and the sup-Chow sweep serve it as they serve that fit."""
    T, N = shape
    X, _ = R.make_panel(T, N)
    y, w = R.regression_inputs(T)
    m = dfm.DynamicFactorModel_em(y, w, X, None, "ICp2", kmax=8, ctx=ctx)
    e = dfm.em_factors(X, None, "ICp2", kmax=8, ctx=ctx)
    assert np.array_equal(m.em.x_standardized, e.x_standardized)     # the host z-score has the device's bits
    assert np.array_equal(m.em.x_completed, e.x_completed)
    assert np.array_equal(m.em.mean, e.mean) and np.array_equal(m.em.std, e.std)
    assert (m.em.iterations, m.em.error, m.em.converged, m.em.n_missing) == \
        (e.iterations, e.error, e.converged, e.n_missing)
    assert m.em.number_of_factors == m.number_of_factors == e.number_of_factors == 3
    p = dfm.DynamicFactorModel(y, w, m.em.x_standardized, m.em.number_of_factors, "ICp2", ctx=ctx)
    for a, b in ((m.eigenvalues, p.eigenvalues), (m.F, p.F), (m.loadings[0], p.loadings[0]),
                 (m.coefficients, p.coefficients), (m.t_stats, p.t_stats), (m.residuals, p.residuals),
                 (m.factor_residuals, p.factor_residuals)):
        assert np.array_equal(a, b)
    assert m.V == p.V and m.number_of_factors_criterion_value == p.number_of_factors_criterion_value
    sm, sp = dfm.chow_sweep(m), dfm.chow_sweep(p)
    for s in ("LR", "LM", "Wald"):
        assert np.array_equal(sm.sup[s], sp.sup[s], equal_nan=True)
        assert np.array_equal(sm.argsup[s], sp.argsup[s])
    idx, eta = dfm.draw_wild(np.random.default_rng(3), 8, T)
    stats = [dfm.Stat.V(), dfm.Stat.criterion(), dfm.Stat.eigenvalue(1)]
    assert np.array_equal(dfm.wild_bootstrap(m, 8, stats, idx=idx, eta=eta),
                          dfm.wild_bootstrap(p, 8, stats, idx=idx, eta=eta))


def test_repeatability_and_device_input(dfm, ctx):
    import torch
    X, _ = R.make_panel(67, 19)
    a = dfm.em_factors(X, 3, ctx=ctx)
    b = dfm.em_factors(X, 3, ctx=ctx)
    xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()   # column-major in HBM
    d = dfm.em_factors(xd, 3, ctx=ctx)
    for o in (b, d):
        assert (o.iterations, o.error, o.number_of_factors) == (a.iterations, a.error, a.number_of_factors)
        for f in ("x_standardized", "x_completed", "mean", "std", "factors", "loadings", "eigenvalues"):
            assert np.array_equal(getattr(a, f), getattr(o, f)), f


def test_errors(dfm, ctx):
    X, _ = R.make_panel(60, 40)
    y, w = R.regression_inputs(60)
    bad = X.copy()
    bad[:, 7] = np.nan
    bad[11, 7] = 1.5
    with pytest.raises(dfm.DFMError) as e:
        dfm.em_factors(bad, 3, ctx=ctx)
    assert e.value.code == -8 and "column 7" in str(e.value)
    flat = X.copy()
    flat[:, 5] = 2.0
    with pytest.raises(dfm.DFMError) as e:
        dfm.em_factors(flat, 3, ctx=ctx)
    assert e.value.code == -8 and "column 5" in str(e.value)
    yn = y.copy()
    yn[4] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.DynamicFactorModel_em(yn, w, X, 3, ctx=ctx)
    assert e.value.code == -2
    # a plain model is not an EM model
    p = dfm.DynamicFactorModel(y, w, dfm.normalize(R.make_panel(60, 40)[1], ctx=ctx), 3, ctx=ctx)
    assert ctx.lib.dfm_model_em_read(p.handle, None, None, None) == -1


def test_clone_stays_an_em_model(dfm, ctx):
    X, _ = R.make_panel(67, 19)
    y, w = R.regression_inputs(67)
    m = dfm.DynamicFactorModel_em(y, w, X, 3, ctx=ctx)
    other = dfm.Context(0)
    c = dfm.clone_model(m, other)
    X2 = np.zeros((67, 19), order="F")
    mu, sd = np.zeros(19), np.zeros(19)
    assert other.lib.dfm_model_em_read(c.handle, X2.ctypes.data_as(dfm._lib.c_double_p), dfm._lib.ptr(mu),
                                       dfm._lib.ptr(sd)) == 0
    assert np.array_equal(X2, m.em.x_completed)
    assert np.array_equal(mu, m.em.mean) and np.array_equal(sd, m.em.std)
    del c
    other.close()


def test_fully_missing_row(dfm, ctx):
    X, _ = R.make_panel(60, 40)
    X = X.copy()
    X[17, :] = np.nan
    ref = R.em(X, r=3, tol=0.0, max_iter=6)
    res = dfm.em_factors(X, 3, tol=0.0, max_iter=6, ctx=ctx)
    assert res.iterations == 6
    check(res, ref, X, "missing row")
