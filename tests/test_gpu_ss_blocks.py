"""Factor blocks on the device (dfm_ss_em_blocks, dfm_ss_fit_blocks through
ss_em(factor_blocks=, block_members=) and DynamicFactorModel_ss(...)) against
the NumPy reference tests/ss_blocks_reference.py, whose M-step solves the
restricted normal equations with numpy.linalg.solve on the index sets.

Bars.  The EM fed from the reference's starts: every array within RTOL =
1e-10 of the reference array's largest magnitude and the loglik path 1e-10
relative, the bar of tests/test_gpu_ss_em.py (the arithmetic is the same).
The fit (the device's own static EM and principal components underneath): the
project's end-to-end E2E = 1e-8 on quantities that do not depend on the
factors' signs.  Restricted positions are exactly 0.0; batch against single
calls, repeated runs, device input, the horizon and the unrestricted dispatch
are bit-for-bit."""
import numpy as np
import pytest

import ss_blocks_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
E2E = 1e-8
PARAMS = (("loadings", "L"), ("sigma2", "sigma2"), ("A", "A"), ("Q", "Q"), ("a0", "a0"), ("P0", "P0"))
OUTPUTS = ("filtered", "smoothed", "smoothed_cov")
FIELDS = tuple(k for k, _ in PARAMS) + OUTPUTS + ("loglik", "n_observed", "loglik_path", "iterations", "converged",
                                                  "criterion")
FIT_FIELDS = ("sigma2", "A", "Q", "P0", "loadings", "filtered", "smoothed", "smoothed_cov", "x_smoothed", "x_completed",
              "forecast")


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


def call(dfm, ctx, i, X, start, low, member, **kw):
    T, N, sizes, p, w, mixed, everyone = R.CASES[i]
    mf = dict(low_freq=low, agg_weights=w) if mixed else {}
    return dfm.ss_em(X, *start, factor_blocks=sizes, block_members=None if everyone else member, ctx=ctx, **mf, **kw)


def same(a, b, fields=FIELDS):
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


# ------------------------------------------------------------------ 1, 2: the EM
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_em_against_the_reference_with_exact_zeros(dfm, ctx, i):
    T, N, sizes, p, w, mixed, everyone = R.CASES[i]
    X, start, low, member, ref = R.em_case(i)
    res = call(dfm, ctx, i, X, start, low, member, tol=0.0, max_iter=R.EM_ITER, horizon=2)
    fig = {k: big(getattr(res, k) - ref[rk]) / big(ref[rk]) for k, rk in PARAMS}
    fig["path"] = float(np.max(np.abs(res.loglik_path - ref["path"]) / np.abs(ref["path"])))
    for k in OUTPUTS + (("smoothed_agg",) if mixed else ()):
        fig[k] = big(getattr(res, k) - ref[k]) / big(ref[k])
    print(R.CASE_IDS[i], "gains", np.diff(res.loglik_path))
    assert res.iterations == R.EM_ITER and res.n_observed == ref["nobs"] and res.factor_blocks == tuple(sizes)
    assert (np.diff(res.loglik_path) > 0).all()
    free = R.free_matrix(sizes, member)
    inside = R.same_block(sizes, p)
    assert (res.loadings[~free] == 0.0).all() and (res.A[~inside] == 0.0).all()
    assert (res.Q[~R.same_block(sizes)] == 0.0).all()
    report(R.CASE_IDS[i], fig, RTOL)


def test_the_restriction_is_what_the_test_sees(dfm, ctx):
    X, start, low, member, ref = R.em_case(0)
    T, N, sizes, p, w, _, _ = R.CASES[0]
    free = dfm.ss_em(X, *start, low_freq=low, agg_weights=w, tol=0.0, max_iter=R.EM_ITER, ctx=ctx)
    off = np.abs(free.loadings[~R.free_matrix(sizes, member)]).max()
    print("unrestricted max |lambda| at the restricted positions", off)
    assert off > 0.1 and free.factor_blocks is None


# ------------------------------------------------------------------ 3: the batch
def test_batch_stops_each_panel_at_its_own_time_and_equals_the_single_calls(dfm, ctx):
    K = len(R.BATCH_SEEDS)
    cases = [R.batch_case(k) for k in range(K)]
    T, N, sizes, p, w, _, _ = R.CASES[0]
    low, member = cases[0][2], cases[0][3]
    its = [c[4]["iterations"] for c in cases]
    assert len(set(its)) > 1
    kw = dict(low_freq=low, agg_weights=w, factor_blocks=sizes, block_members=member, tol=R.BATCH_TOL, max_iter=40,
              ctx=ctx)
    starts = [np.stack([c[1][j] for c in cases]) for j in range(4)]
    batch = dfm.ss_em(np.stack([c[0] for c in cases]), *starts, **kw)
    print("iterations", batch.iterations, "reference", its)
    assert list(batch.iterations) == its and batch.converged.all()
    for k, c in enumerate(cases):
        one = dfm.ss_em(c[0], *c[1], **kw)
        for f in FIELDS + ("smoothed_agg",):
            assert np.array_equal(getattr(batch, f)[k], getattr(one, f), equal_nan=True), (k, f)
        assert abs(one.loglik - c[4]["loglik"]) < RTOL * abs(c[4]["loglik"])


# ------------------------------------------------------------------ 4: no restriction
def test_one_all_member_block_is_the_old_call(dfm, ctx):
    X, start, low, member, _ = R.em_case(0)
    T, N, sizes, p, w, _, _ = R.CASES[0]
    r = sum(sizes)
    dense = tuple(np.where(a == 0.0, 0.1, a) if j in (0, 2) else a for j, a in enumerate(start))   # no zeros needed
    kw = dict(tol=0.0, max_iter=3, horizon=1, ctx=ctx)
    for mf in (dict(), dict(low_freq=low, agg_weights=w)):
        old = dfm.ss_em(X, *dense, **mf, **kw)
        for members in (None, np.ones((N, 1), dtype=bool)):
            new = dfm.ss_em(X, *dense, factor_blocks=(r,), block_members=members, **mf, **kw)
            same(old, new, FIELDS + (("smoothed_agg",) if mf else ()))
            assert new.factor_blocks == (r,)


@pytest.mark.parametrize("method", ["two-step", "ml"])
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mf"])
def test_one_all_member_block_is_the_old_fit(dfm, ctx, method, mixed):
    X, low, _ = R.make_fit_panel((1, 1, 1), mixed)
    mf = dict(low_freq=low, agg_weights=R.FIT_W) if mixed else {}
    kw = dict(lags=1, horizon=R.FIT_HORIZON, tol=0.0, max_iter=4, method=method, ml_tol=0.0, ml_max_iter=2, ctx=ctx, **mf)
    old = dfm.DynamicFactorModel_ss(X, 3, **kw)
    new = dfm.DynamicFactorModel_ss(X, None, factor_blocks=(3,), **kw)
    same(old, new, FIT_FIELDS + (("loglik_path", "a0") if method == "ml" else ()))
    assert old.loglik == new.loglik and new.factor_blocks == (3,) and old.factor_blocks is None


# ------------------------------------------------------------------ 5: the fit
def run_fit(dfm, ctx, X, sizes, member, low, method, **kw):
    mf = dict(low_freq=low, agg_weights=R.FIT_W) if low is not None else {}
    return dfm.DynamicFactorModel_ss(X, sum(sizes), lags=1, horizon=R.FIT_HORIZON, tol=0.0, max_iter=R.FIT_EM_ITER,
                                     method=method, ml_tol=0.0, ml_max_iter=R.FIT_ML_ITER, factor_blocks=sizes,
                                     block_members=member, ctx=ctx, **mf, **kw)


@pytest.mark.parametrize("method", ["two-step", "ml"])
@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mf"])
@pytest.mark.parametrize("sizes", R.FIT_SIZES, ids=["b111", "b211"])
def test_fit_against_the_numpy_chain(dfm, ctx, sizes, mixed, method):
    ref = R.fit_case(sizes, mixed, method)
    X, member = ref["X"], ref["member"]
    T, N = X.shape
    fit = run_fit(dfm, ctx, X, sizes, member, ref["low"] if mixed else None, method)
    obs = ~np.isnan(X)
    fig = {"loglik": abs(fit.loglik - ref["loglik"]) / abs(ref["loglik"]),
           "x_smoothed": big(fit.x_smoothed - ref["x_smoothed"]) / big(ref["x_smoothed"]),
           "x_completed": big(fit.x_completed - ref["x_completed"]) / big(ref["x_completed"]),
           "forecast": big(fit.forecast - ref["forecast"]) / big(ref["forecast"])}
    if method == "ml":
        fig["sigma2"] = big(fit.sigma2 - ref["sigma2"]) / big(ref["sigma2"])
    assert np.array_equal(fit.x_completed[obs], X[obs])
    assert fit.forecast.shape == (R.FIT_HORIZON, N) and fit.factor_blocks == tuple(sizes)
    assert (fit.loadings[~R.free_matrix(sizes, member)] == 0.0).all()
    assert (fit.A[~R.same_block(sizes)] == 0.0).all() and (fit.Q[~R.same_block(sizes)] == 0.0).all()
    if method == "ml":
        assert fit.ml_iterations == R.FIT_ML_ITER and (np.diff(fit.loglik_path) > 0).all()
    report(f"{sizes} {'mf' if mixed else 'plain'} {method}", fig, E2E)


# ------------------------------------------------------------------ 6: repeatability
def test_repeatable_device_input_and_horizon(dfm, ctx):
    import torch
    X, start, low, member, _ = R.em_case(0)
    kw = dict(tol=0.0, max_iter=3)
    a = call(dfm, ctx, 0, X, start, low, member, **kw)
    same(a, call(dfm, ctx, 0, X, start, low, member, **kw), FIELDS + ("smoothed_agg",))
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    same(a, call(dfm, ctx, 0, Xd, start, low, member, **kw), FIELDS + ("smoothed_agg",))
    h = 3
    e0 = call(dfm, ctx, 0, X, start, low, member, tol=0.0, max_iter=0, horizon=h)
    e1 = call(dfm, ctx, 0, np.vstack([X, np.full((h, X.shape[1]), np.nan)]), start, low, member, tol=0.0, max_iter=0)
    for f in ("smoothed", "smoothed_cov", "smoothed_agg", "loglik"):
        assert np.array_equal(getattr(e0, f), getattr(e1, f)), f
    assert np.array_equal(e0.filtered, e1.filtered[:X.shape[0]])
    ref = R.fit_case((2, 1, 1), True, "ml")
    f0 = run_fit(dfm, ctx, ref["X"], (2, 1, 1), ref["member"], ref["low"], "ml")
    f1 = run_fit(dfm, ctx, ref["X"], (2, 1, 1), ref["member"], ref["low"], "ml")
    same(f0, f1, FIT_FIELDS + ("loglik_path", "a0", "smoothed_agg"))


# ------------------------------------------------------------------ 7: errors
def test_errors_name_the_offender(dfm, ctx):
    X, start, low, member, _ = R.em_case(4)   # plain, blocks (1, 1, 1)
    T, N, sizes, p, w, _, _ = R.CASES[4]
    L, sg, A, Q = start

    def refused(code, words, *, st=start, fb=sizes, bm=member, x=X):
        with pytest.raises(dfm.DFMError) as e:
            dfm.ss_em(x, *st, factor_blocks=fb, block_members=bm, max_iter=1, ctx=ctx)
        assert e.value.code == code and all(wd in str(e.value) for wd in words), str(e.value)

    refused(-2, ["sum"], fb=(1, 1))
    refused(-2, ["size"], fb=(1, 0, 2), bm=member)
    refused(-2, ["16"], fb=(1,) * 17, bm=np.ones((N, 17), dtype=bool), st=(np.zeros((N, 17)), sg, np.eye(17), np.eye(17)))
    m = member.copy()
    m[5] = False
    refused(-2, ["column 5", "no block"], bm=m)
    m = member.copy()
    m[:, 2] = False
    m[:, 1] = True
    refused(-2, ["block 2", "no member"], bm=m)
    i, j = np.argwhere(~R.free_matrix(sizes, member))[0]
    L2 = L.copy()
    L2[i, j] = 0.25
    refused(-2, ["lambda", f"[{i}, {j}]"], st=(L2, sg, A, Q))
    A2 = A.copy()
    A2[0, 2] = 0.1
    refused(-2, ["A[0, 2]"], st=(L, sg, A2, Q))
    Q2 = Q.copy()
    Q2[1, 0] = Q2[0, 1] = 0.05
    refused(-2, ["Q[1, 0]"], st=(L, sg, A, Q2))
    # the raw struct: NULL fields, and the limits with blocks that restrict
    lib, C = dfm._lib, __import__("ctypes")
    par, _, keep = dfm.api._ss_param_block(N, L, sg, A, Q, None, None)
    spec = lib.dfm_ss_em_spec(1, 1, 0, 0, 0.0)
    out = lib.dfm_ss_em_out()
    Xc = np.asfortranarray(X)
    bad = lib.dfm_ss_blocks(3, None, None)
    args = (ctx.h, Xc.ctypes.data_as(C.c_void_p), 1, T, N, T, T * N, C.byref(par), 1, None)
    assert ctx.lib.dfm_ss_em_blocks(*args, C.byref(bad), C.byref(spec), C.byref(out), None) == -2
    assert ctx.lib.dfm_ss_em_blocks(*args, None, C.byref(spec), C.byref(out), None) == -2
    big_r = 17
    mem17 = np.ones((N, 2), dtype=bool)
    mem17[0, 1] = False
    refused(-7, ["r <= 16"], fb=(16, 1), bm=mem17, st=(np.zeros((N, big_r)), sg, np.eye(big_r) * 0.5, np.eye(big_r)))
    del keep
    # the fit: a block with too few members, a selected r
    Xf, _, memf = R.make_fit_panel((2, 1, 1), False)
    few = memf.copy()
    few[:, 0] = False
    few[0, 0] = True
    few[:, 1] = True
    with pytest.raises(dfm.DFMError) as e:
        dfm.DynamicFactorModel_ss(Xf, 4, factor_blocks=(2, 1, 1), block_members=few, ctx=ctx)
    assert e.value.code == -11 and "block 0" in str(e.value)
    sp = lib.dfm_em_spec(0, 1, 8, 1, 5, 0, 1e-6)
    sizes32 = np.array([2, 1, 1], dtype=np.int32)
    mem8 = np.asfortranarray(memf.astype(np.uint8))
    bs = lib.dfm_ss_blocks(3, sizes32.ctypes.data_as(C.POINTER(C.c_int32)), mem8.ctypes.data_as(lib.c_uint8_p))
    Xfc = np.asfortranarray(Xf)
    fo, info = lib.dfm_ss_fit_out(), lib.dfm_em_info()
    rc = ctx.lib.dfm_ss_fit_blocks(ctx.h, Xfc.ctypes.data_as(C.c_void_p), Xf.shape[0], Xf.shape[1], Xf.shape[0],
                                   C.byref(sp), 1, C.byref(spec), None, C.byref(bs), 0, C.byref(info), C.byref(fo), None,
                                   None, None, None)
    assert rc == -3
