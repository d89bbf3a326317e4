"""The smoother with AR(1) idiosyncratic terms on the device (dfm_ss_smooth_ar
through kalman_smoother(idio_ar=)) against the dense filter on the state
(alpha_t, e_t) of tests/ss_ar_reference.py: reference (a), the run-wise model
the header states, on every shape, and reference (b), the exact model, on the
single-run shapes 1-4.

Bars.  filtered, smoothed, smoothed_cov within 1e-10 of each reference array's
largest magnitude and loglik 1e-10 relative — the project's smoother bar; on
the CPU the quasi-differenced collapsed recursion and the dense filter differ by
at most 2e-13 at these shapes (tests/test_ss_ar_host.py).  n_observed equal.
Batch against single calls and run to run: bit for bit.  An all-zero idio_ar
against the plain smoother at p = 2: 1e-12 relative."""
import numpy as np
import pytest

import ss_ar_reference as AR
import ss_reference as SR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
IDS = [f"{T}x{N}r{r}p{p}h{h}" for T, N, r, p, h in AR.CASES]


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def figures(res, ref):
    return {"loglik": abs(res.loglik - ref["loglik"]) / abs(ref["loglik"]),
            "filtered": big(res.filtered - ref["filtered"]) / big(ref["filtered"]),
            "smoothed": big(res.smoothed - ref["smoothed"]) / big(ref["smoothed"]),
            "cov": big(res.smoothed_cov - ref["smoothed_cov"]) / big(ref["smoothed_cov"])}


def report(label, fig, bar):
    """Print every figure, then assert each against its bar."""
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < bar, (label, k, v)


@pytest.mark.parametrize("k", range(5), ids=IDS)
def test_smoother_against_the_runwise_reference(dfm, ctx, k):
    X, L, sigma2, rho, A, Q, h, _ = AR.case(k)
    assert np.max(np.abs(rho)) <= 0.9 and (rho > 0).any() and (rho < 0).any() and (rho == 0).any()
    ref = AR.case_reference(k, True)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=h, idio_ar=rho, ctx=ctx)
    assert res.n_observed == ref["nobs"] == int((~np.isnan(X)).sum())
    assert res.smoothed.shape == ref["smoothed"].shape and res.filtered.shape == ref["filtered"].shape
    assert res.smoothed_cov.shape == ref["smoothed_cov"].shape
    report(f"run-wise {IDS[k]}", figures(res, ref), RTOL)


@pytest.mark.parametrize("k", range(4), ids=IDS[:4])
def test_smoother_against_the_exact_reference_on_single_runs(dfm, ctx, k):
    X, L, sigma2, rho, A, Q, h, single = AR.case(k)
    assert single
    ref = AR.case_reference(k, False)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=h, idio_ar=rho, ctx=ctx)
    assert res.n_observed == ref["nobs"]
    report(f"exact {IDS[k]}", figures(res, ref), RTOL)


def test_tile_boundary_pattern_is_what_the_issue_asks():
    """Shape 2: a run that ends at row 63, a start entry at row 64, a pair over 63 | 64."""
    X = AR.case(1)[0]
    m = ~np.isnan(X)
    assert m[63, 0] and not m[64:, 0].any()
    assert m[64, 1] and not m[:64, 1].any()
    assert m[63, 2] and m[64, 2]
    X4 = AR.case(3)[0]
    assert np.isnan(X4[-1, 255]) and np.isnan(X4[-1, 256]) and not np.isnan(X4[0, 255])
    X5 = AR.case(4)[0]
    assert np.isnan(X5[14]).all() and not np.isnan(X5[15]).any()


def test_smoother_with_a0_and_P0_of_the_padded_state(dfm, ctx):
    X, L, sigma2, rho, A, Q, h, _ = AR.case(1)   # p = 1: the state is padded to two lags
    s = 2 * L.shape[1]
    a0 = np.linspace(-1.0, 1.0, s)
    P0 = 2.0 * np.eye(s) + 0.5
    ref = AR.dense(X, L, sigma2, rho, A, Q, a0, P0)
    res = dfm.kalman_smoother(X, L, sigma2, A, Q, a0=a0, P0=P0, idio_ar=rho, ctx=ctx)
    report("a0/P0", figures(res, ref), RTOL)


def test_batch_is_the_single_calls_bit_for_bit(dfm, ctx):
    X, L, sigma2, rho, A, Q, h, _ = AR.case(4)
    rng = np.random.default_rng(5)
    panels = np.stack([X, np.where(rng.uniform(size=X.shape) < 0.2, np.nan, X),
                       np.where(rng.uniform(size=X.shape) < 0.5, np.nan, X)])
    kw = dict(horizon=h, idio_ar=rho, ctx=ctx)
    batch = dfm.kalman_smoother(panels, L, sigma2, A, Q, **kw)
    again = dfm.kalman_smoother(panels, L, sigma2, A, Q, **kw)
    for f in ("filtered", "smoothed", "smoothed_cov", "loglik", "n_observed"):
        assert np.array_equal(getattr(batch, f), getattr(again, f)), f
    for b in range(3):
        one = dfm.kalman_smoother(panels[b], L, sigma2, A, Q, **kw)
        for f in ("filtered", "smoothed", "smoothed_cov", "loglik", "n_observed"):
            assert np.array_equal(getattr(batch, f)[b], getattr(one, f)), (b, f)


def test_zero_rho_is_the_plain_smoother(dfm, ctx):
    """At p = 2 the padded state is the plain one; rho = 0 runs the AR path."""
    X, L, sigma2, A, Q = SR.make_synthetic(40, 24, 3, 2)
    plain = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=2, ctx=ctx)
    ar = dfm.kalman_smoother(X, L, sigma2, A, Q, horizon=2, idio_ar=np.zeros(24), ctx=ctx)
    assert ar.n_observed == plain.n_observed
    ref = dict(loglik=plain.loglik, filtered=plain.filtered, smoothed=plain.smoothed, smoothed_cov=plain.smoothed_cov)
    report("rho = 0", figures(ar, ref), 1e-12)


def test_return_codes(dfm, ctx):
    X, L, sigma2, rho, A, Q, h, _ = AR.case(0)
    N = X.shape[1]
    with pytest.raises(dfm.DFMError) as e:
        dfm.kalman_smoother(np.zeros((6, 12)), np.ones((12, 9)), np.ones(12), 0.5 * np.eye(9), np.eye(9),
                            idio_ar=np.zeros(12), ctx=ctx)
    assert e.value.code == -7
    bad = rho.copy()
    bad[2] = 1.0
    with pytest.raises(dfm.DFMError) as e:
        dfm.kalman_smoother(X, L, sigma2, A, Q, idio_ar=bad, ctx=ctx)
    assert e.value.code == -2 and "column 2" in str(e.value)
    bad[2] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.kalman_smoother(X, L, sigma2, A, Q, idio_ar=bad, ctx=ctx)
    assert e.value.code == -12
    with pytest.raises(ValueError, match="not built yet"):
        dfm.kalman_smoother(X, L, sigma2, A, Q, idio_ar=rho, low_freq=np.zeros(N, dtype=bool),
                            agg_weights=dfm.AGG_MEAN, ctx=ctx)
    with pytest.raises(ValueError):
        dfm.kalman_smoother(X, L, sigma2, A, Q, idio_ar=rho[:2], ctx=ctx)
    for kw in (dict(low_freq=np.zeros(N, dtype=bool), agg_weights=dfm.AGG_MEAN), dict(factor_blocks=[1]),
               dict(method="ml")):
        with pytest.raises(ValueError, match="not built yet"):
            dfm.DynamicFactorModel_ss(X, 1, idiosyncratic_ar1=True, ctx=ctx, **kw)
