"""CPU checks of the mixed-frequency smoother: the NumPy reference against
itself (tests/ss_mf_reference.py: the textbook filter on explicit N x s loading
rows against the header's two updates per row on the collapsed moments of each
class), the degenerate weight, forecast rows, and the Python argument checks
that are made before anything touches the device."""
import numpy as np
import pytest

import ss_mf_reference as R
import ss_reference as S

IDS = R.CASE_IDS


def big(a):
    return float(np.max(np.abs(a)))


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_class_updates_equal_dense_filter(i):
    """Two r-dimensional updates per row against the dense filter: loglik 1e-12
    relative, the arrays 1e-12 of their largest magnitude (measured <= 3e-14)."""
    X, L, sigma2, A, Q, low, w, a = R.case(i)
    b = R.smooth(X, L, sigma2, A, Q, low, w, method="classes")
    fig = {"loglik": abs(a["loglik"] - b["loglik"]) / abs(a["loglik"])}
    for k in ("filtered", "smoothed", "smoothed_cov", "smoothed_agg", "state_cov"):
        fig[k] = big(a[k] - b[k]) / big(a[k])
    print(IDS[i], " ".join(f"{k}={v:.2e}" for k, v in fig.items()),
          "cond", f"{max(np.linalg.cond(P) for P in a['Pp']):.0f}")
    assert a["nobs"] == b["nobs"] == int((~np.isnan(X)).sum())
    for k, v in fig.items():
        assert v < 1e-12, (IDS[i], k, v)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_cases_reach_their_paths(i):
    """Every case has a row with only low-frequency entries, a row with none
    at all, rows with both classes, and low-frequency entries at t % 3 == 2 only."""
    X, _, _, _, _, low, _, _ = R.case(i)
    o = ~np.isnan(X)
    assert o[5, low].all() and not o[5, ~low].any() and not o[7].any()
    assert (o[:, low].any(axis=1) & o[:, ~low].any(axis=1)).any()
    assert not o[np.arange(X.shape[0]) % 3 != 2][:, low].any()


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_cases_are_well_conditioned(i):
    """Every input perturbed by 1e-12 relative moves the reference's outputs by
    less than 1e-11 of their largest magnitude (measured <= 3.1e-12): the
    device's 1e-10 bar measures the device, not the case."""
    X, L, sigma2, A, Q, low, w, ref = R.case(i)
    rng = np.random.default_rng(i)

    def pt(a):
        return np.asarray(a) * (1.0 + 1e-12 * rng.choice([-1.0, 1.0], size=np.shape(a)))
    b = R.smooth(pt(X), pt(L), pt(sigma2), pt(A), pt(Q), low, tuple(pt(w)))
    fig = {k: big(ref[k] - b[k]) / big(ref[k]) for k in ("filtered", "smoothed", "smoothed_cov", "smoothed_agg")}
    fig["loglik"] = abs(ref["loglik"] - b["loglik"]) / abs(ref["loglik"])
    print(IDS[i], " ".join(f"{k}={v:.1e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < 1e-11, (IDS[i], k, v)


def test_restricted_em_raises_the_likelihood_and_start_values_solve_the_normal_equations():
    X, start, low, w, res = R.em_case(1)
    assert (np.diff(res["path"]) > 0).all() and res["A"].shape == (3, 6) and res["P0"].shape == (9, 9)
    ref = R.fit_case("two-step")
    em0, T, nw = ref["em"], ref["X"].shape[0], len(ref["w"])
    Zm = np.where(np.isnan(ref["X"]), np.nan, em0["Z"])
    L, sg = R.start_values(Zm, em0["F"], em0["L"], np.ones(Zm.shape[1]), ref["low"], ref["w"])
    ft = sum(ref["w"][k] * em0["F"][nw - 1 - k:T - k] for k in range(nw))
    for i in np.flatnonzero(ref["low"]):
        o = ~np.isnan(Zm[nw - 1:, i])
        assert big(ft[o].T @ (Zm[nw - 1:, i][o] - ft[o] @ L[i])) < 1e-10   # residuals orthogonal to the regressor
    assert np.array_equal(L[~ref["low"]], em0["L"][~ref["low"]]) and (sg[~ref["low"]] == 1.0).all()


def test_unit_weight_is_the_plain_model():
    """w = (1) with any mask: the loading rows are the plain ones."""
    X, L, sigma2, A, Q, low, _, _ = R.case(1)
    a = R.smooth(X, L, sigma2, A, Q, low, (1.0,))
    b = S.smooth(X, L, sigma2, A, Q)
    assert a["loglik"] == b["loglik"]
    for k in ("filtered", "smoothed", "smoothed_cov"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["smoothed_agg"], b["smoothed"])


def test_smoothed_aggregate_is_the_weighted_sum_of_smoothed_factors():
    """Z_l a_t|T = sum_k w_k f_{t-k}|T for t >= n_w - 1 (fixed-interval smoothing
    of a lagged state element equals the smoothed factor of that date)."""
    X, L, sigma2, A, Q, low, w, a = R.case(0)
    sm, nw = a["smoothed"], len(w)
    T = sm.shape[0]
    direct = sum(w[k] * sm[nw - 1 - k:T - k] for k in range(nw))
    assert big(a["smoothed_agg"][nw - 1:] - direct) < 1e-12 * big(direct)


def test_forecast_rows_are_appended_missing_rows():
    X, L, sigma2, A, Q, low, w, base = R.case(1)
    ext = R.smooth(X, L, sigma2, A, Q, low, w, horizon=3)
    app = R.smooth(np.vstack([X, np.full((3, X.shape[1]), np.nan)]), L, sigma2, A, Q, low, w)
    assert ext["loglik"] == base["loglik"] == app["loglik"]
    assert np.array_equal(ext["smoothed_agg"], app["smoothed_agg"]) and ext["smoothed_agg"].shape[0] == X.shape[0] + 3


def test_python_argument_checks_need_no_device(dfm):
    X, L, sigma2, A, Q, low, w, _ = R.case(4)
    with pytest.raises(dfm.DFMError) as e:   # a mask of the wrong length
        dfm.kalman_smoother(X, L, sigma2, A, Q, low_freq=low[:-1], agg_weights=w)
    assert e.value.code == -2
    with pytest.raises(ValueError):
        dfm.kalman_smoother(X, L, sigma2, A, Q, agg_weights=w)
    with pytest.raises(ValueError):
        dfm.kalman_smoother(X, L, sigma2, A, Q, low_freq=low)
    assert dfm.AGG_FLOW == (1, 2, 3, 2, 1) and dfm.AGG_MEAN == (1 / 3, 1 / 3, 1 / 3)
