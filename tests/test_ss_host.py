"""CPU checks of the state-space pass: the NumPy reference against itself
(tests/ss_reference.py: the textbook filter on the dense innovation covariance
against the header's collapsed arrangement; forecast rows as appended NaN
rows), and dfm_ss_stationary_cov through the loaded library against the
Kronecker solve.  No device work."""
import numpy as np
import pytest

import ss_reference as S

INPUTS = S.smoother_inputs()
IDS = [c[0] for c in INPUTS]


def big(a):
    return float(np.max(np.abs(a)))


@pytest.mark.parametrize("case", INPUTS, ids=IDS)
def test_collapsed_filter_equals_textbook_filter(case):
    """The header's arrangement against the dense one: loglik 1e-12 relative,
    filtered / smoothed means and smoothed covariances 1e-12 of the largest
    magnitude (measured <= 2.2e-14)."""
    label, X, L, sigma2, A, Q, P0 = case
    a = S.smooth(X, L, sigma2, A, Q, None, P0, method="brute")
    b = S.smooth(X, L, sigma2, A, Q, None, P0, method="collapsed")
    fig = {"loglik": abs(a["loglik"] - b["loglik"]) / abs(a["loglik"]),
           "filtered": big(a["filtered"] - b["filtered"]) / big(a["filtered"]),
           "smoothed": big(a["smoothed"] - b["smoothed"]) / big(a["smoothed"]),
           "cov": big(a["smoothed_cov"] - b["smoothed_cov"]) / big(a["smoothed_cov"])}
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert a["nobs"] == b["nobs"] == int((~np.isnan(X)).sum())
    for k, v in fig.items():
        assert v < 1e-12, (label, k, v)


@pytest.mark.parametrize("case", INPUTS, ids=IDS)
def test_forecast_rows_are_appended_missing_rows(case):
    """h appended NaN rows give Tm^k a_T|T, leave the log-likelihood and the
    filtered rows unchanged."""
    label, X, L, sigma2, A, Q, P0 = case
    T, h = X.shape[0], 4
    base = S.smooth(X, L, sigma2, A, Q, None, P0)
    ext = S.smooth(X, L, sigma2, A, Q, None, P0, horizon=h)
    assert ext["loglik"] == base["loglik"]
    assert np.array_equal(ext["filtered"], base["filtered"])
    a = base["state"][T - 1]
    scale = big(base["state"])
    for k in range(1, h + 1):
        a = base["Tm"] @ a
        assert big(ext["state"][T - 1 + k] - a) <= 1e-14 * scale, (label, k)
    assert big(ext["smoothed"][:T] - base["smoothed"]) <= 1e-13 * scale


@pytest.mark.parametrize("shape", S.SYNTHETIC, ids=[f"r{c[2]}p{c[3]}" for c in S.SYNTHETIC])
def test_stationary_cov_equals_kronecker_solve(dfm, shape):
    _, _, _, A, Q = S.make_synthetic(*shape)
    assert abs(S.spectral_radius(A) - 0.8) < 1e-9
    ref = S.stationary_kron(A, Q)
    got = dfm.stationary_covariance(A, Q)
    err = big(got - ref) / big(ref)
    print(shape, "doubling vs Kronecker", err, "numpy doubling", big(S.stationary_doubling(A, Q) - ref) / big(ref))
    assert got.shape == ref.shape and np.array_equal(got, got.T)
    assert err < 1e-12


def test_stationary_cov_return_codes(dfm):
    rng = np.random.default_rng(3)
    A = rng.standard_normal((3, 3))
    A *= 1.05 / S.spectral_radius(A)
    assert abs(S.spectral_radius(A) - 1.05) < 1e-12
    with pytest.raises(dfm.DFMError) as e:
        dfm.stationary_covariance(A, np.eye(3))
    assert e.value.code == 6
    with pytest.raises(dfm.DFMError) as e:   # r = 17
        dfm.stationary_covariance(0.1 * np.eye(17), np.eye(17))
    assert e.value.code == -7
    with pytest.raises(dfm.DFMError) as e:   # s = 36
        dfm.stationary_covariance(np.hstack([0.1 * np.eye(12)] * 3), np.eye(12))
    assert e.value.code == -7
    with pytest.raises(dfm.DFMError) as e:   # p = 9
        dfm.stationary_covariance(np.full((1, 9), 0.01), np.eye(1))
    assert e.value.code == -7
    bad = 0.1 * np.eye(2)
    bad[0, 1] = np.nan
    with pytest.raises(dfm.DFMError) as e:
        dfm.stationary_covariance(bad, np.eye(2))
    assert e.value.code == -12
