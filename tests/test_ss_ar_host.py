"""CPU checks of what the AR(1) idiosyncratic model rests on, in NumPy
(tests/ss_ar_reference.py): on single-run patterns the run-wise model (a) is
the exact model (b); the quasi-differenced collapsed recursion of include/dfm.h
is the dense filter of (a); the fill rule is (b)'s smoothed Lambda f + e at
leading and trailing missing entries; at rho = 0 the reference is
tests/ss_reference.py."""
import numpy as np
import pytest

import ss_ar_reference as AR
import ss_reference as SR

KEYS = ("filtered", "smoothed", "smoothed_cov")


def _close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b))) <= tol * max(float(np.max(np.abs(b))), 1e-300)


@pytest.mark.parametrize("k", range(4))
def test_runwise_equals_exact_on_single_runs(k):
    a, b = AR.case_reference(k, True), AR.case_reference(k, False)
    assert abs(a["loglik"] - b["loglik"]) <= 1e-10 * abs(b["loglik"])
    assert a["nobs"] == b["nobs"]
    for key in KEYS:
        assert _close(a[key], b[key], 1e-10), key


@pytest.mark.parametrize("k", range(5))
def test_collapsed_recursion_equals_dense_runwise(k):
    X, L, sigma2, rho, A, Q, h, _ = AR.case(k)
    a, c = AR.case_reference(k, True), AR.collapsed(X, L, sigma2, rho, A, Q, horizon=h)
    assert abs(a["loglik"] - c["loglik"]) <= 1e-10 * abs(a["loglik"])
    assert a["nobs"] == c["nobs"] == int((~np.isnan(X)).sum())
    for key in KEYS:
        assert _close(c[key], a[key], 1e-10), key


def test_interior_holes_change_the_likelihood():
    """With holes the run-wise model is another model than the exact one."""
    a, b = AR.case_reference(4, True), AR.case_reference(4, False)
    assert abs(a["loglik"] - b["loglik"]) > 1e-8 * abs(b["loglik"])


@pytest.mark.parametrize("k", range(4))
def test_fill_rule_equals_exact_smoothed_idio_at_the_edges(k):
    X, L, sigma2, rho, A, Q, h, _ = AR.case(k)
    b = AR.case_reference(k, False)
    want = b["smoothed"] @ L.T + b["idio"]
    got = AR.fill(X, L, rho, b["smoothed"])
    miss = np.isnan(X)
    assert miss.any()
    assert np.max(np.abs(got[:X.shape[0]][miss] - want[:X.shape[0]][miss])) <= 1e-10 * np.max(np.abs(want))
    assert np.array_equal(got[:X.shape[0]][~miss], X[~miss])


def test_fill_rule_bridges_a_hole_as_the_exact_model_given_the_factors():
    """The bridge is E[e_t | e_u, e_v] of an AR(1): checked against the
    conditional mean from the stationary covariance."""
    rho, d1, d2 = 0.7, 2, 3
    u, t, v = 0, d1, d1 + d2
    cov = lambda a, b: rho ** abs(a - b)   # noqa: E731
    S = np.array([[cov(u, u), cov(u, v)], [cov(v, u), cov(v, v)]])
    w = np.linalg.solve(S, np.array([cov(t, u), cov(t, v)]))
    X = np.full((v + 1, 1), np.nan)
    X[u, 0], X[v, 0] = 1.5, -0.5
    got = AR.fill(X, np.zeros((1, 1)), np.array([rho]), np.zeros((v + 1, 1)))
    assert abs(got[t, 0] - (w[0] * 1.5 + w[1] * -0.5)) < 1e-14


def test_reference_at_rho_zero_is_the_plain_reference():
    X, L, sigma2, A, Q = SR.make_synthetic(33, 33, 1, 1)
    X2, L2, s2, A2, Q2 = SR.make_synthetic(40, 24, 3, 2)
    for X, L, sigma2, A, Q in ((X, L, sigma2, A, Q), (X2, L2, s2, A2, Q2)):
        plain = SR.smooth(X, L, sigma2, A, Q, horizon=2)
        for runwise in (True, False):
            ar = AR.dense(X, L, sigma2, np.zeros(X.shape[1]), A, Q, horizon=2, runwise=runwise)
            assert abs(ar["loglik"] - plain["loglik"]) <= 1e-10 * abs(plain["loglik"])
            assert ar["nobs"] == plain["nobs"]
            for key in KEYS:
                assert _close(ar[key], plain[key], 1e-10), key


def test_estimate_recovers_rho_of_a_long_series():
    rng = np.random.default_rng(3)
    T, rho = 4000, np.array([0.6, -0.3, 0.0])
    e = np.zeros((T, 3))
    for t in range(1, T):
        e[t] = rho * e[t - 1] + rng.standard_normal(3)
    F = rng.standard_normal((T, 1))
    L = np.array([[1.0], [0.5], [-1.0]])
    sigma2, _, _, P0, est = AR.estimate_ar(F @ L.T + e, F, L, 1)
    assert np.max(np.abs(est - rho)) < 0.05 and np.max(np.abs(sigma2 - 1.0)) < 0.1
    assert P0.shape == (2, 2)
