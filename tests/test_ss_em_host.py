"""CPU checks of the quasi-ML EM's NumPy reference (tests/ss_em_reference.py):
the lag-one identity Cov(f_t, alpha_{t-1} | T) = (P_t|T J_{t-1}')[:r] against
the smoothed covariance of the state augmented with p more lags, the
log-likelihood rising along the path, and the conditions on the inputs that
tests/test_gpu_ss_em.py relies on.  No device work."""
import numpy as np
import pytest

import ss_em_reference as R
import ss_reference as S


def big(a):
    return float(np.max(np.abs(a)))


@pytest.mark.parametrize("i", (2, 3), ids=("r1p1", "r5p3"))
def test_lag_one_identity_against_the_augmented_state(i):
    """[A, 0] as a VAR(2p): alpha_{t-1} is entries r..r+s of the augmented
    state at t, so its smoothed covariance holds the lag-one block."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(i)
    r, s = A.shape
    es = R.e_step(X, L, sigma2, A, Q, None, None)
    aug = S.smooth(X, L, sigma2, np.hstack([A, np.zeros((r, s))]), Q)
    want = aug["state_cov"][1:, :r, r:r + s]
    err = big(es["lag"][1:] - want) / big(want)
    print(S.SYNTHETIC[i], "lag-one identity", err, "loglik", abs(es["loglik"] - aug["loglik"]) / abs(aug["loglik"]))
    assert err < 1e-12
    assert big(es["state"] - aug["state"][:, :s]) < 1e-12 * big(es["state"])
    sa, sP = S.rts(S.filter_brute(X, L, sigma2, A, Q))
    assert np.array_equal(sa, es["state"]) and np.array_equal(sP, es["state_cov"])


@pytest.mark.parametrize("update_init", (True, False), ids=("init", "fixed"))
@pytest.mark.parametrize("i", range(4))
def test_reference_path_rises(i, update_init):
    ref = R.fitted_em(i, update_init)
    steps = np.diff(ref["path"])
    print(S.SHAPES[i], update_init, "smallest increment", steps.min())
    assert ref["iterations"] == 8 and len(ref["path"]) == 9 and (steps > 0).all()


def test_conditions_of_the_device_tests():
    """What tests/test_gpu_ss_em.py assumes of its inputs, on the reference."""
    runs = [R.fitted_em(i, u) for i in range(4) for u in (True, False)] + [R.synthetic_em(i) for i in range(4)] + \
        [R.chunk_case(k)[1] for k in range(2)]
    assert R.CHUNK_SHAPE[0] > 256 and R.CHUNK_SHAPE[0] % 16 and R.CHUNK_SHAPE[1] > 64   # two K chunks, two row tiles
    inc = min(np.diff(r["path"]).min() for r in runs)
    sig = min(r["sigma2"].min() for r in runs)
    eig = min(np.linalg.eigvalsh(r["Q"]).min() for r in runs)
    print("smallest increment", inc, "smallest sigma2", sig, "smallest eigenvalue of Q", eig)
    # every run's increments stay three orders above 1e-10 of its loglik (the device tests' bar on the path), so a
    # device path that rises is no accident of rounding; the reference well conditioned
    for r in runs:
        assert np.diff(r["path"]).min() > 1e3 * 1e-10 * abs(r["loglik"])
    assert inc > 1e-3
    assert sig > 0.05 and eig > 1e-3
    batch = [R.batch_case(k)[1] for k in range(5)]
    its = tuple(b["iterations"] for b in batch)
    assert its == R.BATCH_ITERATIONS and len(set(its)) > 1 and max(its) < 60 and all(b["converged"] for b in batch)
    closest = min(np.min(np.abs(b["crit"] / 1e-4 - 1.0)) for b in batch)
    print("iterations", its, "closest c_j to tol", closest)
    assert closest > 0.01
    for b in batch:
        assert (b["crit"][:-1] >= 1e-4).all() and b["crit"][-1] < 1e-4 and len(b["path"]) == b["iterations"] + 1


def test_horizon_leaves_the_parameters():
    _, ts = S.two_step_case(3)
    args = (ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], None, ts["P0"])
    a = R.em(*args, tol=0.0, max_iter=2)
    b = R.em(*args, tol=0.0, max_iter=2, horizon=3)
    for k in ("L", "sigma2", "A", "Q", "a0", "P0", "path"):
        assert big(a[k] - b[k]) <= 1e-13 * big(a[k]), k
    assert b["smoothed"].shape[0] == a["smoothed"].shape[0] + 3
