"""The simulation smoother's construction (include/dfm.h, dfm_ss_simulate) in
NumPy, tests/ss_sim_reference.py, against the dense textbook smoother of
tests/ss_reference.py — no device.

The draw is affine in z, so feeding z = 0 and then the unit vectors of z shows
all of its first two moments exactly: z = 0 must return the smoothed state, and
with W the unit-vector responses W_t' W_t must be P_t|T and W_{t+1}' W_t must
be P_{t+1|T} J_t'.  Every panel has a row with one entry, a row with two (both
rank-deficient C_t), an empty row and a caller's a0.

Bar: 1e-12 of the reference array's largest magnitude.  The errors measured
are 6e-16 to 1.5e-15 (a handful of roundings of O(1) quantities): nearly three
orders below the bar."""
import numpy as np
import pytest

import ss_reference as S
import ss_sim_reference as R

BAR = 1e-12
IDS = [f"{T}x{N}r{r}p{p}h{h}" for T, N, r, p, h in R.HOST_SHAPES]


@pytest.mark.parametrize("shape", R.HOST_SHAPES, ids=IDS)
def test_unit_vector_moments(shape):
    X, L, sigma2, A, Q, a0, ref, J = R.moment_case(*shape)
    T, N, r, p, h = shape
    n = R.nz(T + h, r, r * p)
    state = R.simulate(X, L, sigma2, A, Q, R.unit_z(n), a0=a0, horizon=h)
    assert state.shape == (n + 1, T + h, r * p)
    fig = R.moment_figures(state, ref, J)
    print(IDS[R.HOST_SHAPES.index(shape)], " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert set(fig) == {"mean", "cov", "lag"}
    for k, v in fig.items():
        assert v < BAR, (k, v)


@pytest.mark.parametrize("shape", R.HOST_SHAPES, ids=IDS)
def test_psd_factor_of_every_row(shape):
    """R_t R_t' = C_t on every row, the rank-deficient ones included, and R_t
    has as many non-zero columns as the row has independent loadings."""
    X, L, sigma2, A, Q, a0, _, _ = R.moment_case(*shape)
    T, N, r, p, h = shape
    g = R.gains(X, L, sigma2, A, Q, a0, None, h)
    C = g["C"]
    err = max(float(np.max(np.abs(g["R"][t] @ g["R"][t].T - C[t]))) for t in range(T + h))
    print("R R' - C", err / float(np.max(np.abs(C))))
    assert err < BAR * float(np.max(np.abs(C)))
    nonzero = lambda t: int((np.abs(np.diag(g["R"][t])) > 0).sum())   # noqa: E731
    assert nonzero(1) == 1 and nonzero(2) == min(2, r) and nonzero(3) == 0 and not g["obs"][3]
    assert np.allclose(g["L0"] @ g["L0"].T, S.stationary_kron(A, Q), rtol=0, atol=BAR * float(np.max(np.abs(g["L0"]))) ** 2)


def test_layout_of_the_normals():
    """An h-row call's first s + 2 r T normals are the h = 0 call's: the rows
    t < T of the pre-smoothing draw alpha+ agree, and a draw's row depends on
    its own row of z only."""
    shape = R.HOST_SHAPES[0]
    X, L, sigma2, A, Q, a0, _, _ = R.moment_case(*shape)
    T, N, r, p, _ = shape
    s = r * p
    rng = np.random.default_rng(5)
    z3 = rng.standard_normal((4, R.nz(T + 3, r, s)))
    z0 = z3[:, :R.nz(T, r, s)]
    a = R.simulate(X, L, sigma2, A, Q, z3, a0=a0, horizon=3)
    b = R.simulate(X, L, sigma2, A, Q, z0, a0=a0, horizon=0)
    assert np.allclose(a[:, :T], b, rtol=0, atol=1e-12 * float(np.max(np.abs(b))))
    one = R.simulate(X, L, sigma2, A, Q, z3[2:3], a0=a0, horizon=3)
    assert np.allclose(one[0], a[2], rtol=0, atol=1e-12 * float(np.max(np.abs(b))))
