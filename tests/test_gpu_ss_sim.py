"""The simulation smoother on the device (dfm_ss_simulate through
simulation_smoother) against the dense textbook smoother of
tests/ss_reference.py and the NumPy restatement tests/ss_sim_reference.py.

Exact moments: the draw is affine in z, so z = [0; I_nz] shows its mean and
its whole covariance — the zero draw is the smoothed path, the unit-vector
responses W give W_t' W_t = P_t|T and W_{t+1}' W_t = P_{t+1|T} J_t' (factor
blocks).  Parity: seeded random z against the restatement.  Bars are
test_gpu_ss.py's: 1e-10 of the reference array's largest magnitude.  What the
header promises bit for bit is checked bit for bit: the smoother's own outputs,
independence of D, of the pass, of the lane and of the horizon's extra rows,
device inputs, repeatability, and a NaN staying in its draw."""
import numpy as np
import pytest

import ss_reference as S
import ss_sim_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GPU_IDS = [f"{T}x{N}r{r}p{p}h{h}" for T, N, r, p, h in R.GPU_SHAPES]
SYN_IDS = [f"{T}x{N}r{r}p{p}" for T, N, r, p in S.SYNTHETIC]


@pytest.fixture(scope="module")
def ctx(dfm):
    return dfm.default_context()


def big(a):
    return float(np.max(np.abs(a)))


def report(label, fig):
    """Print every figure, then assert each against the bar."""
    print(label, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < RTOL, (label, k, v)


# ------------------------------------------------------------- exact moments
@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=GPU_IDS)
def test_exact_moments_against_the_dense_smoother(dfm, ctx, shape):
    """D = nz + 1: 73 (one full wave and a partial one), 69 (the scalar case),
    417 (s = 32).  Each panel has a one-entry row, a two-entry row, an empty
    row and a caller's a0."""
    X, L, sigma2, A, Q, a0, ref, J = R.moment_case(*shape)
    T, N, r, p, h = shape
    n = R.nz(T + h, r, r * p)
    res = dfm.simulation_smoother(X, L, sigma2, A, Q, draws=n + 1, z=R.unit_z(n), a0=a0, horizon=h, ctx=ctx)
    assert res.draws.shape == (n + 1, T + h, r)
    fig = R.moment_figures(res.draws, ref, J)
    assert set(fig) == {"mean", "cov", "lag"}
    fig["smoothed"] = big(res.draws[0] - ref["smoothed"]) / big(ref["smoothed"])
    report(f"moments {GPU_IDS[R.GPU_SHAPES.index(shape)]}", fig)


# -------------------------------------------------------------------- parity
def parity(dfm, ctx, label, X, L, sigma2, A, Q, P0, h):
    r, s = L.shape[1], A.shape[1]
    z = np.random.default_rng(2026).standard_normal((70, R.nz(X.shape[0] + h, r, s)))
    ref = R.simulate(X, L, sigma2, A, Q, z, P0=P0, horizon=h)[:, :, :r]
    res = dfm.simulation_smoother(X, L, sigma2, A, Q, draws=70, z=z, P0=P0, horizon=h, ctx=ctx)
    report(label, {"draws": big(res.draws - ref) / big(ref)})


@pytest.mark.parametrize("i", range(4), ids=SYN_IDS)
def test_parity_on_synthetic_parameters(dfm, ctx, i):
    """s = 32, r = 16, the scalar case, s = 15; P0 left to the library."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(i)
    parity(dfm, ctx, f"parity {SYN_IDS[i]}", X, L, sigma2, A, Q, None, 0)


def test_parity_on_fitted_parameters_with_horizon(dfm, ctx):
    _, ts = S.two_step_case(3)
    parity(dfm, ctx, "parity fitted 67x19", ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], ts["P0"], S.HORIZON)


# --------------------------------------------------------------- bit for bit
@pytest.fixture(scope="module")
def base(dfm, ctx):
    """60 x 40, r = 5, p = 3: 150 rows of normals long enough for three forecast
    rows, and the D = 70 call on the horizon-free prefix the others compare with."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(3)
    T, r, s = X.shape[0], L.shape[1], A.shape[1]
    z3 = np.random.default_rng(77).standard_normal((150, R.nz(T + 3, r, s)))
    z = np.ascontiguousarray(z3[:, :R.nz(T, r, s)])
    run = lambda zz, **kw: dfm.simulation_smoother(X, L, sigma2, A, Q, draws=len(zz), z=zz, ctx=ctx, **kw)   # noqa: E731
    return dict(X=X, par=(L, sigma2, A, Q), z=z, z3=z3, run=run, d70=run(z[:70]))


def test_smoother_outputs_are_kalman_smoothers(dfm, ctx, base):
    ks = dfm.kalman_smoother(base["X"], *base["par"], ctx=ctx)
    d = base["d70"]
    assert np.array_equal(d.smoothed, ks.smoothed) and np.array_equal(d.smoothed_cov, ks.smoothed_cov)
    assert d.loglik == ks.loglik
    assert np.isfinite(d.draws).all() and big(d.draws - d.smoothed) > 0.0


@pytest.mark.parametrize("D", (1, 5, 64, 65))
def test_a_draw_does_not_depend_on_D(base, D):
    assert np.array_equal(base["run"](base["z"][:D]).draws, base["d70"].draws[:D])


def test_a_draw_does_not_depend_on_its_pass(base):
    a = base["run"](base["z"])
    b = base["run"](base["z"], pass_draws=64)   # 64 + 64 + 22
    assert np.array_equal(a.draws, b.draws) and np.array_equal(a.draws[:70], base["d70"].draws)


def test_horizon_rows_extend_the_same_draws(base):
    T = base["X"].shape[0]
    hor = base["run"](base["z3"][:70], horizon=3)
    assert hor.draws.shape[1] == T + 3 and np.isfinite(hor.draws).all()
    assert np.array_equal(hor.draws[:, :T], base["d70"].draws)


def test_device_inputs_and_repeatability(dfm, ctx, base):
    import torch
    z = base["z"][:70]
    zd = torch.from_numpy(np.ascontiguousarray(z.T)).cuda().T            # (D, nz), strides (1, D)
    xd = torch.from_numpy(np.ascontiguousarray(base["X"].T)).cuda().t()   # column-major in HBM
    L, sigma2, A, Q = base["par"]
    for x, zz in ((base["X"], zd), (xd, z), (xd, zd), (base["X"], z)):
        o = dfm.simulation_smoother(x, L, sigma2, A, Q, draws=70, z=zz, ctx=ctx)
        assert np.array_equal(o.draws, base["d70"].draws)
        assert np.array_equal(o.smoothed_cov, base["d70"].smoothed_cov) and o.loglik == base["d70"].loglik


def test_a_nan_stays_in_its_draw(base):
    z = base["z"][:70].copy()
    z[3, 40] = np.nan   # zeta_2's first entry (s = 15, r = 5)
    o = base["run"](z)
    assert np.isnan(o.draws[3]).any()
    keep = np.arange(70) != 3
    assert np.array_equal(o.draws[keep], base["d70"].draws[keep])


def test_rng_draws_the_normals(dfm, ctx, base):
    L, sigma2, A, Q = base["par"]
    kw = dict(draws=6, ctx=ctx)
    a = dfm.simulation_smoother(base["X"], L, sigma2, A, Q, rng=np.random.default_rng(3), **kw)
    b = dfm.simulation_smoother(base["X"], L, sigma2, A, Q, rng=np.random.default_rng(3), **kw)
    c = dfm.simulation_smoother(base["X"], L, sigma2, A, Q, rng=np.random.default_rng(4), **kw)
    assert a.draws.shape == (6, 60, 5) and np.array_equal(a.draws, b.draws) and not np.array_equal(a.draws, c.draws)


# ------------------------------------------------------------------ refusals
def test_refusals(dfm, ctx, base):
    import torch
    X, (L, sigma2, A, Q), z = base["X"], base["par"], base["z"][:8]
    Qb = Q.copy()
    Qb[0, 0] = -1.0
    with pytest.raises(dfm.DFMError) as e:   # Q not positive definite
        dfm.simulation_smoother(X, L, sigma2, A, Qb, draws=8, z=z, ctx=ctx)
    assert e.value.code == 5
    with pytest.raises((dfm.DFMError, ValueError)):
        dfm.simulation_smoother(X, L, sigma2, A, Q, draws=0, z=z[:0], ctx=ctx)
    with pytest.raises((dfm.DFMError, ValueError)):   # one normal short
        dfm.simulation_smoother(X, L, sigma2, A, Q, draws=8, z=z[:, :-1], ctx=ctx)
    with pytest.raises((dfm.DFMError, ValueError)):   # draws and z disagree
        dfm.simulation_smoother(X, L, sigma2, A, Q, draws=7, z=z, ctx=ctx)
    zd = torch.from_numpy(np.ascontiguousarray(z.T)).cuda()
    with pytest.raises((dfm.DFMError, ValueError)):   # ldz = 7 < D = 8
        dfm.simulation_smoother(X, L, sigma2, A, Q, draws=8, z=zd.as_strided((8, z.shape[1]), (1, 7)), ctx=ctx)
    with pytest.raises(dfm.DFMError) as e:   # r = 17
        dfm.simulation_smoother(X, np.ones((40, 17)), sigma2, 0.1 * np.eye(17), np.eye(17), draws=2,
                                z=np.zeros((2, 17 + 34 * 60)), ctx=ctx)
    assert e.value.code == -7
    ok = base["run"](base["z"][:5])   # the context still serves a good call
    assert np.array_equal(ok.draws, base["d70"].draws[:5])
