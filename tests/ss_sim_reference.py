"""NumPy restatement of the simulation smoother as include/dfm.h states it
(dfm_ss_simulate), on ss_reference's collapse, filter_collapsed and rts, and
the inputs of tests/test_ss_sim_host.py and tests/test_gpu_ss_sim.py.

`simulate` runs every draw at once (a row of z per draw) and returns the whole
state, so that the unit-vector check can compare all of P_t|T: with z = 0 a
draw is the smoothed state, and with W the responses to the unit vectors of z,
W_t' W_t = P_t|T and W_{t+1}' W_t = P_{t+1|T} J_t'."""
import functools

import numpy as np

import ss_reference as S

# (T, N, r, p, horizon) of the exact-moment checks: the host's, then the device's
HOST_SHAPES = ((9, 7, 3, 2, 2), (8, 5, 2, 1, 0), (7, 20, 4, 2, 1))
GPU_SHAPES = ((9, 7, 3, 2, 2), (33, 33, 1, 1, 0), (12, 20, 16, 2, 0))


def psd_cholesky(C):
    """Lower-triangular R with R R' = C for a positive semi-definite C: column j
    is zero when its pivot d <= 1e-12 C_jj."""
    C = np.atleast_2d(np.asarray(C, dtype=np.float64))
    n = C.shape[0]
    R = np.zeros((n, n))
    for j in range(n):
        d = C[j, j] - R[j, :j] @ R[j, :j]
        if not d > 1e-12 * C[j, j]:
            continue
        R[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            R[i, j] = (C[i, j] - R[i, :j] @ R[j, :j]) / R[j, j]
    return R


def nz(Tt, r, s):
    return s + 2 * r * Tt


def gains(X, L, sigma2, A, Q, a0=None, P0=None, horizon=0):
    """Per row: n_t > 0, b_t, C_t, R_t, K_t, J_t (J of the last row zero), and
    the draw's constants a0, L0, Lq, Tm."""
    f = S.filter_collapsed(X, L, sigma2, A, Q, a0, P0, horizon)
    Xp, L, sigma2, r, s, Tm, _, a, P = S._prepare(X, L, sigma2, A, Q, a0, P0, horizon)
    C, b, _, n, _ = S.collapse(Xp, L, sigma2)
    Tt = Xp.shape[0]
    K = np.zeros((Tt, s, r))
    J = np.zeros((Tt, s, s))
    R = np.zeros((Tt, r, r))
    for t in range(Tt):
        if n[t] > 0:
            Pp = f["Pp"][t]
            K[t] = Pp[:, :r] @ np.linalg.inv(np.eye(r) + C[t] @ Pp[:r, :r])
            R[t] = psd_cholesky(C[t])
        if t < Tt - 1:
            J[t] = np.linalg.solve(f["Pp"][t + 1], Tm @ f["Pu"][t]).T
    return dict(obs=n > 0, b=b, C=C, R=R, K=K, J=J, a0=a, L0=psd_cholesky(P), Lq=np.linalg.cholesky(np.atleast_2d(Q)),
                Tm=Tm, r=r, s=s, Tt=Tt)


def simulate(X, L, sigma2, A, Q, z, a0=None, P0=None, horizon=0):
    """z: (D, nz).  Returns the draws of the state, (D, Tt, s); the factors'
    are [:, :, :r]."""
    g = gains(X, L, sigma2, A, Q, a0, P0, horizon)
    r, s, Tt, Tm = g["r"], g["s"], g["Tt"], g["Tm"]
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    D = z.shape[0]
    assert z.shape[1] == nz(Tt, r, s)
    alpha = np.zeros((D, Tt, s))
    cf = np.zeros((D, Tt, s))
    c = np.zeros((D, s))
    for t in range(Tt):
        o = s + 2 * r * t
        if t == 0:
            alpha[:, 0] = g["a0"] + z[:, :s] @ g["L0"].T
        else:
            alpha[:, t] = alpha[:, t - 1] @ Tm.T
            alpha[:, t, :r] += z[:, o:o + r] @ g["Lq"].T
        if g["obs"][t]:
            bs = g["b"][t] - alpha[:, t, :r] @ g["C"][t].T - z[:, o + r:o + 2 * r] @ g["R"][t].T
            c = c + (bs - c[:, :r] @ g["C"][t].T) @ g["K"][t].T
        cf[:, t] = c
        c = c @ Tm.T
    cs = cf.copy()
    for t in range(Tt - 2, -1, -1):
        cs[:, t] = cf[:, t] + (cs[:, t + 1] - cf[:, t] @ Tm.T) @ g["J"][t].T
    return alpha + cs


def unit_z(n):
    """[0; I_n]: the zero draw, then the unit vectors."""
    return np.vstack([np.zeros((1, n)), np.eye(n)])


def moment_figures(state, ref, J):
    """Errors of the unit-vector check, each relative to the reference array's
    largest magnitude.  state: (nz + 1, Tt, k) draws under unit_z (k = s, or r
    with the factor blocks of ref and J's products)."""
    big = lambda a: float(np.max(np.abs(a)))   # noqa: E731
    k = state.shape[2]
    W = state[1:] - state[0]
    cov = np.einsum("dti,dtj->tij", W, W)
    lag = np.einsum("dti,dtj->tij", W[:, 1:], W[:, :-1])
    lag_ref = np.einsum("tik,tjk->tij", ref["state_cov"][1:], J[:-1])[:, :k, :k]
    fig = {"mean": big(state[0] - ref["state"][:, :k]) / big(ref["state"][:, :k]),
           "cov": big(cov - ref["state_cov"][:, :k, :k]) / big(ref["state_cov"][:, :k, :k])}
    if lag_ref.size:
        fig["lag"] = big(lag - lag_ref) / big(lag_ref)
    return fig


@functools.lru_cache(maxsize=None)
def moment_case(T, N, r, p, h):
    """Parameters of ss_reference.make_synthetic at (T, N, r, p) with a panel of
    its own: 20 % missing at random, row 1 observed on column 0 only, row 2 on
    columns 0 and 1, row 3 empty; a caller's a0.  With it the dense reference
    smoother's record and its J_t (read-only)."""
    X, L, sigma2, A, Q = S.make_synthetic(T, N, r, p, complete=True)
    rng = np.random.Generator(np.random.PCG64(9100 + 100 * T + N))
    miss = rng.uniform(size=X.shape) < 0.20
    miss[1:4] = True
    miss[1, 0] = miss[2, 0] = miss[2, 1] = False
    X[miss] = np.nan
    a0 = np.linspace(-1.0, 1.0, r * p)
    f = S.filter_brute(X, L, sigma2, A, Q, a0, None, h)
    J = np.zeros_like(f["Pu"])
    for t in range(f["Pu"].shape[0] - 1):
        J[t] = np.linalg.solve(f["Pp"][t + 1], f["Tm"] @ f["Pu"][t]).T
    ref = S.smooth(X, L, sigma2, A, Q, a0, None, h, method="brute")
    return X, L, sigma2, A, Q, a0, ref, J
