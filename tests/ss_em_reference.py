"""NumPy restatement of the quasi-maximum-likelihood EM of the state-space
factor model as include/dfm.h states it (dfm_ss_em, dfm_ss_fit_ml), and the
inputs of tests/test_ss_em_host.py and tests/test_gpu_ss_em.py.

The E-step is ss_reference.filter_brute (the textbook filter on the dense
innovation covariance) and a Rauch-Tung-Striebel pass of its own that also
forms the lag-one block Cov(f_t, alpha_{t-1} | T) = (P_t|T J_{t-1}')[:r]; the
M-step solves the per-series normal equations and the transition regression
with numpy.linalg.solve.  Nothing here follows the library's arrangement
(collapsed rows, triangular operands, K chunks)."""
import functools
import math

import numpy as np

import ss_reference as S

BATCH_RP = (2, 2)                 # (r, p) of the same-shape batch
BATCH_ITERATIONS = (8, 15, 7, 12, 27)


def backward(f):
    """RTS pass over a filter's record with the lag-one blocks: (a_t|T, P_t|T,
    lag), lag[t] = Cov(f_t, alpha_{t-1} | T) for t >= 1 (row 0 unused)."""
    au, Pu, ap, Pp, Tm, r = f["au"], f["Pu"], f["ap"], f["Pp"], f["Tm"], f["r"]
    Tt, s = au.shape
    sa, sP = au.copy(), Pu.copy()
    lag = np.zeros((Tt, r, s))
    for t in range(Tt - 2, -1, -1):
        J = np.linalg.solve(Pp[t + 1], Tm @ Pu[t]).T
        lag[t + 1] = (sP[t + 1] @ J.T)[:r]
        sa[t] = au[t] + J @ (sa[t + 1] - ap[t + 1])
        sP[t] = Pu[t] + J @ (sP[t + 1] - Pp[t + 1]) @ J.T
    return sa, sP, lag


def e_step(X, L, sigma2, A, Q, a0, P0, horizon=0):
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    f = S.filter_brute(X, L, sigma2, A, Q, a0, P0, horizon)
    sa, sP, lag = backward(f)
    r = f["r"]
    return dict(loglik=f["loglik"], nobs=f["nobs"], state=sa, state_cov=sP, lag=lag, r=r,
                filtered=f["au"][:T, :r].copy(), smoothed=sa[:, :r].copy(), smoothed_cov=sP[:, :r, :r].copy())


def m_step(X, es, update_init, a0, P0):
    """theta_{j+1} from the smoothed moments of rows < T."""
    X = np.asarray(X, dtype=np.float64)
    T, N = X.shape
    r = es["r"]
    a, P, lag = es["state"][:T], es["state_cov"][:T], es["lag"][:T]
    f = a[:, :r]
    E = f[:, :, None] * f[:, None, :] + P[:, :r, :r]
    S11 = E[1:].sum(axis=0)
    S10 = (f[1:, :, None] * a[:-1, None, :] + lag[1:]).sum(axis=0)
    S00 = (a[:-1, :, None] * a[:-1, None, :] + P[:-1]).sum(axis=0)
    m = ~np.isnan(X)
    x0 = np.where(m, X, 0.0)
    L = np.zeros((N, r))
    sigma2 = np.zeros(N)
    for i in range(N):
        Si = E[m[:, i]].sum(axis=0)
        gi = (x0[:, i, None] * f).sum(axis=0)
        L[i] = np.linalg.solve(Si, gi)
        sigma2[i] = ((x0[:, i] ** 2).sum() - L[i] @ gi) / m[:, i].sum()
    An = np.linalg.solve(S00.T, S10.T).T
    Qn = (S11 - An @ S10.T) / (T - 1)
    Qn = 0.5 * (Qn + Qn.T)
    if update_init:
        a0, P0 = es["state"][0].copy(), es["state_cov"][0].copy()
    return L, sigma2, An, Qn, a0, P0


def criterion(ll, prev):
    den = 0.5 * (abs(ll) + abs(prev))
    return (ll - prev) / den if den > 0 else 0.0


def em(X, L, sigma2, A, Q, a0=None, P0=None, tol=1e-4, max_iter=100, update_init=True, horizon=0):
    """The loop of the header.  Returns the parameters of the last E-step, its
    outputs, the path, `iterations`, `converged` and every c_j."""
    X = np.asarray(X, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64)).copy()
    sigma2 = np.asarray(sigma2, dtype=np.float64).copy()
    A = np.atleast_2d(np.asarray(A, dtype=np.float64)).copy()
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64)).copy()
    s = A.shape[1]
    a0 = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    P0 = S.stationary_kron(A, Q) if P0 is None else np.asarray(P0, dtype=np.float64).copy()
    path, crit, converged, j = [], [], False, 0
    while True:
        es = e_step(X, L, sigma2, A, Q, a0, P0, horizon)
        path.append(es["loglik"])
        if j >= 1:
            crit.append(criterion(path[j], path[j - 1]))
            if tol > 0 and crit[-1] < tol:
                converged = True
                break
        if j == max_iter:
            break
        L, sigma2, A, Q, a0, P0 = m_step(X, es, update_init, a0, P0)
        j += 1
    return dict(L=L, sigma2=sigma2, A=A, Q=Q, a0=a0, P0=P0, path=np.array(path), crit=np.array(crit), iterations=j,
                converged=converged, loglik=es["loglik"], nobs=es["nobs"], filtered=es["filtered"],
                smoothed=es["smoothed"], smoothed_cov=es["smoothed_cov"])


# ------------------------------------------------------------- the generators
def batch_panel(k, T=40, N=24, r=2):
    rng = np.random.Generator(np.random.PCG64(20261101 + k))
    rho = (0.3, 0.5, 0.7, 0.8, 0.9)[k % 5]
    f = np.zeros((T + 50, r))
    for t in range(1, T + 50):
        f[t] = rho * f[t - 1] + math.sqrt(1 - rho * rho) * rng.standard_normal(r)
    f = f[50:]
    X = f @ rng.standard_normal((N, r)).T + math.sqrt(r) * rng.standard_normal((T, N))
    miss = rng.uniform(size=(T, N)) < 0.10 + 0.05 * k
    miss[T - 4:, k % 3::3] = True
    miss[T // 2 + k, :] = True
    miss[:, 0] = False; miss[T // 2 + k, 0] = True
    X[miss] = np.nan
    return X


@functools.lru_cache(maxsize=None)
def fitted_em(i, update_init):
    """EM on two-step panel i from the reference's Zm and two-step parameters:
    tol = 0, 8 iterations, HORIZON forecast rows (read-only)."""
    _, ts = S.two_step_case(i)
    return em(ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], None, ts["P0"], tol=0.0, max_iter=8,
              update_init=update_init, horizon=S.HORIZON)


@functools.lru_cache(maxsize=None)
def synthetic_em(i):
    """EM on synthetic set i from its true parameters: tol = 0, 4 iterations (read-only)."""
    X, L, sigma2, A, Q, _ = S.synthetic_case(i)
    return em(X, L, sigma2, A, Q, tol=0.0, max_iter=4)


@functools.lru_cache(maxsize=None)
def batch_case(k):
    """Batch panel k: its reference two-step start (static EM tol = 0, six
    iterations) and the EM from it at tol = 1e-4, max_iter = 60 (read-only)."""
    X = batch_panel(k)
    r, p = BATCH_RP
    ts = S.two_step(X, r, p, horizon=0, tol=0.0, max_iter=6)
    start = dict(Zm=ts["Zm"], L=ts["em"]["L"], sigma2=ts["sigma2"], A=ts["A"], Q=ts["Q"], P0=ts["P0"])
    return start, em(ts["Zm"], start["L"], start["sigma2"], start["A"], start["Q"], None, start["P0"], tol=1e-4,
                     max_iter=60)


CHUNK_SHAPE = (270, 70)           # T beyond one K chunk of the M-step GEMM (256 rows), N beyond one row tile (64)


@functools.lru_cache(maxsize=None)
def chunk_case(k):
    """Panel k at CHUNK_SHAPE (r = 2, p = 1): its reference two-step start and
    three EM iterations at tol = 0 from it (read-only)."""
    T, N = CHUNK_SHAPE
    X = batch_panel(k, T=T, N=N)
    ts = S.two_step(X, 2, 1, horizon=0, tol=0.0, max_iter=6)
    start = dict(Zm=ts["Zm"], L=ts["em"]["L"], sigma2=ts["sigma2"], A=ts["A"], Q=ts["Q"], P0=ts["P0"])
    return start, em(ts["Zm"], start["L"], start["sigma2"], start["A"], start["Q"], None, start["P0"], tol=0.0,
                     max_iter=3)


def ml_chain(i, max_iter=5, update_init=True):
    """dfm_ss_fit_ml in NumPy on two-step panel i: the two-step fit, `max_iter`
    EM iterations at tol = 0 from it, and the panels from the ML parameters."""
    X, ts = S.two_step_case(i)
    T = X.shape[0]
    res = em(ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], None, ts["P0"], tol=0.0, max_iter=max_iter,
             update_init=update_init, horizon=S.HORIZON)
    m = ~np.isnan(X)
    common = res["smoothed"] @ res["L"].T
    mu, sd = ts["em"]["mu"], ts["em"]["sd"]
    return dict(em=res, x_completed=np.where(m, X, common[:T] * sd + mu), forecast=common[T:] * sd + mu)
