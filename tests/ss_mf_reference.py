"""NumPy restatement of the mixed-frequency state-space smoother as
include/dfm.h states it (dfm_ss_smooth_mf), and the inputs of
tests/test_ss_mf_host.py and tests/test_gpu_ss_mf.py.

A low-frequency series loads on ft_t = sum_k w_k f_{t-k}; the state keeps L =
max(p, n_w) lags.  Two filters: `filter_dense`, the textbook one with an
explicit N x s loading matrix (row i is lambda_i' in the first r columns for a
high-frequency series, [w_0 lambda_i' ... w_{n_w-1} lambda_i' 0 ...] for a
low-frequency one) on the dense n_t x n_t innovation covariance — the
reference — and `filter_classes`, the header's arrangement: per row one
r-dimensional update per class on that class's collapsed moments.  The
backward pass is ss_reference.rts at the padded state."""
import functools
import math

import numpy as np

import ss_reference as S

LOG2PI = S.LOG2PI
AGG_FLOW = (1.0, 2.0, 3.0, 2.0, 1.0)
AGG_MEAN = (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)

# (T, N, r, p, w): the shapes of the device tests
CASES = ((36, 10, 2, 1, AGG_FLOW),          # L > p: padded companion
         (40, 12, 3, 2, AGG_MEAN),          # n_w > p, odd s
         (30, 9, 4, 8, AGG_FLOW),           # s = 32 with L = p
         (30, 40, 16, 1, (0.5, 0.5)),       # r = 16, s = 32, five column tiles of the collapse
         (30, 6, 1, 1, (1.0,)),             # scalar
         (70, 300, 2, 1, AGG_FLOW))         # two K chunks of the collapse, two row tiles
CASE_IDS = [f"{T}x{N}r{r}p{p}w{len(w)}" for T, N, r, p, w in CASES]


# ------------------------------------------------------------------ the model
def lags(p, w):
    return max(p, len(w))


def padded_A(A, L):
    """[A 0]: r x rL."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    r = A.shape[0]
    out = np.zeros((r, r * L))
    out[:, :A.shape[1]] = A
    return out


def z_low(w, r, s):
    """Z_l = [w_0 I_r ... w_{n_w-1} I_r 0 ...] (r x s)."""
    Z = np.zeros((r, s))
    for k, wk in enumerate(w):
        Z[:, k * r:(k + 1) * r] = wk * np.eye(r)
    return Z


def loading_rows(L, low, w, s):
    """The N x s loading matrix of the padded state."""
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    N, r = L.shape
    Z = np.zeros((N, s))
    Z[:, :r] = L
    Zl = z_low(w, r, s)
    for i in np.flatnonzero(low):
        Z[i] = L[i] @ Zl
    return Z


def _prepare(X, L, A, Q, w, a0, P0, horizon):
    X = np.asarray(X, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    r = L.shape[1]
    Ap = padded_A(A, lags(np.atleast_2d(A).shape[1] // r, w))
    Tm = S.companion(Ap)
    s = Tm.shape[0]
    if horizon:
        X = np.vstack([X, np.full((horizon, X.shape[1]), np.nan)])
    a = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    P = S.stationary_kron(Ap, Q) if P0 is None else np.asarray(P0, dtype=np.float64).copy()
    return X, L, r, s, Tm, S.state_noise(Q, s), a, P


def filter_dense(X, L, sigma2, A, Q, low, w, a0=None, P0=None, horizon=0):
    """The textbook filter on the explicit loading rows; the record of
    ss_reference.filter_brute."""
    X, L, r, s, Tm, Qs, a, P = _prepare(X, L, A, Q, w, a0, P0, horizon)
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    Zall = loading_rows(L, low, w, s)
    Tt = X.shape[0]
    au, ap = np.zeros((Tt, s)), np.zeros((Tt, s))
    Pu, Pp = np.zeros((Tt, s, s)), np.zeros((Tt, s, s))
    ll, nobs = 0.0, 0
    for t in range(Tt):
        ap[t], Pp[t] = a, P
        o = ~np.isnan(X[t])
        n = int(o.sum())
        if n:
            Z = Zall[o]
            F = Z @ P @ Z.T + np.diag(sigma2[o])
            v = X[t, o] - Z @ a
            Fiv = np.linalg.solve(F, v)
            K = np.linalg.solve(F, Z @ P).T
            ll -= 0.5 * (n * LOG2PI + np.linalg.slogdet(F)[1] + v @ Fiv)
            a = a + K @ v
            P = P - K @ Z @ P
            nobs += n
        au[t], Pu[t] = a, P
        a = Tm @ a
        P = Tm @ P @ Tm.T + Qs
    return dict(au=au, Pu=Pu, ap=ap, Pp=Pp, loglik=float(ll), nobs=nobs, Tm=Tm, r=r)


def filter_classes(X, L, sigma2, A, Q, low, w, a0=None, P0=None, horizon=0):
    """The header's recursion: per row the high class against Z_h, then the
    low class against Z_l, each on its own collapsed moments."""
    X, L, r, s, Tm, Qs, a, P = _prepare(X, L, A, Q, w, a0, P0, horizon)
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    low = np.asarray(low, dtype=bool)
    Zc = (np.hstack([np.eye(r), np.zeros((r, s - r))]), z_low(w, r, s))
    mom = [S.collapse(X[:, sel], L[sel], sigma2[sel]) if sel.any() else None for sel in (~low, low)]
    Tt = X.shape[0]
    au, ap = np.zeros((Tt, s)), np.zeros((Tt, s))
    Pu, Pp = np.zeros((Tt, s, s)), np.zeros((Tt, s, s))
    ll, nobs = 0.0, 0
    for t in range(Tt):
        ap[t], Pp[t] = a, P
        for c in range(2):
            if mom[c] is None or not mom[c][3][t] > 0:
                continue
            C, b, q, n, ell = (m[t] for m in mom[c])
            PZ = P @ Zc[c].T
            V = Zc[c] @ PZ
            z = Zc[c] @ a
            G = np.eye(r) + C @ V
            Gi = np.linalg.inv(G)
            K = PZ @ Gi
            d = b - C @ z
            ll -= 0.5 * (n * LOG2PI + ell + np.linalg.slogdet(G)[1] + q - 2.0 * b @ z + z @ C @ z - d @ V @ Gi @ d)
            a = a + K @ d
            P = P - K @ C @ PZ.T
            P = 0.5 * (P + P.T)
            nobs += int(n)
        au[t], Pu[t] = a, P
        a = Tm @ a
        P = Tm @ P @ Tm.T + Qs
    return dict(au=au, Pu=Pu, ap=ap, Pp=Pp, loglik=float(ll), nobs=nobs, Tm=Tm, r=r)


def smooth(X, L, sigma2, A, Q, low, w, a0=None, P0=None, horizon=0, method="dense"):
    """What dfm_ss_smooth_mf returns for one panel."""
    T = np.asarray(X).shape[0]
    f = (filter_dense if method == "dense" else filter_classes)(X, L, sigma2, A, Q, low, w, a0, P0, horizon)
    sa, sP = S.rts(f)
    r = f["r"]
    return dict(filtered=f["au"][:T, :r].copy(), smoothed=sa[:, :r].copy(), smoothed_cov=sP[:, :r, :r].copy(),
                smoothed_agg=sa @ z_low(w, r, sa.shape[1]).T, loglik=f["loglik"], nobs=f["nobs"], state=sa,
                state_cov=sP, Pp=f["Pp"])


# ------------------------------------------------------------- the generators
def make_case(T, N, r, p, w, seed=0):
    """Parameters and a panel simulated from them: Lambda ~ N(0, 1), sigma^2 ~
    U(0.3, 1.3), A_1 = 0.5 I + N(0, 0.05^2), A_k = N(0, 0.05^2) / k beyond,
    Q = 0.5 I; the last third of the columns low-frequency, observed at
    t % 3 == 2 only.  Missing: 10 % holes, a 3-row ragged edge on every other
    high-frequency column, row 5 with only its low-frequency series, row 7
    with nothing.  Returns (X, L, sigma2, A, Q, low)."""
    rng = np.random.Generator(np.random.PCG64(9100 + 1000 * seed + 100 * T + 10 * r + p + len(w)))
    L = rng.standard_normal((N, r))
    sigma2 = rng.uniform(0.3, 1.3, size=N)
    A = np.hstack([(0.5 * np.eye(r) if k == 0 else 0.0) + 0.05 * rng.standard_normal((r, r)) / (k + 1)
                   for k in range(p)])
    assert S.spectral_radius(A) < 0.95
    Q = 0.5 * np.eye(r)
    low = np.zeros(N, dtype=bool)
    low[N - max(N // 3, 1):] = True
    nw, burn = len(w), 50
    f = np.zeros((T + burn, r))
    for t in range(p, T + burn):
        f[t] = sum(A[:, k * r:(k + 1) * r] @ f[t - 1 - k] for k in range(p)) + math.sqrt(0.5) * rng.standard_normal(r)
    agg = sum(w[k] * f[burn - k:T + burn - k] for k in range(nw))
    f = f[burn:]
    X = np.where(low, agg @ L.T, f @ L.T) + np.sqrt(sigma2) * rng.standard_normal((T, N))
    miss = rng.uniform(size=(T, N)) < 0.10
    miss[np.arange(T) % 3 != 2, N - int(low.sum()):] = True
    miss[T - 3:, 0:N - int(low.sum()):2] = True
    miss[5, ~low] = True
    miss[5, low] = False
    miss[7, :] = True
    X[miss] = np.nan
    return X, L, sigma2, A, Q, low


@functools.lru_cache(maxsize=None)
def case(i):
    """Case i with its reference smoother output (read-only)."""
    T, N, r, p, w = CASES[i]
    X, L, sigma2, A, Q, low = make_case(T, N, r, p, w)
    return X, L, sigma2, A, Q, low, w, smooth(X, L, sigma2, A, Q, low, w)


# ------------------------------------------------------- the quasi-ML EM
def e_step(X, L, sigma2, A, Q, low, w, a0, P0, horizon=0):
    """The dense filter, then ss_em_reference.backward for the lag-one
    covariances Cov(f_t, alpha_{t-1} | T) at the padded state."""
    import ss_em_reference as EM
    T = np.asarray(X).shape[0]
    f = filter_dense(X, L, sigma2, A, Q, low, w, a0, P0, horizon)
    sa, sP, lag = EM.backward(f)
    r = f["r"]
    return dict(loglik=f["loglik"], nobs=f["nobs"], state=sa, state_cov=sP, lag=lag, r=r,
                filtered=f["au"][:T, :r].copy(), smoothed=sa[:, :r].copy(), smoothed_cov=sP[:, :r, :r].copy(),
                smoothed_agg=sa @ z_low(w, r, sa.shape[1]).T)


def m_step(X, es, low, w, p, update_init, a0, P0):
    """The restricted M-step (Banbura & Modugno 2014): a low-frequency series
    regresses on Z_l alpha_t, and the VAR on the leading rp block."""
    X = np.asarray(X, dtype=np.float64)
    T, N = X.shape
    r = es["r"]
    a, P, lag = es["state"][:T], es["state_cov"][:T], es["lag"][:T]
    s, rp = a.shape[1], r * p
    M2 = a[:, :, None] * a[:, None, :] + P
    f = a[:, :r]
    S11 = M2[1:, :r, :r].sum(axis=0)
    S10 = (f[1:, :, None] * a[:-1, None, :] + lag[1:]).sum(axis=0)
    S00 = M2[:-1].sum(axis=0)
    Zc = (np.hstack([np.eye(r), np.zeros((r, s - r))]), z_low(w, r, s))
    m = ~np.isnan(X)
    x0 = np.where(m, X, 0.0)
    L = np.zeros((N, r))
    sigma2 = np.zeros(N)
    for i in range(N):
        Z = Zc[int(low[i])]
        Si = Z @ M2[m[:, i]].sum(axis=0) @ Z.T
        gi = Z @ (x0[:, i, None] * a).sum(axis=0)
        L[i] = np.linalg.solve(Si, gi)
        sigma2[i] = ((x0[:, i] ** 2).sum() - L[i] @ gi) / m[:, i].sum()
    An = np.linalg.solve(S00[:rp, :rp].T, S10[:, :rp].T).T
    Qn = (S11 - An @ S10[:, :rp].T) / (T - 1)
    Qn = 0.5 * (Qn + Qn.T)
    if update_init:
        a0, P0 = es["state"][0].copy(), es["state_cov"][0].copy()
    return L, sigma2, An, Qn, a0, P0


def em(X, L, sigma2, A, Q, low, w, a0=None, P0=None, tol=1e-4, max_iter=100, update_init=True, horizon=0):
    """The loop of dfm_ss_em with the restricted M-step; the record of ss_em_reference.em plus smoothed_agg."""
    import ss_em_reference as EM
    X = np.asarray(X, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64)).copy()
    sigma2 = np.asarray(sigma2, dtype=np.float64).copy()
    A = np.atleast_2d(np.asarray(A, dtype=np.float64)).copy()
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64)).copy()
    r = L.shape[1]
    p = A.shape[1] // r
    s = r * lags(p, w)
    a0 = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    P0 = S.stationary_kron(padded_A(A, s // r), Q) if P0 is None else np.asarray(P0, dtype=np.float64).copy()
    path, crit, converged, j = [], [], False, 0
    while True:
        es = e_step(X, L, sigma2, A, Q, low, w, a0, P0, horizon)
        path.append(es["loglik"])
        if j >= 1:
            crit.append(EM.criterion(path[j], path[j - 1]))
            if tol > 0 and crit[-1] < tol:
                converged = True
                break
        if j == max_iter:
            break
        L, sigma2, A, Q, a0, P0 = m_step(X, es, low, w, p, update_init, a0, P0)
        j += 1
    return dict(L=L, sigma2=sigma2, A=A, Q=Q, a0=a0, P0=P0, path=np.array(path), crit=np.array(crit), iterations=j,
                converged=converged, loglik=es["loglik"], nobs=es["nobs"], filtered=es["filtered"],
                smoothed=es["smoothed"], smoothed_cov=es["smoothed_cov"], smoothed_agg=es["smoothed_agg"])


EM_CHUNK = (270, 8, 2, 1, AGG_MEAN)   # two K chunks of the M-step GEMM


def perturbed_start(L, sigma2, A, Q, seed=3):
    """A start away from the truth: loadings and A scaled, variances and Q inflated."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (L * (1.0 + 0.2 * rng.standard_normal(L.shape)), sigma2 * 1.5, 0.8 * A, 1.3 * Q)


@functools.lru_cache(maxsize=None)
def em_case(i, max_iter=5):
    """Case i (len(CASES): EM_CHUNK) from a perturbed start: tol = 0, max_iter M-steps, 2 forecast rows (read-only)."""
    T, N, r, p, w = CASES[i] if i < len(CASES) else EM_CHUNK
    X, L, sigma2, A, Q, low = make_case(T, N, r, p, w)
    start = perturbed_start(L, sigma2, A, Q)
    return X, start, low, w, em(X, *start, low, w, tol=0.0, max_iter=max_iter, horizon=2)


BATCH_TOL = 1e-3


@functools.lru_cache(maxsize=None)
def em_batch_case(k):
    """Panel k of the stopping-time batch (the first case's shape, its own
    draw) from a perturbed start at tol = BATCH_TOL, max_iter = 40 (read-only)."""
    T, N, r, p, w = CASES[0]
    X, L, sigma2, A, Q, low = make_case(T, N, r, p, w, seed=k)
    start = perturbed_start(L, sigma2, A, Q, seed=10 + k)
    return X, start, low, w, em(X, *start, low, w, tol=BATCH_TOL, max_iter=40)


# ------------------------------------------------------------------ the fit
def start_values(Zm, F, L, sigma2, low, w):
    """The low series' lambda_i, sigma^2_i by OLS of Zm_ti on sum_k w_k F[t-k]
    over the observed rows t >= n_w - 1 (numpy.linalg.lstsq); the others stay."""
    T, nw = F.shape[0], len(w)
    ft = sum(w[k] * F[nw - 1 - k:T - k] for k in range(nw))
    L, sigma2 = L.copy(), sigma2.copy()
    for i in np.flatnonzero(low):
        z = Zm[nw - 1:, i]
        o = ~np.isnan(z)
        L[i] = np.linalg.lstsq(ft[o], z[o], rcond=None)[0]
        sigma2[i] = ((z[o] - ft[o] @ L[i]) ** 2).sum() / o.sum()
    return L, sigma2


FIT_SHAPE = (60, 14, 2, 1, AGG_FLOW)
FIT_HORIZON = 3


def make_fit_panel():
    """The FIT_SHAPE case in original units: columns rescaled by U(0.5, 3) and shifted by U(-2, 2)."""
    X, _, _, _, _, low = make_case(*FIT_SHAPE)
    rng = np.random.Generator(np.random.PCG64(77))
    return X * rng.uniform(0.5, 3.0, size=X.shape[1]) + rng.uniform(-2.0, 2.0, size=X.shape[1]), low


@functools.lru_cache(maxsize=None)
def fit_case(method):
    """dfm_ss_fit_mf in NumPy: em_reference.em (tol = 0, six iterations),
    ss_reference.estimate, start_values, then the smoother ("two-step") or four
    EM iterations at tol = 0 ("ml"), and the panels (read-only)."""
    import em_reference as E
    T, N, r, p, w = FIT_SHAPE
    X, low = make_fit_panel()
    em0 = E.em(X, r=r, tol=0.0, max_iter=6)
    m = ~np.isnan(X)
    Zm = np.where(m, em0["Z"], np.nan)
    sigma2, A, Q, _ = S.estimate(Zm, em0["F"], em0["L"], p)
    L, sigma2 = start_values(Zm, em0["F"], em0["L"], sigma2, low, w)
    if method == "ml":
        res = em(Zm, L, sigma2, A, Q, low, w, tol=0.0, max_iter=4, horizon=FIT_HORIZON)
        L = res["L"]
    else:
        res = smooth(Zm, L, sigma2, A, Q, low, w, horizon=FIT_HORIZON)
    common = np.where(low, res["smoothed_agg"] @ L.T, res["smoothed"] @ L.T)
    return dict(X=X, low=low, w=w, em=em0, res=res, loglik=res["loglik"],
                x_smoothed=np.where(m, em0["Z"], common[:T]),
                x_completed=np.where(m, X, common[:T] * em0["sd"] + em0["mu"]),
                forecast=common[T:] * em0["sd"] + em0["mu"])
