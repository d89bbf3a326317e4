"""NumPy restatement of the state-space pass as include/dfm.h states it
(dfm_ss_smooth, dfm_ss_estimate, dfm_ss_fit) and the inputs of
tests/test_ss_host.py and tests/test_gpu_ss.py.

Two filters: `filter_brute`, the textbook one on the dense n_t x n_t
innovation covariance F_t = Lambda_o Pff Lambda_o' + R_o (gain P Z' F_t^-1,
slogdet(F_t)) — the reference — and `filter_collapsed`, the header's
arrangement on the r x r collapsed moments C_t, b_t, q_t, n_t, l_t.  Then the
Rauch-Tung-Striebel pass, the stationary covariance by the Kronecker solve
(I - Tm (x) Tm)^-1 vec Qs, the two-step fit on em_reference.em, and the two
generators (fitted panels, drawn parameters)."""
import functools
import math

import numpy as np

import em_reference as E

SHAPES = E.SHAPES                                   # 60x40, 40x72, 33x33, 67x19
TWO_STEP_RP = ((3, 1), (3, 2), (2, 3), (3, 2))      # (r, p) of the two-step panels, in SHAPES order
SYNTHETIC = ((67, 19, 8, 4), (40, 72, 16, 2), (33, 33, 1, 1), (60, 40, 5, 3))   # (T, N, r, p)
HORIZON = 4                                         # forecast rows of the two-step reference fits
LOG2PI = math.log(2.0 * math.pi)


# ------------------------------------------------------------------ the model
def companion(A):
    """Tm of A = [A_1 ... A_p] (r x rp): A on top, the identity shift below."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    r, s = A.shape
    Tm = np.zeros((s, s))
    Tm[:r] = A
    Tm[r:, :s - r] = np.eye(s - r)
    return Tm


def state_noise(Q, s):
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    Qs = np.zeros((s, s))
    Qs[:Q.shape[0], :Q.shape[0]] = Q
    return Qs


def spectral_radius(A):
    return float(np.max(np.abs(np.linalg.eigvals(companion(A)))))


def stationary_kron(A, Q):
    """P = Tm P Tm' + Qs by the Kronecker solve."""
    Tm = companion(A)
    s = Tm.shape[0]
    v = np.linalg.solve(np.eye(s * s) - np.kron(Tm, Tm), state_noise(Q, s).reshape(-1))
    P = v.reshape(s, s)
    return 0.5 * (P + P.T)


def stationary_doubling(A, Q):
    """The header's doubling iteration (what dfm_ss_stationary_cov runs)."""
    M = companion(A)
    P = state_noise(Q, M.shape[0])
    for _ in range(60):
        P = P + M @ P @ M.T
        M = M @ M
        if not (np.isfinite(M).all() and np.isfinite(P).all()):
            raise FloatingPointError("not stationary")
        if np.max(np.abs(M)) < 1e-40:
            return 0.5 * (P + P.T)
    raise FloatingPointError("not stationary")


def _prepare(X, L, sigma2, A, Q, a0, P0, horizon):
    X = np.asarray(X, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    r = L.shape[1]
    Tm = companion(A)
    s = Tm.shape[0]
    if horizon:
        X = np.vstack([X, np.full((horizon, X.shape[1]), np.nan)])
    a = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    P = stationary_kron(A, Q) if P0 is None else np.asarray(P0, dtype=np.float64).copy()
    return X, L, np.asarray(sigma2, dtype=np.float64), r, s, Tm, state_noise(Q, s), a, P


def filter_brute(X, L, sigma2, A, Q, a0=None, P0=None, horizon=0):
    """The textbook filter.  Returns au, Pu (a_t|t, P_t|t), ap, Pp (a_t|t-1,
    P_t|t-1; row 0 is a0, P0), loglik, nobs — rows t = 0..T+h-1."""
    X, L, sigma2, r, s, Tm, Qs, a, P = _prepare(X, L, sigma2, A, Q, a0, P0, horizon)
    Tt = X.shape[0]
    au, ap = np.zeros((Tt, s)), np.zeros((Tt, s))
    Pu, Pp = np.zeros((Tt, s, s)), np.zeros((Tt, s, s))
    ll, nobs = 0.0, 0
    for t in range(Tt):
        ap[t], Pp[t] = a, P
        o = ~np.isnan(X[t])
        n = int(o.sum())
        if n:
            Z = np.zeros((n, s))
            Z[:, :r] = L[o]
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


def collapse(X, L, sigma2):
    """C_t (T x r x r), b_t (T x r), q_t, n_t, l_t (T each) of the header."""
    X = np.asarray(X, dtype=np.float64)
    m = ~np.isnan(X)
    x0 = np.where(m, X, 0.0)
    w = 1.0 / sigma2
    C = np.einsum("ti,ia,ib->tab", m.astype(np.float64), L * w[:, None], L)
    b = x0 @ (L * w[:, None])
    q = (x0 * x0) @ w
    n = m.sum(axis=1).astype(np.float64)
    ell = m.astype(np.float64) @ np.log(sigma2)
    return C, b, q, n, ell


def filter_collapsed(X, L, sigma2, A, Q, a0=None, P0=None, horizon=0):
    """The header's recursion on the collapsed moments; same record as filter_brute."""
    X, L, sigma2, r, s, Tm, Qs, a, P = _prepare(X, L, sigma2, A, Q, a0, P0, horizon)
    Tt = X.shape[0]
    C, b, q, n, ell = collapse(X, L, sigma2)
    au, ap = np.zeros((Tt, s)), np.zeros((Tt, s))
    Pu, Pp = np.zeros((Tt, s, s)), np.zeros((Tt, s, s))
    ll, nobs = 0.0, 0
    for t in range(Tt):
        ap[t], Pp[t] = a, P
        if n[t] > 0:
            Pff, Pf, af = P[:r, :r], P[:, :r], a[:r]
            G = np.eye(r) + C[t] @ Pff
            Gi = np.linalg.inv(G)
            K = Pf @ Gi
            d = b[t] - C[t] @ af
            ll -= 0.5 * (n[t] * LOG2PI + ell[t] + np.linalg.slogdet(G)[1] + q[t] - 2.0 * b[t] @ af
                         + af @ C[t] @ af - d @ Pff @ Gi @ d)
            a = a + K @ d
            P = P - K @ C[t] @ Pf.T
            P = 0.5 * (P + P.T)
            nobs += int(n[t])
        au[t], Pu[t] = a, P
        a = Tm @ a
        P = Tm @ P @ Tm.T + Qs
    return dict(au=au, Pu=Pu, ap=ap, Pp=Pp, loglik=float(ll), nobs=nobs, Tm=Tm, r=r)


def rts(f):
    """Rauch-Tung-Striebel pass over a filter's record: (a_t|T, P_t|T)."""
    au, Pu, ap, Pp, Tm = f["au"], f["Pu"], f["ap"], f["Pp"], f["Tm"]
    Tt = au.shape[0]
    sa, sP = au.copy(), Pu.copy()
    for t in range(Tt - 2, -1, -1):
        J = np.linalg.solve(Pp[t + 1], Tm @ Pu[t]).T
        sa[t] = au[t] + J @ (sa[t + 1] - ap[t + 1])
        sP[t] = Pu[t] + J @ (sP[t + 1] - Pp[t + 1]) @ J.T
    return sa, sP


def smooth(X, L, sigma2, A, Q, a0=None, P0=None, horizon=0, method="brute"):
    """What dfm_ss_smooth returns for one panel."""
    T = np.asarray(X).shape[0]
    f = (filter_brute if method == "brute" else filter_collapsed)(X, L, sigma2, A, Q, a0, P0, horizon)
    sa, sP = rts(f)
    r = f["r"]
    return dict(filtered=f["au"][:T, :r].copy(), smoothed=sa[:, :r].copy(), smoothed_cov=sP[:, :r, :r].copy(),
                loglik=f["loglik"], nobs=f["nobs"], state=sa, state_cov=sP, Tm=f["Tm"])


# ------------------------------------------------------------ the two-step fit
def estimate(Zm, F, L, p):
    """Steps 2-4: sigma^2, A (r x rp), Q, P0 (Kronecker solve)."""
    Zm, F, L = (np.asarray(v, dtype=np.float64) for v in (Zm, F, L))
    T, r = F.shape
    m = ~np.isnan(Zm)
    res = np.where(m, Zm - F @ L.T, 0.0)
    sigma2 = (res ** 2).sum(axis=0) / m.sum(axis=0)
    Y = F[p:]
    Xl = np.hstack([F[p - 1 - k:T - 1 - k] for k in range(p)])
    At = np.linalg.solve(Xl.T @ Xl, Xl.T @ Y)
    U = Y - Xl @ At
    Q = U.T @ U / (T - p)
    A = At.T.copy()
    return sigma2, A, Q, stationary_kron(A, Q)


def two_step(X, r, p, horizon=0, tol=1e-6, max_iter=50):
    """dfm_ss_fit in NumPy on em_reference.em."""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    em = E.em(X, r=r, tol=tol, max_iter=max_iter)
    m = ~np.isnan(X)
    Zm = np.where(m, em["Z"], np.nan)
    sigma2, A, Q, P0 = estimate(Zm, em["F"], em["L"], p)
    sm = smooth(Zm, em["L"], sigma2, A, Q, None, P0, horizon)
    common = sm["smoothed"] @ em["L"].T
    return dict(em=em, Zm=Zm, sigma2=sigma2, A=A, Q=Q, P0=P0, smooth=sm, loglik=sm["loglik"],
                x_smoothed=np.where(m, em["Z"], common[:T]),
                x_completed=np.where(m, X, common[:T] * em["sd"] + em["mu"]),
                forecast=common[T:] * em["sd"] + em["mu"])


# ------------------------------------------------------------- the generators
def make_two_step_panel(T, N):
    """A panel for the two-step fit: three AR(1) factors (rho = 0.7, 50 rows of
    burn-in), Gaussian loadings, sqrt(3) noise, columns rescaled by U(0.5, 3)
    and shifted by U(-2, 2) as em_reference.make_panel.  Missing: 15 % at
    random; a 6-row ragged edge on every 5th column; 6 leading rows on columns
    2, 9, ...; column 1 complete but for: row T/2 wholly missing; the last row
    observed on its first three columns only."""
    rng = np.random.Generator(np.random.PCG64(20261021 + T))
    r = 3
    u = rng.standard_normal((T + 50, r)) * math.sqrt(1.0 - 0.7 ** 2)
    f = np.zeros((T + 50, r))
    for t in range(1, T + 50):
        f[t] = 0.7 * f[t - 1] + u[t]
    f = f[50:]
    lam = rng.standard_normal((N, r))
    full = f @ lam.T + math.sqrt(r) * rng.standard_normal((T, N))
    full = full * rng.uniform(0.5, 3.0, size=N) + rng.uniform(-2.0, 2.0, size=N)
    miss = rng.uniform(size=(T, N)) < 0.15
    miss[T - 6:, ::5] = True
    miss[:6, 2::7] = True
    miss[:, 1] = False
    miss[T // 2, :] = True
    miss[T - 1, :] = True
    miss[T - 1, :3] = False
    X = full.copy()
    X[miss] = np.nan
    return X


def _scaled_var(A0, r, p, c):
    return np.hstack([A0[:, k * r:(k + 1) * r] * c ** (k + 1) for k in range(p)])


def make_synthetic(T, N, r, p, complete=False):
    """Parameters drawn directly and a panel simulated from them: Lambda ~
    N(0, 1), sigma^2 ~ U(0.5, 2), A random r x rp with lag block k scaled by
    c^k so that the spectral radius is 0.8, Q = G G'/r + 0.5 I.  Missing: 20 %
    at random, a 5-row edge on every 4th column, row T/2 wholly missing, the
    last row observed on its first two columns.  Returns (X, L, sigma2, A, Q);
    complete=True returns the panel before the entries are removed."""
    rng = np.random.Generator(np.random.PCG64(7000 + 100 * T + 10 * r + p))
    L = rng.standard_normal((N, r))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    A0 = rng.standard_normal((r, r * p)) / math.sqrt(r)
    lo, hi = 0.0, 1.0
    while spectral_radius(_scaled_var(A0, r, p, hi)) < 0.8:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if spectral_radius(_scaled_var(A0, r, p, mid)) < 0.8:
            lo = mid
        else:
            hi = mid
    A = _scaled_var(A0, r, p, lo)
    G = rng.standard_normal((r, r))
    Q = G @ G.T / r + 0.5 * np.eye(r)
    Qc = np.linalg.cholesky(Q)
    f = np.zeros((T + 50 + p, r))
    for t in range(p, T + 50 + p):
        f[t] = sum(A[:, k * r:(k + 1) * r] @ f[t - 1 - k] for k in range(p)) + Qc @ rng.standard_normal(r)
    f = f[50 + p:]
    X = f @ L.T + np.sqrt(sigma2) * rng.standard_normal((T, N))
    miss = rng.uniform(size=(T, N)) < 0.20
    miss[T - 5:, ::4] = True
    miss[T // 2, :] = True
    miss[T - 1, :] = True
    miss[T - 1, :2] = False
    if not complete:
        X[miss] = np.nan
    return X, L, sigma2, A, Q


@functools.lru_cache(maxsize=None)
def two_step_case(i):
    """Two-step panel i (SHAPES order) and its reference fit at tol = 0, six
    iterations, HORIZON forecast rows (read-only)."""
    T, N = SHAPES[i]
    r, p = TWO_STEP_RP[i]
    X = make_two_step_panel(T, N)
    return X, two_step(X, r, p, horizon=HORIZON, tol=0.0, max_iter=6)


@functools.lru_cache(maxsize=None)
def synthetic_case(i):
    """Synthetic set i with its reference smoother output (read-only)."""
    X, L, sigma2, A, Q = make_synthetic(*SYNTHETIC[i])
    return X, L, sigma2, A, Q, smooth(X, L, sigma2, A, Q)


def two_pass_case(M=9, horizon=4088):
    """(panels, L, sigma2, A, Q, horizon): M tiny panels whose workspace is
    large — T = 8, N = 4, r = 8, p = 4 (s = 32) and many forecast rows — so
    that the half-GB rule of the drivers splits them into two passes: at Tt =
    4096 the smoother's M = 9 into 7 and 2.  The parameters are those of
    tools/ss_bench.py::parameters."""
    T, N, r, p = 8, 4, 8, 4
    rng = np.random.default_rng(23)
    L = rng.standard_normal((N, r))
    sigma2 = rng.uniform(0.5, 2.0, size=N)
    A = np.hstack([0.5 * np.eye(r)] + [0.2 / k * np.eye(r) for k in range(1, p)])
    panels = rng.standard_normal((M, T, N))
    panels[2, 3, 1] = panels[7, 0, 2] = panels[8, 5, :] = np.nan
    return panels, L, sigma2, A, np.eye(r), horizon


def smoother_inputs():
    """Every (label, X, L, sigma2, A, Q, P0) the smoother tests run: the four
    two-step panels with the reference's fitted parameters, then the four
    synthetic sets (P0 None: the stationary covariance)."""
    out = []
    for i, (T, N) in enumerate(SHAPES):
        _, ts = two_step_case(i)
        out.append((f"fit{T}x{N}", ts["Zm"], ts["em"]["L"], ts["sigma2"], ts["A"], ts["Q"], ts["P0"]))
    for i, (T, N, r, p) in enumerate(SYNTHETIC):
        X, L, sigma2, A, Q, _ = synthetic_case(i)
        out.append((f"syn{T}x{N}r{r}p{p}", X, L, sigma2, A, Q, None))
    return out
