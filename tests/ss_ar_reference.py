"""NumPy restatement of the state-space model with AR(1) idiosyncratic terms
as include/dfm.h states it (dfm_ss_smooth_ar, dfm_ss_estimate_ar,
dfm_ss_ar_fill, dfm_ss_fit_ar) and the inputs of tests/test_ss_ar_host.py,
tests/test_gpu_ss_ar.py and tests/test_gpu_ss_ar_fit.py.

`dense` is the textbook filter and smoother on the state (alpha_t, e_t) with no
measurement noise, x_t = [Lambda 0 | I] (alpha_t, e_t) on the observed rows:
  runwise=True   (a) the run-wise model: at a run start (m_ti = 1, m_{t-1,i} =
                 0) e_ti's transition coefficient is 0 and its innovation
                 variance the stationary one, sigma^2 / (1 - rho^2)
  runwise=False  (b) the exact model: plain AR(1) through holes.
`collapsed` is the header's arrangement: quasi-differenced pair and start
entries collapsed to the 2r x 2r moments.  Then the fill rule, the two-step
estimate of rho, the two-step fit on em_reference.em and the test cases."""
import functools
import math

import numpy as np

import em_reference as E
import ss_reference as SR

LOG2PI = SR.LOG2PI
RHO_MAX = 0.99


def pad_A(A, r):
    """[A 0] at L = max(p, 2) lags."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    L = max(A.shape[1] // r, 2)
    out = np.zeros((r, r * L))
    out[:, :A.shape[1]] = A
    return out


def _prepare(X, L, A, Q, a0, P0, horizon):
    X = np.asarray(X, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    r = L.shape[1]
    Ap = pad_A(A, r)
    Tm = SR.companion(Ap)
    s = Tm.shape[0]
    if horizon:
        X = np.vstack([X, np.full((horizon, X.shape[1]), np.nan)])
    a = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    P = SR.stationary_kron(Ap, Q) if P0 is None else np.asarray(P0, dtype=np.float64).copy()
    return X, L, r, s, Tm, SR.state_noise(Q, s), a, P


def dense(X, L, sigma2, rho, A, Q, a0=None, P0=None, horizon=0, runwise=True):
    """What dfm_ss_smooth_ar returns for one panel, by the dense filter on
    (alpha_t, e_t), and the smoothed e_t|T (`idio`, (T + h) x N)."""
    T = np.asarray(X).shape[0]
    X, L, r, s, Tm, Qs, a, P = _prepare(X, L, A, Q, a0, P0, horizon)
    sigma2, rho = np.asarray(sigma2, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    Tt, N = X.shape
    n = s + N
    m = ~np.isnan(X)
    stat = sigma2 / (1.0 - rho ** 2)
    av = np.concatenate([a, np.zeros(N)])
    Pv = np.zeros((n, n))
    Pv[:s, :s] = P
    Pv[s:, s:] = np.diag(stat)
    au, ap = np.zeros((Tt, n)), np.zeros((Tt, n))
    Pu, Pp = np.zeros((Tt, n, n)), np.zeros((Tt, n, n))
    Tr = np.zeros((Tt, n, n))   # Tr[t]: the transition into row t
    ll, nobs = 0.0, 0
    for t in range(Tt):
        if t > 0:
            coef, var = rho.copy(), sigma2.copy()
            if runwise:
                start = m[t] & ~m[t - 1]
                coef[start], var[start] = 0.0, stat[start]
            Tr[t, :s, :s] = Tm
            Tr[t, s:, s:] = np.diag(coef)
            Qf = np.zeros((n, n))
            Qf[:s, :s] = Qs
            Qf[s:, s:] = np.diag(var)
            av = Tr[t] @ av
            Pv = Tr[t] @ Pv @ Tr[t].T + Qf
        ap[t], Pp[t] = av, Pv
        o = np.flatnonzero(m[t])
        if len(o):
            Z = np.zeros((len(o), n))
            Z[:, :r] = L[o]
            Z[np.arange(len(o)), s + o] = 1.0
            F = Z @ Pv @ Z.T
            F = 0.5 * (F + F.T)
            v = X[t, o] - Z @ av
            K = np.linalg.solve(F, Z @ Pv).T
            ll -= 0.5 * (len(o) * LOG2PI + np.linalg.slogdet(F)[1] + v @ np.linalg.solve(F, v))
            av = av + K @ v
            Pv = Pv - K @ Z @ Pv
            Pv = 0.5 * (Pv + Pv.T)
            nobs += len(o)
        au[t], Pu[t] = av, Pv
    sa, sP = au.copy(), Pu.copy()
    for t in range(Tt - 2, -1, -1):
        J = np.linalg.solve(Pp[t + 1], Tr[t + 1] @ Pu[t]).T
        sa[t] = au[t] + J @ (sa[t + 1] - ap[t + 1])
        sP[t] = Pu[t] + J @ (sP[t + 1] - Pp[t + 1]) @ J.T
    return dict(filtered=au[:T, :r].copy(), smoothed=sa[:, :r].copy(), smoothed_cov=sP[:, :r, :r].copy(),
                loglik=float(ll), nobs=nobs, idio=sa[:, s:].copy())


def collapse(X, L, sigma2, rho):
    """C_t (T x ru x ru), b_t (T x ru), q_t, n_t, l_t of the header, ru = 2r."""
    X = np.asarray(X, dtype=np.float64)
    T, N = X.shape
    r = L.shape[1]
    m = ~np.isnan(X)
    prev = np.vstack([np.zeros((1, N), dtype=bool), m[:-1]])
    pair, start = m & prev, m & ~prev
    xp = np.vstack([np.zeros((1, N)), np.where(m[:-1], X[:-1], 0.0)])
    y = np.where(pair, np.where(m, X, 0.0) - rho * xp, np.where(start, X, 0.0))
    zp = np.hstack([L, -rho[:, None] * L])                   # N x ru
    z0 = np.hstack([L, np.zeros((N, r))])
    vp, v0 = sigma2, sigma2 / (1.0 - rho ** 2)
    C = np.einsum("ti,ia,ib->tab", pair / vp, zp, zp) + np.einsum("ti,ia,ib->tab", start / v0, z0, z0)
    b = (pair * y / vp) @ zp + (start * y / v0) @ z0
    q = (pair * y * y) @ (1.0 / vp) + (start * y * y) @ (1.0 / v0)
    n = m.sum(axis=1).astype(np.float64)
    ell = pair @ np.log(vp) + start @ np.log(v0)
    return C, b, q, n, ell


def collapsed(X, L, sigma2, rho, A, Q, a0=None, P0=None, horizon=0):
    """The header's recursion on the quasi-differenced collapsed moments; the
    record of `dense` without `idio`."""
    T = np.asarray(X).shape[0]
    X, L, r, s, Tm, Qs, a, P = _prepare(X, L, A, Q, a0, P0, horizon)
    sigma2, rho = np.asarray(sigma2, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    ru = 2 * r
    Tt = X.shape[0]
    C, b, q, n, ell = collapse(X, L, sigma2, rho)
    au, ap = np.zeros((Tt, s)), np.zeros((Tt, s))
    Pu, Pp = np.zeros((Tt, s, s)), np.zeros((Tt, s, s))
    ll, nobs = 0.0, 0
    for t in range(Tt):
        ap[t], Pp[t] = a, P
        if n[t] > 0:
            Pff, Pf, af = P[:ru, :ru], P[:, :ru], a[:ru]
            Gi = np.linalg.inv(np.eye(ru) + C[t] @ Pff)
            K = Pf @ Gi
            d = b[t] - C[t] @ af
            ll -= 0.5 * (n[t] * LOG2PI + ell[t] - np.linalg.slogdet(Gi)[1] + q[t] - 2.0 * b[t] @ af
                         + af @ C[t] @ af - d @ Pff @ Gi @ d)
            a = a + K @ d
            P = P - K @ C[t] @ Pf.T
            P = 0.5 * (P + P.T)
            nobs += int(n[t])
        au[t], Pu[t] = a, P
        a = Tm @ a
        P = Tm @ P @ Tm.T + Qs
    sa, sP = SR.rts(dict(au=au, Pu=Pu, ap=ap, Pp=Pp, Tm=Tm))
    return dict(filtered=au[:T, :r].copy(), smoothed=sa[:, :r].copy(), smoothed_cov=sP[:, :r, :r].copy(),
                loglik=float(ll), nobs=nobs)


# ---------------------------------------------------------------- fill, estimate
def fill(X, L, rho, smoothed):
    """The header's fill rule: (T + h) x N."""
    X = np.asarray(X, dtype=np.float64)
    T, N = X.shape
    common = np.asarray(smoothed) @ np.asarray(L).T
    Tt = common.shape[0]
    out = common.copy()
    for i in range(N):
        obs = np.flatnonzero(~np.isnan(X[:, i]))
        ehat = X[obs, i] - common[obs, i]
        out[obs, i] = X[obs, i]
        rh = rho[i]
        for t in range(Tt):
            if t < T and not np.isnan(X[t, i]):
                continue
            k = int(np.searchsorted(obs, t))
            hu, hv = k > 0, k < len(obs)
            if hu and hv:
                d1, d2 = t - obs[k - 1], obs[k] - t
                e = (rh ** d1 * (1 - rh ** (2 * d2)) * ehat[k - 1] + rh ** d2 * (1 - rh ** (2 * d1)) * ehat[k]) / \
                    (1 - rh ** (2 * (d1 + d2)))
            elif hu:
                e = rh ** (t - obs[k - 1]) * ehat[k - 1]
            elif hv:
                e = rh ** (obs[k] - t) * ehat[k]
            else:
                e = 0.0
            out[t, i] = common[t, i] + e
    return out


def estimate_ar(Zm, F, L, p):
    """Steps 2-4 with the two-step estimate of rho: sigma2 (innovation), A, Q,
    P0 (padded form, Kronecker solve), rho."""
    Zm, F, L = (np.asarray(v, dtype=np.float64) for v in (Zm, F, L))
    sigma2, A, Q, _ = SR.estimate(Zm, F, L, p)
    eps = Zm - F @ L.T
    N = Zm.shape[1]
    rho = np.zeros(N)
    for i in range(N):
        e1, e0 = eps[1:, i], eps[:-1, i]
        P = ~np.isnan(e1) & ~np.isnan(e0)
        den = float(np.sum(e0[P] ** 2))
        if P.sum() < 3 or den == 0.0:
            continue
        rho[i] = min(max(float(np.sum(e1[P] * e0[P])) / den, -RHO_MAX), RHO_MAX)
        sigma2[i] = float(np.sum((e1[P] - rho[i] * e0[P]) ** 2)) / P.sum()
    r = F.shape[1]
    return sigma2, A, Q, SR.stationary_kron(pad_A(A, r), Q), rho


def two_step_ar(X, r, p, horizon=0, tol=1e-6, max_iter=50):
    """dfm_ss_fit_ar in NumPy on em_reference.em, with reference (a)."""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    em = E.em(X, r=r, tol=tol, max_iter=max_iter)
    m = ~np.isnan(X)
    Zm = np.where(m, em["Z"], np.nan)
    sigma2, A, Q, P0, rho = estimate_ar(Zm, em["F"], em["L"], p)
    sm = dense(Zm, em["L"], sigma2, rho, A, Q, None, P0, horizon)
    z = fill(Zm, em["L"], rho, sm["smoothed"])
    return dict(em=em, Zm=Zm, sigma2=sigma2, A=A, Q=Q, P0=P0, rho=rho, smooth=sm, loglik=sm["loglik"],
                x_smoothed=z[:T], x_completed=np.where(m, X, z[:T] * em["sd"] + em["mu"]),
                forecast=z[T:] * em["sd"] + em["mu"])


# ------------------------------------------------------------------- the cases
def _single_runs(rng, T, N, lead, tail):
    """A mask of one consecutive run per series: it starts within the first
    `lead` rows and ends within the last `tail` (every third series is complete)."""
    m = np.zeros((T, N), dtype=bool)
    for i in range(N):
        lo = 0 if i % 3 == 0 else int(rng.integers(0, lead + 1))
        hi = T if i % 3 == 0 else T - int(rng.integers(0, tail + 1))
        m[lo:hi, i] = True
    return m


# (T, N, r, p, horizon) of tests/test_gpu_ss_ar.py's shapes 1-5
CASES = ((5, 3, 1, 1, 0), (70, 20, 2, 1, 0), (40, 40, 8, 4, 0), (24, 270, 3, 2, 0), (30, 12, 4, 3, 3))


@functools.lru_cache(maxsize=None)
def case(k):
    """Shape k + 1 of the issue: (X, L, sigma2, rho, A, Q, horizon, single_run).
    |rho| <= 0.9 with mixed signs and rho_1 = 0.  Shapes 1-4 are single-run
    patterns; shape 5 has interior holes, a row without an observed entry
    (row 14: every series restarts at row 15, a row of start entries only)."""
    T, N, r, p, h = CASES[k]
    Xc, L, sigma2, A, Q = SR.make_synthetic(T, N, r, p, complete=True)
    rng = np.random.Generator(np.random.PCG64(9100 + k))
    rho = rng.uniform(-0.9, 0.9, size=N)
    rho[1] = 0.0
    rho[0], rho[2] = 0.9, -0.9
    e = np.zeros((T + 30, N))
    for t in range(1, T + 30):
        e[t] = rho * e[t - 1] + np.sqrt(sigma2) * rng.standard_normal(N)
    X = Xc + e[30:]
    if k == 0:
        m = np.ones((T, N), dtype=bool)
        m[0, 1] = False          # a late starter
        m[3:, 2] = False         # a ragged edge
    elif k == 1:
        m = _single_runs(rng, T, N, 8, 8)
        m[:, 0], m[:, 1], m[:, 2] = True, True, True
        m[64:, 0] = False        # a run that ends at row 63
        m[:64, 1] = False        # a start entry on the second tile's first row
    elif k == 2:
        m = _single_runs(rng, T, N, 6, 6)
    elif k == 3:
        m = _single_runs(rng, T, N, 4, 4)
        m[:, 255], m[:, 256] = True, True
        m[T - 3:, 255] = False   # ragged series on both sides of the K chunks' border
        m[T - 5:, 256] = False
    else:
        m = rng.uniform(size=(T, N)) >= 0.15
        m[:, 0] = True
        m[14, :] = False
        m[15, :] = True
        m[5:8, 3] = False
        m[T - 4:, 5] = False
    X = np.where(m, X, np.nan)
    return X, L, sigma2, rho, A, Q, h, k < 4


@functools.lru_cache(maxsize=None)
def case_reference(k, runwise=True):
    """`dense` on case k (read-only)."""
    X, L, sigma2, rho, A, Q, h, _ = case(k)
    return dense(X, L, sigma2, rho, A, Q, horizon=h, runwise=runwise)


FIT_T, FIT_N, FIT_R, FIT_P, FIT_H = 60, 14, 2, 2, 3
FIT_RAGGED = (8, 13)    # the series of the ragged edge: their last FIT_GAP rows are missing
FIT_GAP = (2, 4)


@functools.lru_cache(maxsize=None)
def fit_panel():
    """The 60 x 14 panel of tests/test_gpu_ss_ar_fit.py: two AR(1) factors,
    AR(1) idiosyncratic terms with rho up to 0.8; late starters (series 1, 9),
    a ragged edge (series 8, 13) and two holes (series 5, 11)."""
    T, N, r = FIT_T, FIT_N, FIT_R
    rng = np.random.Generator(np.random.PCG64(20261021))
    f = np.zeros((T + 50, r))
    e = np.zeros((T + 50, N))
    rho = np.linspace(-0.4, 0.8, N)
    for t in range(1, T + 50):
        f[t] = 0.7 * f[t - 1] + rng.standard_normal(r) * math.sqrt(1.0 - 0.49)
        e[t] = rho * e[t - 1] + rng.standard_normal(N) * np.sqrt(1.0 - rho ** 2)
    lam = rng.standard_normal((N, r))
    X = (f[50:] @ lam.T + e[50:]) * rng.uniform(0.5, 3.0, size=N) + rng.uniform(-2.0, 2.0, size=N)
    X[:5, 1] = X[:9, 9] = np.nan
    for i, g in zip(FIT_RAGGED, FIT_GAP):
        X[T - g:, i] = np.nan
    X[20:23, 5] = X[40, 11] = np.nan
    return X


@functools.lru_cache(maxsize=None)
def fit_reference():
    """The reference chain on fit_panel at tol = 0, six EM iterations (read-only)."""
    return two_step_ar(fit_panel(), FIT_R, FIT_P, horizon=FIT_H, tol=0.0, max_iter=6)
