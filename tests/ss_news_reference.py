"""Two references for the news decomposition as include/dfm.h states it
(dfm_ss_news), and the inputs of tests/test_ss_news_host.py and
tests/test_gpu_ss_news.py.

Route (a), `dense`, uses no Kalman recursion: the joint Gaussian of alpha_0 ..
alpha_{Tt-1} is built densely (the stacked mean and a factor of the stacked
covariance from Tm, Qs, a0 and P0; explicit loading rows as
ss_mf_reference.loading_rows), conditional means come from numpy.linalg.solve
on the shocks' posterior precision (`_condition`), and the weights are the
textbook Cov(alpha_t, I) Var(I)^-1.

Route (b), `recursion`, restates the header: the gains C^c_t, K^c_t, J_t of the
new vintage's filter, then one mean-only impulse recursion per release."""
import functools

import numpy as np

import ss_mf_reference as MF
import ss_reference as S

HORIZON = 2
# of ss_reference.SYNTHETIC; r = 16, p = 2 (s = 32) is the one shape whose lane
# kernel needs more than 64 KB of LDS and fills its prefetch depth exactly
PLAIN = ((33, 33, 1, 1), (40, 72, 16, 2), (60, 40, 5, 3))
N_CASES = len(MF.CASES) + len(PLAIN)
CASE_IDS = MF.CASE_IDS + [f"plain{T}x{N}r{r}p{p}" for T, N, r, p in PLAIN]


# ------------------------------------------------------------------ the model
def _model(L, A, Q, low, w, a0, P0):
    """(r, s, Tm, Qs, a0, P0, Zrows, Z_l) at the state the library keeps: the
    padded one with a low series, the plain one without."""
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    N, r = L.shape
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    mixed = low is not None and bool(np.any(low))
    if mixed:
        A = MF.padded_A(A, MF.lags(A.shape[1] // r, w))
    Tm = S.companion(A)
    s = Tm.shape[0]
    a = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64)
    P = S.stationary_kron(A, Q) if P0 is None else np.asarray(P0, dtype=np.float64)
    if mixed:
        Z, Zl = MF.loading_rows(L, low, w, s), MF.z_low(w, r, s)
    else:
        Z, Zl = np.hstack([L, np.zeros((N, s - r))]), None
    return r, s, Tm, S.state_noise(Q, s), a, P, Z, Zl


def releases_of(X_old, X_new):
    """(J, 2) int64, sorted by (t, i)."""
    return np.argwhere(~np.isnan(X_new) & np.isnan(X_old)).astype(np.int64)


def revised(X_old, X_new):
    return np.where(np.isnan(X_old), np.nan, X_new)


# ------------------------------------------------------- (a) the joint Gaussian
def _psd_root(P):
    lam, U = np.linalg.eigh(0.5 * (P + P.T))
    return U * np.sqrt(np.maximum(lam, 0.0))


def joint_moments(Tm, Qs, a0, P0, Tt):
    """The stacked states alpha = m + Lc eps, eps ~ N(0, I): the mean (Tt s)
    and a factor Lc (Tt s x (s + (Tt - 1) s)) of the stacked covariance V = Lc
    Lc', from alpha_0 = a0 + P0^(1/2) eps_0, alpha_t = Tm alpha_t-1 + Qs^(1/2)
    eps_t written out for every t."""
    s = Tm.shape[0]
    m = np.zeros((Tt, s))
    Lc = np.zeros((Tt, s, Tt, s))
    m[0] = a0
    Lc[0, :, 0, :] = _psd_root(P0)
    Qr = _psd_root(Qs)
    for t in range(1, Tt):
        m[t] = Tm @ m[t - 1]
        Lc[t] = np.einsum("ab,bus->aus", Tm, Lc[t - 1])
        Lc[t, :, t, :] = Qr
    return m.reshape(-1), Lc.reshape(Tt * s, Tt * s)


def _rows(Z, entries, Tt, s):
    """H: one row per entry (t, i), Z[i] in the columns of alpha_t."""
    H = np.zeros((len(entries), Tt * s))
    for k, (t, i) in enumerate(entries):
        H[k, t * s:(t + 1) * s] = Z[i]
    return H


def _condition(Lc, H, var):
    """(B, rhs, Ai) with B rhs = V H' (H V H' + R)^-1, V = Lc Lc', R =
    diag(var): the gain of conditioning on y = H alpha + e, and Var(alpha | y)
    = Lc Ai Lc'.  In the shocks' coordinates y = H m + F eps + e with F = H Lc,
    so eps | y has the precision A = I + F' R^-1 F, symmetric with every
    eigenvalue >= 1 (V itself is singular for p > 1): B = Lc A^-1 Lc', rhs =
    H' R^-1."""
    F = H @ Lc
    Ai = np.linalg.solve(np.eye(Lc.shape[1]) + (F.T / var) @ F, np.eye(Lc.shape[1]))
    Ai = 0.5 * (Ai + Ai.T)
    return Lc @ Ai @ Lc.T, H.T / var, Ai


def dense(X_old, X_new, L, sigma2, A, Q, low=None, w=None, a0=None, P0=None, horizon=0):
    """Everything dfm_ss_news returns, by conditioning the joint Gaussian."""
    X_old, X_new = np.asarray(X_old, dtype=np.float64), np.asarray(X_new, dtype=np.float64)
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    T = X_old.shape[0]
    Tt = T + horizon
    r, s, Tm, Qs, a0, P0, Z, Zl = _model(L, A, Q, low, w, a0, P0)
    m, Lc = joint_moments(Tm, Qs, a0, P0, Tt)
    rel = releases_of(X_old, X_new)
    obs = np.argwhere(~np.isnan(X_old))
    Ho, Hr = _rows(Z, obs, Tt, s), _rows(Z, rel, Tt, s)
    Vpost, rhs, _ = _condition(Lc, Ho, sigma2[obs[:, 1]])   # Var(alpha | the old observed set)
    yo = np.stack([X_old[obs[:, 0], obs[:, 1]], X_new[obs[:, 0], obs[:, 1]]], axis=1) - (Ho @ m)[:, None]
    upd = Vpost @ (rhs @ yo)
    a_old, a_rev = m + upd[:, 0], m + upd[:, 1]
    fc = Hr @ a_rev
    news = X_new[rel[:, 0], rel[:, 1]] - fc
    cov_aI = Vpost @ Hr.T                             # Cov(alpha, I)
    var_I = Hr @ cov_aI + np.diag(sigma2[rel[:, 1]])
    Wt = np.linalg.solve(var_I, cov_aI.T) if len(rel) else np.zeros((0, Tt * s))   # (J, Tt s)
    a_new = a_rev + news @ Wt
    st = lambda v: v.reshape(Tt, s)   # noqa: E731
    Wst = Wt.reshape(len(rel), Tt, s)
    out = dict(releases=rel, news=news, release_forecast=fc, weights_state=Wst, weights_f=Wst[:, :, :r].copy(),
               state_old=st(a_old), state_rev=st(a_rev), state_new=st(a_new), Z=Z, Zl=Zl, r=r)
    out["weights_agg"] = None if Zl is None else Wst @ Zl.T
    return out


def smooth_dense(X, L, sigma2, A, Q, low=None, w=None, a0=None, P0=None, horizon=0):
    """a_t|T (Tt x s) of one panel by conditioning the joint Gaussian."""
    X = np.asarray(X, dtype=np.float64)
    Tt = X.shape[0] + horizon
    r, s, Tm, Qs, a0, P0, Z, _ = _model(L, A, Q, low, w, a0, P0)
    m, Lc = joint_moments(Tm, Qs, a0, P0, Tt)
    obs = np.argwhere(~np.isnan(X))
    H = _rows(Z, obs, Tt, s)
    B, rhs, _ = _condition(Lc, H, np.asarray(sigma2, dtype=np.float64)[obs[:, 1]])
    return (m + B @ (rhs @ (X[obs[:, 0], obs[:, 1]] - H @ m))).reshape(Tt, s)


# --------------------------------------------------- (b) the header's recursion
def gains(X_new, L, sigma2, A, Q, low=None, w=None, a0=None, P0=None, horizon=0):
    """Per row: per class (flag, C, K), and J_t, from the covariance recursion
    of the new vintage's filter."""
    X = np.asarray(X_new, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    r, s, Tm, Qs, _, P, _, Zl = _model(L, A, Q, low, w, a0, P0)
    if horizon:
        X = np.vstack([X, np.full((horizon, X.shape[1]), np.nan)])
    Tt = X.shape[0]
    Zh = np.hstack([np.eye(r), np.zeros((r, s - r))])
    if Zl is None:
        classes = [(Zh, np.ones(L.shape[0], dtype=bool))]
    else:
        lowb = np.asarray(low, dtype=bool)
        classes = [(Zh, ~lowb), (Zl, lowb)]
    mom = [S.collapse(X[:, sel], L[sel], sigma2[sel]) if sel.any() else None for _, sel in classes]
    rows, Pu, Pp = [], np.zeros((Tt, s, s)), np.zeros((Tt, s, s))
    for t in range(Tt):
        Pp[t] = P
        row = []
        for c, (Zc, _) in enumerate(classes):
            if mom[c] is None or not mom[c][3][t] > 0:
                row.append(None)
                continue
            C = mom[c][0][t]
            PZ = P @ Zc.T
            K = PZ @ np.linalg.inv(np.eye(r) + C @ (Zc @ PZ))
            P = P - K @ C @ PZ.T
            P = 0.5 * (P + P.T)
            row.append((C, K))
        rows.append(row)
        Pu[t] = P
        P = Tm @ P @ Tm.T + Qs
    Js = [np.linalg.solve(Pp[t + 1], Tm @ Pu[t]).T for t in range(Tt - 1)]
    return dict(rows=rows, J=Js, Tm=Tm, Z=[Zc for Zc, _ in classes], r=r, s=s, Tt=Tt, ncls=len(classes))


def impulse(g, t_j, cls, beta):
    """c_t|T (Tt x s) of one release."""
    Tt, s, Tm = g["Tt"], g["s"], g["Tm"]
    c = np.zeros(s)
    cf = np.zeros((Tt, s))
    for t in range(Tt):
        for k in range(g["ncls"]):
            if g["rows"][t][k] is None:
                continue
            C, K = g["rows"][t][k]
            d = (beta if (t == t_j and k == cls) else 0.0) - C @ (g["Z"][k] @ c)
            c = c + K @ d
        cf[t] = c
        c = Tm @ c
    cs = cf.copy()
    for t in range(Tt - 2, -1, -1):
        cs[t] = cf[t] + g["J"][t] @ (cs[t + 1] - Tm @ cf[t])
    return cs


def recursion(X_old, X_new, L, sigma2, A, Q, low=None, w=None, a0=None, P0=None, horizon=0):
    """The weights by the header's recursion (the smoothed states are not its subject)."""
    L = np.atleast_2d(np.asarray(L, dtype=np.float64))
    sigma2 = np.asarray(sigma2, dtype=np.float64)
    g = gains(X_new, L, sigma2, A, Q, low, w, a0, P0, horizon)
    rel = releases_of(np.asarray(X_old), np.asarray(X_new))
    mixed = g["ncls"] == 2
    Wst = np.zeros((len(rel), g["Tt"], g["s"]))
    for j, (t, i) in enumerate(rel):
        Wst[j] = impulse(g, t, int(mixed and bool(low[i])), L[i] / sigma2[i])
    return dict(releases=rel, weights_state=Wst, weights_f=Wst[:, :, :g["r"]].copy(),
                weights_agg=Wst @ g["Z"][1].T if mixed else None)


# ------------------------------------------------------------- the generators
def _vintages(X, low, single=False):
    """Two vintages of the panel X (which becomes the new one).

    Releases: every second observed entry of the last six rows; by hand a
    release at row 0, a release that is the only observed entry of its row in
    X_new (the panel's empty row gets one value), and, with low-frequency
    series, one in row 5, which holds low-frequency entries only.  Two old
    values are revised.  single: only the row-0 release (J = 1)."""
    Xn = X.copy()
    T, N = Xn.shape
    empty = int(np.flatnonzero(np.isnan(Xn).all(axis=1))[0])
    Xn[empty, 1 % N] = 0.3
    Xo = Xn.copy()
    first = int(np.flatnonzero(~np.isnan(Xn[0]))[0])
    Xo[0, first] = np.nan
    if not single:
        tail = np.argwhere(~np.isnan(Xn[T - 6:]))
        tail[:, 0] += T - 6
        for t, i in tail[::2]:
            Xo[t, i] = np.nan
        Xo[empty, 1 % N] = np.nan
        if low is not None and np.any(low):
            assert np.isnan(Xn[5, ~np.asarray(low)]).all()
            Xo[5, int(np.flatnonzero(~np.isnan(Xn[5]))[0])] = np.nan
    both = np.argwhere(~np.isnan(Xo))
    for k, (t, i) in enumerate(both[[len(both) // 3, 2 * len(both) // 3]]):
        Xo[t, i] = Xn[t, i] + (0.25 if k else -0.5)
    return Xo, Xn


def inputs(i, single=False):
    """(X_old, X_new, L, sigma2, A, Q, low, w) of case i: the six
    ss_mf_reference.CASES, then the two plain ones (low, w None)."""
    if i < len(MF.CASES):
        X, L, sigma2, A, Q, low = MF.make_case(*MF.CASES[i])
        w = MF.CASES[i][4]
    else:
        X, L, sigma2, A, Q = S.make_synthetic(*PLAIN[i - len(MF.CASES)])
        low, w = None, None
    Xo, Xn = _vintages(X, low, single)
    return Xo, Xn, L, sigma2, A, Q, low, w


@functools.lru_cache(maxsize=None)
def case(i, single=False):
    """Case i with route (a)'s output at HORIZON forecast rows (read-only)."""
    inp = inputs(i, single)
    return inp, dense(*inp, horizon=HORIZON)


def targets(T, N, low):
    """(t, k) pairs: inside the sample, on the ragged edge and in the forecast
    rows; high and (when there are any) low series."""
    ks = [0, N // 2] + ([N - 1] if low is not None and np.any(low) else [])
    return np.array([(t, k) for t in (3, T // 2, T - 2, T - 1, T, T + HORIZON - 1) for k in ks], dtype=np.int64)


def target_values(ref, L, low, tg):
    """old, revised, new (K each) and impacts (K x J) of route (a)."""
    L = np.atleast_2d(L)
    Zk = ref["Z"][tg[:, 1]]                                  # (K, s): the loading row of the target's series
    val = [np.einsum("ks,ks->k", Zk, ref[f"state_{v}"][tg[:, 0]]) for v in ("old", "rev", "new")]
    imp = np.einsum("ks,jks->kj", Zk, ref["weights_state"][:, tg[:, 0], :]) * ref["news"][None, :]
    return val[0], val[1], val[2], imp
