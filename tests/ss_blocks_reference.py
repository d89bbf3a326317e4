"""NumPy restatement of the state-space model with factor blocks as
include/dfm.h states it (dfm_ss_em_blocks, dfm_ss_fit_blocks), and the inputs
of tests/test_ss_blocks_host.py and tests/test_gpu_ss_blocks.py.

The E-step is ss_mf_reference.e_step (the textbook filter on the explicit
loading rows; the plain model is the one without a low-frequency series and
the single weight 1).  The M-step solves, per series, the normal equations of
its free factors and, per block, the regression of its factors on their own
lags, with numpy.linalg.solve on the index sets.  The fit chain is
em_reference.em, per block a symmetric eigendecomposition in dfm_pca's
normalisation, per block an OLS.  Nothing here follows the kernels'
arrangement (unit rows in place of restricted ones, LDS gathers)."""
import functools
import math

import numpy as np

import em_reference as E
import ss_em_reference as EM
import ss_mf_reference as MF
import ss_reference as S

PLAIN_W = (1.0,)


# ------------------------------------------------------------------ the model
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def block_of(sizes):
    """g(j): the block that owns factor j."""
    return np.repeat(np.arange(len(sizes)), sizes)


def free_matrix(sizes, member):
    """free_ij = member[i, g(j)] (N x r, bool)."""
    return np.asarray(member, dtype=bool)[:, block_of(sizes)]


def same_block(sizes, p=1):
    """r x rp: True where A_k may be non-zero."""
    g = block_of(sizes)
    return np.tile(g[:, None] == g[None, :], (1, p))


def all_members(N, sizes):
    return np.ones((N, len(sizes)), dtype=bool)


def moments(X, es, low, w):
    """The sums of the header from an E-step's record: S11, S10, S00 and per
    series (S_i, g_i, q_i, n_i) at its class's regressor."""
    X = np.asarray(X, dtype=np.float64)
    T, N = X.shape
    r = es["r"]
    a, P, lag = es["state"][:T], es["state_cov"][:T], es["lag"][:T]
    s = a.shape[1]
    M2 = a[:, :, None] * a[:, None, :] + P
    f = a[:, :r]
    S11 = M2[1:, :r, :r].sum(axis=0)
    S10 = (f[1:, :, None] * a[:-1, None, :] + lag[1:]).sum(axis=0)
    S00 = M2[:-1].sum(axis=0)
    Zc = (np.hstack([np.eye(r), np.zeros((r, s - r))]), MF.z_low(w, r, s))
    m = ~np.isnan(X)
    x0 = np.where(m, X, 0.0)
    per = []
    for i in range(N):
        Z = Zc[int(low[i])]
        per.append((Z @ M2[m[:, i]].sum(axis=0) @ Z.T, Z @ (x0[:, i, None] * a).sum(axis=0),
                    float((x0[:, i] ** 2).sum()), int(m[:, i].sum())))
    return S11, S10, S00, per


def m_step(X, es, sizes, member, low, w, p, update_init, a0, P0):
    """The exact maximiser under the restrictions."""
    T, N = np.asarray(X).shape
    r = es["r"]
    S11, S10, S00, per = moments(X, es, low, w)
    free = free_matrix(sizes, member)
    L = np.zeros((N, r))
    sigma2 = np.zeros(N)
    for i, (Si, gi, qi, ni) in enumerate(per):
        J = np.flatnonzero(free[i])
        L[i, J] = np.linalg.solve(Si[np.ix_(J, J)], gi[J])
        sigma2[i] = (qi - L[i] @ gi) / ni
    A = np.zeros((r, r * p))
    Q = np.zeros((r, r))
    off = offsets(sizes)
    for g in range(len(sizes)):
        G = np.arange(off[g], off[g + 1])
        c = np.concatenate([k * r + G for k in range(p)])
        Ag = np.linalg.solve(S00[np.ix_(c, c)].T, S10[np.ix_(G, c)].T).T
        A[np.ix_(G, c)] = Ag
        Qg = (S11[np.ix_(G, G)] - Ag @ S10[np.ix_(G, c)].T) / (T - 1)
        Q[np.ix_(G, G)] = 0.5 * (Qg + Qg.T)
    if update_init:
        a0, P0 = es["state"][0].copy(), es["state_cov"][0].copy()
    return L, sigma2, A, Q, a0, P0


def expected_loglik(X, es, low, w, L, sigma2, A, Q):
    """The expected complete-data log-likelihood at (L, sigma2, A, Q) given an
    E-step's moments, up to the terms that hold none of them."""
    T = np.asarray(X).shape[0]
    r = es["r"]
    rp = A.shape[1]
    S11, S10, S00, per = moments(X, es, low, w)
    v = 0.0
    for i, (Si, gi, qi, ni) in enumerate(per):
        v -= 0.5 * (ni * math.log(sigma2[i]) + (qi - 2.0 * L[i] @ gi + L[i] @ Si @ L[i]) / sigma2[i])
    Rm = S11 - A @ S10[:, :rp].T - S10[:, :rp] @ A.T + A @ S00[:rp, :rp] @ A.T
    v -= 0.5 * ((T - 1) * np.linalg.slogdet(Q)[1] + np.trace(np.linalg.solve(Q, Rm)))
    return float(v)


def em(X, L, sigma2, A, Q, sizes, member, low=None, w=PLAIN_W, a0=None, P0=None, tol=1e-4, max_iter=100,
       update_init=True, horizon=0):
    """The loop of dfm_ss_em with the blocks' M-step; the record of ss_mf_reference.em."""
    X = np.asarray(X, dtype=np.float64)
    L = np.atleast_2d(np.asarray(L, dtype=np.float64)).copy()
    sigma2 = np.asarray(sigma2, dtype=np.float64).copy()
    A = np.atleast_2d(np.asarray(A, dtype=np.float64)).copy()
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64)).copy()
    N, r = L.shape
    low = np.zeros(N, dtype=bool) if low is None else np.asarray(low, dtype=bool)
    if not low.any():
        w = PLAIN_W
    p = A.shape[1] // r
    s = r * MF.lags(p, w)
    a0 = np.zeros(s) if a0 is None else np.asarray(a0, dtype=np.float64).copy()
    P0 = S.stationary_kron(MF.padded_A(A, s // r), Q) if P0 is None else np.asarray(P0, dtype=np.float64).copy()
    path, crit, converged, j = [], [], False, 0
    while True:
        es = MF.e_step(X, L, sigma2, A, Q, low, w, a0, P0, horizon)
        path.append(es["loglik"])
        if j >= 1:
            crit.append(EM.criterion(path[j], path[j - 1]))
            if tol > 0 and crit[-1] < tol:
                converged = True
                break
        if j == max_iter:
            break
        L, sigma2, A, Q, a0, P0 = m_step(X, es, sizes, member, low, w, p, update_init, a0, P0)
        j += 1
    return dict(L=L, sigma2=sigma2, A=A, Q=Q, a0=a0, P0=P0, path=np.array(path), crit=np.array(crit), iterations=j,
                converged=converged, loglik=es["loglik"], nobs=es["nobs"], filtered=es["filtered"],
                smoothed=es["smoothed"], smoothed_cov=es["smoothed_cov"], smoothed_agg=es["smoothed_agg"], last=es)


# ------------------------------------------------------------- the generators
def membership(N, sizes):
    """Block 0 is global; series i is a member of group block 1 + i % (n_b - 1),
    and every seventh series of the last block as well."""
    nb = len(sizes)
    mem = np.zeros((N, nb), dtype=bool)
    mem[:, 0] = True
    if nb > 1:
        mem[np.arange(N), 1 + np.arange(N) % (nb - 1)] = True
        mem[3::7, nb - 1] = True
    return mem


def make_case(T, N, sizes, p, w, seed=0, mixed=True, scale=1.0):
    """Parameters that respect the blocks and a panel simulated from them:
    Lambda ~ scale N(0, 1) at the free positions, sigma^2 ~ U(0.3, 1.3), A_1 =
    0.5 I + N(0, 0.05^2) inside the blocks, A_k = N(0, 0.05^2) / k beyond, Q =
    0.5 I.  mixed: the last third of the columns low-frequency, observed at
    t % 3 == 2 only.  Missing: 10 % holes, a 3-row ragged edge on every other
    high-frequency column, row 7 with nothing.  Returns (X, L, sigma2, A, Q,
    low, member)."""
    r = int(sum(sizes))
    rng = np.random.Generator(np.random.PCG64(77100 + 1000 * seed + 100 * T + 10 * r + p + len(sizes)))
    member = membership(N, sizes)
    L = scale * rng.standard_normal((N, r)) * free_matrix(sizes, member)
    sigma2 = rng.uniform(0.3, 1.3, size=N)
    A = np.hstack([(0.5 * np.eye(r) if k == 0 else 0.0) + 0.05 * rng.standard_normal((r, r)) / (k + 1)
                   for k in range(p)]) * same_block(sizes, p)
    assert S.spectral_radius(A) < 0.95
    Q = 0.5 * np.eye(r)
    low = np.zeros(N, dtype=bool)
    if mixed:
        low[N - max(N // 3, 1):] = True
    nw, burn = len(w), 50
    f = np.zeros((T + burn, r))
    for t in range(p, T + burn):
        f[t] = sum(A[:, k * r:(k + 1) * r] @ f[t - 1 - k] for k in range(p)) + math.sqrt(0.5) * rng.standard_normal(r)
    agg = sum(w[k] * f[burn - k:T + burn - k] for k in range(nw))
    f = f[burn:]
    X = np.where(low, agg @ L.T, f @ L.T) + np.sqrt(sigma2) * rng.standard_normal((T, N))
    miss = rng.uniform(size=(T, N)) < 0.10
    nh = N - int(low.sum())
    miss[np.arange(T) % 3 != 2, nh:] = True
    miss[T - 3:, 0:nh:2] = True
    miss[7, :] = True
    X[miss] = np.nan
    return X, L, sigma2, A, Q, low, member


# (T, N, sizes, p, w, mixed, every series in every block): the shapes of the device tests
CASES = ((36, 12, (1, 1, 1), 1, MF.AGG_FLOW, True, False),        # the padded companion
         (40, 14, (2, 1, 1), 2, MF.AGG_MEAN, True, False),        # unequal blocks, a lag gather
         (30, 40, (1,) * 16, 1, (0.5, 0.5), True, False),         # r = 16, s = 32, N beyond one workgroup
         (30, 40, (4, 4, 4, 4), 1, (0.5, 0.5), True, False),
         (48, 12, (1, 1, 1), 1, PLAIN_W, False, False),           # plain
         (36, 12, (2, 1), 1, PLAIN_W, False, True))               # block_members=None: only the VAR is restricted
CASE_IDS = ["36x12b111mf", "40x14b211p2mf", "30x40b1x16mf", "30x40b4444mf", "48x12b111", "36x12b21all"]
EM_ITER = 5


def start_of(i, seed=0):
    """Case i's panel and a perturbed start that keeps the restrictions' zeros."""
    T, N, sizes, p, w, mixed, everyone = CASES[i]
    X, L, sigma2, A, Q, low, member = make_case(T, N, sizes, p, w, seed=seed, mixed=mixed)
    if everyone:
        member = all_members(N, sizes)
        rng = np.random.Generator(np.random.PCG64(5 + seed))
        L = np.where(L == 0.0, 0.3 * rng.standard_normal(L.shape), L)
    return X, MF.perturbed_start(L, sigma2, A, Q, seed=3 + seed), low, member


@functools.lru_cache(maxsize=None)
def em_case(i):
    """Case i from its perturbed start: tol = 0, EM_ITER M-steps, 2 forecast rows (read-only)."""
    T, N, sizes, p, w, mixed, _ = CASES[i]
    X, start, low, member = start_of(i)
    return X, start, low, member, em(X, *start, sizes, member, low, w, tol=0.0, max_iter=EM_ITER, horizon=2)


BATCH_TOL = 1e-3
BATCH_SEEDS = (0, 1, 2, 4, 5, 8)   # draws whose margins |c_j - tol| / tol stay above 0.02


@functools.lru_cache(maxsize=None)
def batch_case(k):
    """Panel k of the stopping-time batch (the first case's shape, its own
    draw and start) at tol = BATCH_TOL, max_iter = 40 (read-only)."""
    T, N, sizes, p, w, mixed, _ = CASES[0]
    X, start, low, member = start_of(0, seed=BATCH_SEEDS[k])
    return X, start, low, member, em(X, *start, sizes, member, low, w, tol=BATCH_TOL, max_iter=40)


def batch_margins():
    """|c_j - tol| / tol over every criterion of every panel of the batch."""
    return np.concatenate([np.abs(batch_case(k)[4]["crit"] - BATCH_TOL) / BATCH_TOL for k in range(len(BATCH_SEEDS))])


# ------------------------------------------------------------------ the fit
def pca(Rg, k):
    """dfm_pca's normalisation (include/dfm.h): T >= N: G = X'X, L = sqrt(N) V,
    F = X L / N; N > T: G = XX', F = sqrt(T) U, L = X'F / T.  Returns (F, L,
    the k + 1 leading eigenvalues)."""
    T, N = Rg.shape
    G = Rg.T @ Rg if T >= N else Rg @ Rg.T
    ev, V = np.linalg.eigh(G)
    ev, V = ev[::-1], V[:, ::-1]
    if T >= N:
        L = math.sqrt(N) * V[:, :k]
        F = Rg @ L / N
    else:
        F = math.sqrt(T) * V[:, :k]
        L = Rg.T @ F / T
    return F, L, ev[:k + 1].copy()


def block_start(Z, Zm, sizes, member, p):
    """Steps 2-3: the blocks' principal components in order, the variances
    over the observed entries, a VAR(p) by OLS per block.  Also the eigengap
    (ev_{r_g} - ev_{r_g + 1}) / ev_{r_g} of every block's PCA."""
    T, N = Z.shape
    r = int(sum(sizes))
    off = offsets(sizes)
    R = Z.copy()
    F, L, gaps = np.zeros((T, r)), np.zeros((N, r)), []
    for g, rg in enumerate(sizes):
        cols = np.flatnonzero(member[:, g])
        Fg, Lg, ev = pca(R[:, cols], rg)
        gaps.append((ev[rg - 1] - ev[rg]) / ev[rg - 1])
        F[:, off[g]:off[g + 1]] = Fg
        L[cols, off[g]:off[g + 1]] = Lg
        R[:, cols] -= Fg @ Lg.T
    m = ~np.isnan(Zm)
    sigma2 = (np.where(m, Zm - F @ L.T, 0.0) ** 2).sum(axis=0) / m.sum(axis=0)
    A, Q = np.zeros((r, r * p)), np.zeros((r, r))
    for g in range(len(sizes)):
        G = np.arange(off[g], off[g + 1])
        Fg = F[:, G]
        Y = Fg[p:]
        Xl = np.hstack([Fg[p - 1 - k:T - 1 - k] for k in range(p)])
        At = np.linalg.solve(Xl.T @ Xl, Xl.T @ Y)
        U = Y - Xl @ At
        c = np.concatenate([k * r + G for k in range(p)])
        A[np.ix_(G, c)] = At.T
        Q[np.ix_(G, G)] = U.T @ U / (T - p)
    return F, L, sigma2, A, Q, np.array(gaps)


def low_start(Zm, F, L, sigma2, low, w, free):
    """A low series' lambda_i, sigma^2_i by OLS on the aggregate of its free factors only."""
    T, nw = F.shape[0], len(w)
    ft = sum(w[k] * F[nw - 1 - k:T - k] for k in range(nw))
    L, sigma2 = L.copy(), sigma2.copy()
    for i in np.flatnonzero(low):
        z = Zm[nw - 1:, i]
        o = ~np.isnan(z)
        J = np.flatnonzero(free[i])
        L[i] = 0.0
        L[i, J] = np.linalg.lstsq(ft[o][:, J], z[o], rcond=None)[0]
        sigma2[i] = ((z[o] - ft[o] @ L[i]) ** 2).sum() / o.sum()
    return L, sigma2


FIT_TN = (60, 18)
FIT_SIZES = ((1, 1, 1), (2, 1, 1))
# draws whose eigengap is at least 0.3 in every block's PCA
FIT_SEEDS = {((1, 1, 1), False): 0, ((1, 1, 1), True): 4, ((2, 1, 1), False): 1, ((2, 1, 1), True): 3}
FIT_HORIZON = 3
FIT_EM_ITER, FIT_ML_ITER = 6, 4
FIT_W = MF.AGG_MEAN


def make_fit_panel(sizes, mixed, seed=None):
    """A FIT_TN panel with strong block factors, in original units: columns
    rescaled by U(0.5, 3) and shifted by U(-2, 2)."""
    T, N = FIT_TN
    seed = FIT_SEEDS[(tuple(sizes), bool(mixed))] if seed is None else seed
    X, _, _, _, _, low, member = make_case(T, N, sizes, 1, FIT_W, seed=seed, mixed=mixed, scale=1.5)
    rng = np.random.Generator(np.random.PCG64(177 + seed))
    return X * rng.uniform(0.5, 3.0, size=N) + rng.uniform(-2.0, 2.0, size=N), low, member


def fit(X, sizes, member, p, method, low=None, w=PLAIN_W, horizon=0, em_iter=FIT_EM_ITER, ml_iter=FIT_ML_ITER):
    """dfm_ss_fit_blocks in NumPy: em_reference.em (tol = 0), block_start,
    low_start, then the smoother ("two-step") or ml_iter EM iterations at tol
    = 0 ("ml"), and the panels."""
    X = np.asarray(X, dtype=np.float64)
    T, N = X.shape
    r = int(sum(sizes))
    low = np.zeros(N, dtype=bool) if low is None else np.asarray(low, dtype=bool)
    if not low.any():
        w = PLAIN_W
    em0 = E.em(X, r=r, tol=0.0, max_iter=em_iter)
    m = ~np.isnan(X)
    Zm = np.where(m, em0["Z"], np.nan)
    F, L, sigma2, A, Q, gaps = block_start(em0["Z"], Zm, sizes, member, p)
    start_L = L
    if low.any():
        L, sigma2 = low_start(Zm, F, L, sigma2, low, w, free_matrix(sizes, member))
    if method == "ml":
        res = em(Zm, L, sigma2, A, Q, sizes, member, low, w, tol=0.0, max_iter=ml_iter, horizon=horizon)
        L, sigma2 = res["L"], res["sigma2"]
    else:
        res = MF.smooth(Zm, L, sigma2, A, Q, low, w, horizon=horizon)
    common = np.where(low, res["smoothed_agg"] @ L.T, res["smoothed"] @ L.T)
    return dict(em=em0, res=res, gaps=gaps, loglik=res["loglik"], sigma2=sigma2, L=L, start_F=F, start_L=start_L,
                x_smoothed=np.where(m, em0["Z"], common[:T]),
                x_completed=np.where(m, X, common[:T] * em0["sd"] + em0["mu"]),
                forecast=common[T:] * em0["sd"] + em0["mu"])


@functools.lru_cache(maxsize=None)
def fit_case(sizes, mixed, method):
    X, low, member = make_fit_panel(sizes, mixed)
    return dict(X=X, low=low, member=member, w=FIT_W,
                **fit(X, sizes, member, 1, method, low if mixed else None, FIT_W, horizon=FIT_HORIZON))
