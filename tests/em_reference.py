"""NumPy restatement of the EM iteration for principal components with missing
observations (Stock & Watson 2002; McCracken & Ng 2016, factors_em with
DEMEAN = 2) as include/dfm.h states it, and the test panels of
tests/test_gpu_em.py / tests/test_em_host.py.  The PCA is the oracle's
(oracle/dfm_oracle.py: scipy eigh(driver="evr"), X'X for T >= N, XX' for
N > T, T == N the first), the criteria are those of src/criteria.jl computed
from the eigenvalues and the trace (V(k) = (trace - sum_{i<=k} ev_i) / (N T))."""
import functools
import math

import numpy as np

import dfm_oracle as O

SHAPES = ((60, 40), (40, 72), (33, 33), (67, 19))
R_TRUE = 3


def make_panel(T: int, N: int):
    """The test panel: r = 3 Gaussian factors and loadings plus sqrt(r) noise,
    columns rescaled by U(0.5, 3) and shifted by U(-2, 2); missing: 15 % at
    random, a 6-row ragged edge on every 5th column, 6 missing leading rows on
    columns 2, 9, 16, ..., row T/2 missing except every 3rd column; column 1
    complete (0-based indices throughout).  Returns (X with NaN, complete X)."""
    rng = np.random.Generator(np.random.PCG64(20261020 + T))
    r = R_TRUE
    f = rng.standard_normal((T, r))
    lam = rng.standard_normal((N, r))
    full = f @ lam.T + math.sqrt(r) * rng.standard_normal((T, N))
    full = full * rng.uniform(0.5, 3.0, size=N) + rng.uniform(-2.0, 2.0, size=N)
    miss = rng.uniform(size=(T, N)) < 0.15
    miss[T - 6:, ::5] = True
    miss[:6, 2::7] = True
    row = np.ones(N, dtype=bool)
    row[::3] = False
    miss[T // 2, row] = True
    miss[:, 1] = False
    X = full.copy()
    X[miss] = np.nan
    return X, full


def regression_inputs(T: int):
    """(y, w) for the model tests: a constant and one regressor, no NaN."""
    rng = np.random.Generator(np.random.PCG64(977 + T))
    return rng.standard_normal(T), np.column_stack([np.ones(T), rng.standard_normal(T)])


def zscore(X2, standardize=True):
    if not standardize:
        return np.zeros(X2.shape[1]), np.ones(X2.shape[1]), X2.copy()
    mu = X2.mean(axis=0)
    sd = X2.std(axis=0, ddof=1)
    return mu, sd, (X2 - mu) / sd


def criterion_values(ev, trace, T, N, kmax, crit):
    """ICp1-3 / BIC for k = 1..kmax from the descending eigenvalues and the trace."""
    NT = float(N) * float(T)
    c = (N + T) / NT
    m = min(T, N)
    out = np.empty(kmax)
    cum = trace
    for k in range(1, kmax + 1):
        cum -= ev[k - 1]
        V = cum / NT
        out[k - 1] = {"ICp1": math.log(V) + k * c * math.log(1.0 / c),
                      "ICp2": math.log(V) + k * c * math.log(m),
                      "ICp3": math.log(V) + k * math.log(m) / m,
                      "BIC": V + k * math.log(T) / T}[crit]
    return out


def pca(Z, r, crit, kmax):
    """(F, L, ev[:r], r): the oracle's PCA at r, or at the first arg-min of crit over 1..kmax."""
    T, N = Z.shape
    F, L, ev = O.principal_components(Z, T, N)
    if r is None:
        r = int(np.argmin(criterion_values(ev, float(np.sum(Z * Z)), T, N, kmax, crit))) + 1
    return F[:, :r], L[:, :r], ev[:r].copy(), r


def em_step(X, C, mu, sd, r, crit="ICp2", kmax=8, standardize=True):
    """One iteration: refill from C with the mu, sd that produced it, z-score, PCA."""
    obs = ~np.isnan(X)
    X2 = np.where(obs, X, C * sd + mu)
    mu, sd, Z = zscore(X2, standardize)
    F, L, ev, rr = pca(Z, r, crit, kmax)
    Cn = F @ L.T
    err = float(np.sum((Cn - C) ** 2) / np.sum(C ** 2))
    return dict(X2=X2, Z=Z, mu=mu, sd=sd, F=F, L=L, ev=ev, r=rr, C=Cn, err=err)


def em(X, r=None, crit="ICp2", kmax=8, tol=1e-6, max_iter=50, standardize=True):
    """The whole iteration.  Returns the last step's record plus `errs`, `rs`
    (per iteration), `iterations`, `converged`, `n_missing`."""
    X = np.asarray(X, dtype=np.float64)
    obs = ~np.isnan(X)
    mu0 = np.nanmean(X, axis=0)
    X2 = np.where(obs, X, mu0)
    mu, sd, Z = zscore(X2, standardize)
    F, L, ev, rr = pca(Z, r, crit, kmax)
    s = dict(X2=X2, Z=Z, mu=mu, sd=sd, F=F, L=L, ev=ev, r=rr, C=F @ L.T, err=math.inf)
    errs, rs, it = [], [rr], 0
    while s["err"] > tol and it < max_iter:
        it += 1
        s = em_step(X, s["C"], s["mu"], s["sd"], r, crit, kmax, standardize)
        errs.append(s["err"])
        rs.append(s["r"])
    s.update(errs=errs, rs=rs, iterations=it, converged=s["err"] <= tol, n_missing=int((~obs).sum()))
    return s


@functools.lru_cache(maxsize=None)
def cached(T, N, r=R_TRUE, tol=1e-6, max_iter=50, standardize=True):
    """Reference runs shared between tests (treat the arrays as read-only)."""
    X, _ = make_panel(T, N)
    return em(X, r=r, tol=tol, max_iter=max_iter, standardize=standardize)


def max_principal_angle(A, B):
    """Largest principal angle between the column spaces of A and B (radians)."""
    Qa, _ = np.linalg.qr(A)
    Qb, _ = np.linalg.qr(B)
    return float(math.asin(min(1.0, np.linalg.norm(Qb - Qa @ (Qa.T @ Qb), 2))))
