"""Matrices with chosen spectra and the checkers of tests/test_gpu_eig.py
(NumPy and SciPy only; tests/test_eig_checks.py shows on the CPU that the
checkers reject wrong outputs).

Exact cases: G = P (H D H' / n (+) diag(e)) P' with H the Sylvester Hadamard
matrix of order n = 2^q <= m, D and e small integers times one power of two,
P a permutation (the diagonal part takes the values of rank 2, 4, .. so
that a tie straddles both parts).  Every entry of G is a sum of at most n integers divided by
n: exact in fp64, so a tie is an exact tie, and the eigenvalues (D and e) and
eigenvectors (columns of H / sqrt(n) and unit vectors) are known without
LAPACK.  Rounded cases: G = V diag(lambda) V' (V from a QR of normals), whose
reference is scipy.linalg.eigh(driver="evr") of the G actually passed.

All residuals are formed in np.longdouble.  Every checker returns the worst
measured / bound ratio and raises AssertionError naming the case.
"""
import functools

import numpy as np
import scipy.linalg as sla

LD = np.longdouble
EPS = 2.0 ** -52
ORTH_BAR = 1e-10      # STAT_RTOL: the loosest figure anything downstream asserts of these vectors
STAGN = 1e-11         # column_verdict: the loosest residual the stagnation clause may accept, times lambda_1
FLOOR = 2e-14         # column_verdict: the rounding floor, times lambda_1
SIGN_MARGIN = 1e-8


def block_p(m, k, block=0):
    """eig_block_p of dfm_eig.hip."""
    p = max(block, k + 1) if block > 0 else max(k + 8, 16)
    return min(p, m)


class Case:
    """G (m x m fp64), lam (all m true eigenvalues, descending, longdouble), V (m x m orthonormal eigenvectors in
    lam's order, longdouble), trace (longdouble), tie (values closer than tie * lam[0] form one cluster)."""

    def __init__(self, name, G, lam, V, trace, tie):
        self.name, self.G, self.lam, self.V, self.trace, self.tie = name, G, lam, V, trace, tie
        self.m = G.shape[0]
        for a in (self.G, self.lam, self.V):
            a.setflags(write=False)

    def clusters(self):
        """[(first, last + 1)] of the runs of true values closer than tie * lam[0] to their neighbour."""
        thr = LD(self.tie) * abs(self.lam[0])
        out, a = [], 0
        for j in range(1, self.m + 1):
            if j == self.m or self.lam[j - 1] - self.lam[j] > thr:
                out.append((a, j))
                a = j
        return out


# ------------------------------------------------------------------ exact cases
def exact_case(name, vals, e2=0, seed=0):
    """vals: m integers, non-increasing; eigenvalues vals * 2^e2.  The m - n diagonal entries take vals[1], vals[3],
    .. (a tie then straddles the Hadamard block and the diagonal part), the Hadamard block the rest."""
    vals = [int(v) for v in vals]
    m = len(vals)
    assert all(vals[j] >= vals[j + 1] for j in range(m - 1)) and max(abs(v) for v in vals + [0]) < 2 ** 26
    n = 1 << (m.bit_length() - 1)
    didx = list(range(1, m, 2))[:m - n]
    hidx = sorted(set(range(m)) - set(didx))
    H = sla.hadamard(n).astype(np.float64) if n > 1 else np.ones((1, 1))
    d = np.array([vals[j] for j in hidx], dtype=np.float64)
    G0 = np.zeros((m, m))
    G0[:n, :n] = ((H * d) @ H.T) / n          # integers below 2^26 n, divided by a power of two: exact
    V0 = np.zeros((m, m), dtype=LD)
    for c, j in enumerate(hidx):
        V0[:n, j] = H[:, c].astype(LD) / np.sqrt(LD(n))
    for c, j in enumerate(didx):
        G0[n + c, n + c] = vals[j]
        V0[n + c, j] = 1
    perm = np.random.default_rng([7100, m, seed]).permutation(m)
    s = 2.0 ** e2
    G = np.ascontiguousarray(G0[np.ix_(perm, perm)] * s)
    lam = np.array(vals, dtype=LD) * LD(s)
    return Case(name, G, lam, np.ascontiguousarray(V0[perm]), lam.sum(), 0.0)


def base_vals(m):
    """48 separated values 1024, 1008, .. 272 above a bulk 256, 255, .. (>= 4 at m = 300)."""
    return [1024 - 16 * j if j < 48 else 256 - (j - 48) for j in range(m)]


def family_vals(fam, m, k, p):
    """The integer spectrum (and power of two) of an exact family at (m, k, p), or None where m is too small
    for it.  Index j is 0-based: the wanted values are v[0 .. k-1]."""
    v, e2 = base_vals(m), 0
    f = fam.rstrip("+-")
    if f == "a":      # geometric 2^-j, j < 24, over a flat tail 2^-24
        v, e2 = [2 ** (24 - j) if j < 24 else 1 for j in range(m)], -24
    elif f == "b":    # lambda_2 = lambda_3, and a triple lambda_{k-4} = lambda_{k-3} = lambda_{k-2} from k = 8 on
        if k < 3:
            return None
        v[2] = v[1]
        if k >= 8:
            v[k - 4] = v[k - 3] = v[k - 5]
    elif f == "c":    # lambda_k = lambda_{k+1} = lambda_{k+2}
        if m < k + 2:
            return None
        v[k] = v[k + 1] = v[k - 1]
    elif f == "d":    # lambda_k = .. = lambda_{k+g+2}, g = p - k guard columns: the tie does not fit the block
        mult = p - k + 3
        if p <= k or m < k - 1 + mult:
            return None
        v[k - 1:k - 1 + mult] = [v[k - 1]] * mult
    elif f == "e":    # exact rank rho = k - 2 < k (k <= 2: G = 0)
        rho = max(k - 2, 0)
        v[rho:] = [0] * (m - rho)
    elif f == "f":    # k < rho < p: dead guard columns
        if p < k + 2:
            return None
        rho = k + (p - k) // 2
        v[rho:] = [0] * (m - rho)
    elif f == "z":    # G = 0
        v = [0] * m
    else:
        raise ValueError(fam)
    if fam.endswith("+"):
        e2 += 100
    if fam.endswith("-"):
        e2 -= 100
    return v, e2


EXACT_FAMILIES = ["a", "b", "c", "d", "e", "f", "z", "a+", "a-", "b+", "b-"]
ROUNDED_FAMILIES = ["g", "h"]


# ---------------------------------------------------------------- rounded cases
def rounded_case(name, lam, seed=0):
    """G = V diag(lam) V' rounded and symmetrised; the reference is LAPACK's dsyevr of that G."""
    m = len(lam)
    rng = np.random.default_rng([7200, m, seed])
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    G = (Q * np.asarray(lam, dtype=np.float64)) @ Q.T
    G = np.ascontiguousarray(0.5 * (G + G.T))
    w, V = sla.eigh(G, driver="evr")
    Gl = G.astype(LD)
    return Case(name, G, w[::-1].astype(LD), np.ascontiguousarray(V[:, ::-1]).astype(LD), np.trace(Gl), 1e-5)


def rounded_lams(fam, m, k, p):
    v = [float(x) for x in base_vals(m)]
    if fam == "g":    # lambda_{k+1} = lambda_k (1 - 1e-6)
        if m < k + 1:
            return None
        v[k] = v[k - 1] * (1.0 - 1e-6)
    elif fam == "h":  # p + 6 values within 1e-6 relative at the top
        c = p + 6
        if m < c:
            return None
        v[:c] = [1024.0 * (1.0 - 1e-6 * j / (c - 1)) for j in range(c)]
    else:
        raise ValueError(fam)
    return v


@functools.lru_cache(maxsize=None)
def make_case(fam, m, k, p):
    """The case of family fam at (m, k, p), or None where it does not exist.  Cached and read-only."""
    name = f"{fam} m={m} k={k} p={p}"
    if fam in ROUNDED_FAMILIES:
        lam = rounded_lams(fam, m, k, p)
        return None if lam is None else rounded_case(name, lam, seed=k)
    fv = family_vals(fam, m, k, p)
    return None if fv is None else exact_case(name, fv[0], fv[1], seed=k)


def scaled(case, e):
    """case times 2^e: the same eigenvectors, every entry and eigenvalue scaled exactly."""
    s = 2.0 ** e
    return Case(f"{case.name} x2^{e}", case.G * s, case.lam * LD(s), case.V.copy(), case.trace * LD(s), case.tie)


def warm_start(case, kw, delta=1e-3):
    """The first kw exact eigenvectors plus delta times normals (m x kw, fp64)."""
    rng = np.random.default_rng([7300, case.m, kw])
    return np.ascontiguousarray(case.V[:, :kw].astype(np.float64) + delta * rng.standard_normal((case.m, kw)))


# --------------------------------------------------------------------- checkers
def _fail(case, what):
    raise AssertionError(f"{case.name}: {what}")


def check_extent(buf, n, case, what):
    """buf: the flat NaN-filled buffer; exactly the first n entries may have been written, and all of them were."""
    buf = np.asarray(buf).ravel()
    if np.isnan(buf[:n]).any():
        _fail(case, f"{what}: {int(np.isnan(buf[:n]).sum())} of {n} entries were never written")
    if not np.isnan(buf[n:]).all():
        _fail(case, f"{what}: written past its extent of {n}")


def residuals(case, lam, U):
    """r_j = G u_j - lam_j u_j in longdouble -> (R as m x k, |r_j|, |u_j|)."""
    Gl, Ul = case.G.astype(LD), np.asarray(U).astype(LD)
    R = Gl @ Ul - Ul * np.asarray(lam).astype(LD)
    return R, np.sqrt((R * R).sum(axis=0)), np.sqrt((Ul * Ul).sum(axis=0))


def _slack(case):
    return LD(case.m) * LD(EPS) * abs(case.lam[0])   # Weyl for the reference's own rounding of G


def check_always(case, k, lam, U, trace, res=None):
    """Holds whatever the status.  lam is non-increasing; with vectors, every lam_j is within |r_j| / |u_j| +
    m 2^-52 lambda_1 of a true eigenvalue; trace is the exact one to m 2^-53 tr."""
    lam = np.asarray(lam, dtype=np.float64)
    if not np.isfinite(lam).all():
        _fail(case, "lam is not finite")
    if (np.diff(lam) > 0).any():
        _fail(case, f"lam increases at {int(np.argmax(np.diff(lam) > 0))}")
    worst = 0.0
    tb = LD(case.m) * LD(2.0 ** -53) * abs(case.trace)
    te = abs(LD(trace) - case.trace)
    if not te <= tb:
        _fail(case, f"trace {trace!r} is {float(te):.3e} from {float(case.trace)!r}, bound {float(tb):.3e}")
    if tb > 0:
        worst = max(worst, float(te / tb))
    if U is not None:
        if not np.isfinite(U).all():
            _fail(case, "Uk is not finite")
        _, rn, un = res or residuals(case, lam, U)
        for j in range(k):
            if not un[j] > 0:
                _fail(case, f"column {j} is zero")
            dist = np.abs(case.lam - LD(lam[j])).min()
            bound = rn[j] / un[j] + _slack(case)
            if not dist <= bound:
                _fail(case, f"lam[{j}] = {lam[j]!r} is {float(dist):.3e} from the spectrum, its residual allows "
                            f"{float(bound):.3e}")
            if bound > 0:
                worst = max(worst, float(dist / bound))
    return worst


def true_gaps(case, k, p, subspace):
    """gap_j of column_verdict on the true values: the neighbours, or lambda_{k+1} in the subspace form (k < p)."""
    L, g = case.lam, []
    for j in range(k):
        if subspace and k < p:
            g.append(abs(L[j] - L[k]))
        else:
            a = abs(L[j] - L[j - 1]) if j > 0 else LD(np.inf)
            b = abs(L[j] - L[j + 1]) if j + 1 < case.m else LD(np.inf)
            g.append(min(a, b))
    return g


def check_strict(case, k, p, lam, U, tol, subspace, res=None):
    """Status 0 under the strict rule: |r_j| <= max(tol gap_j, 1e-11 lambda_1) + m 2^-52 lambda_1, and lam_j is
    the j-th true value to the same figure."""
    _, rn, _ = res or residuals(case, lam, U)
    gaps, worst = true_gaps(case, k, p, subspace), 0.0
    for j in range(k):
        g = gaps[j] if np.isfinite(gaps[j]) else abs(case.lam[0])
        bound = max(LD(tol) * g, LD(STAGN) * abs(case.lam[0])) + _slack(case)
        ev = abs(LD(lam[j]) - case.lam[j])
        if not rn[j] <= bound:
            _fail(case, f"|r_{j}| = {float(rn[j]):.3e} > {float(bound):.3e}")
        if not ev <= bound:
            _fail(case, f"lam[{j}] = {lam[j]!r} is {float(ev):.3e} from lambda_{j} = {float(case.lam[j])!r}, bound "
                        f"{float(bound):.3e}")
        if bound > 0:
            worst = max(worst, float(rn[j] / bound), float(ev / bound))
    return worst


def check_values(case, k, lam, tol):
    """Status 0 under the eigenvalue rule (tol < 0): |lam_j - lambda_j| <= -tol max(|lambda_j|, |tr - sum_{i<k}
    lambda_i|, 1e-6 tr) + 2e-14 lambda_1 + m 2^-52 lambda_1."""
    worst, L = 0.0, case.lam
    energy = abs(case.trace - L[:k].sum())
    for j in range(k):
        bound = LD(-tol) * max(abs(L[j]), energy, LD(1e-6) * abs(case.trace)) + LD(FLOOR) * abs(L[0]) + _slack(case)
        ev = abs(LD(lam[j]) - L[j])
        if not ev <= bound:
            _fail(case, f"lam[{j}] = {lam[j]!r} is {float(ev):.3e} from lambda_{j}, bound {float(bound):.3e}")
        if bound > 0:
            worst = max(worst, float(ev / bound))
    return worst


def check_subspace(case, k, lam, U, res=None):
    """Davis-Kahan (sin Theta theorem, Frobenius form) for every cluster J of true values that lies wholly inside
    the wanted set, at distance g > 0 from every other true value: with R_J = G U_J - U_J diag(lam_J) and the
    lam_J within d of the cluster, |sin Theta(span U_J, eigenspace)|_F <= |R_J|_F / (g - d).  Measured as
    |(I - V_J V_J') U_J|_F / sigma_min(U_J); the bound carries the reference's m 2^-52 lambda_1 beside |R_J|_F
    and m 2^-52 for V's own rounding.  A cluster that crosses the k | k+1 boundary is not compared."""
    R, _, _ = res or residuals(case, lam, U)
    Ul, worst = np.asarray(U).astype(LD), 0.0
    for a, b in case.clusters():
        if b > k:
            break
        L = case.lam
        g = min(L[a - 1] - L[a] if a > 0 else LD(np.inf), L[b - 1] - L[b] if b < case.m else LD(np.inf))
        if not np.isfinite(g):
            continue    # k == m and one cluster: the whole space
        d = max(abs(LD(lam[j]) - L[j]) for j in range(a, b))
        if not g - d > 0:
            _fail(case, f"columns {a}..{b - 1}: lam is {float(d):.3e} from its cluster, the gap is {float(g):.3e}")
        VJ, UJ = case.V[:, a:b], Ul[:, a:b]
        W = UJ - VJ @ (VJ.T @ UJ)
        smin = np.linalg.svd(UJ.astype(np.float64), compute_uv=False).min()
        sin = np.sqrt((W * W).sum()) / LD(smin)
        RJ = R[:, a:b]
        bound = (np.sqrt((RJ * RJ).sum()) + np.sqrt(LD(b - a)) * _slack(case)) / (g - d) + LD(case.m) * LD(EPS)
        if not sin <= bound:
            _fail(case, f"columns {a}..{b - 1}: sin Theta = {float(sin):.3e} > {float(bound):.3e} "
                        f"(|R_J| = {float(np.sqrt((RJ * RJ).sum())):.3e}, gap {float(g):.3e})")
        worst = max(worst, float(sin / bound))
    return worst


def orthonormality(U):
    Ul = np.asarray(U).astype(LD)
    return float(np.abs(Ul.T @ Ul - np.eye(Ul.shape[1], dtype=LD)).max())


def check_orthonormality(case, U):
    """|U'U - I|_max <= 1e-10 (the hard bar; the measured value is returned for the table against LAPACK)."""
    o = orthonormality(U)
    if not o <= ORTH_BAR:
        _fail(case, f"|U'U - I|_max = {o:.3e} > {ORTH_BAR:.0e}")
    return o


def check_signs(case, U):
    """eig_final_body's rule: the largest-|.| entry of a column (first index on ties) is positive; checked
    where it exceeds the runner-up by more than 1e-8.  Returns how many columns were checked."""
    U, n = np.asarray(U), 0
    for j in range(U.shape[1]):
        a = np.abs(U[:, j])
        i0 = int(np.argmax(a))
        rest = np.delete(a, i0)
        if rest.size and a[i0] - rest.max() <= SIGN_MARGIN:
            continue
        n += 1
        if not U[i0, j] > 0:
            _fail(case, f"column {j}: its largest entry U[{i0}] = {U[i0, j]!r} is not positive")
    return n


def lapack_orthonormality(case, k):
    """|U'U - I|_max of dsyevr's top-k vectors of the same G."""
    _, V = sla.eigh(case.G, driver="evr", subset_by_index=[case.m - k, case.m - 1])
    return orthonormality(V)


def verify(case, k, p, lam, U, trace, status, tol, subspace, iters=None, maxit=None):
    """All checks that apply to one replicate's output -> {name: worst share}.  U None: eigenvalue-only."""
    res = None   # the residuals, formed once for the three checks that read them
    if U is not None and np.isfinite(U).all() and np.isfinite(lam).all():
        res = residuals(case, lam, U)
    out = {"always": check_always(case, k, lam, U, trace, res)}
    if status not in (0, 1):
        _fail(case, f"status {status}")
    if status == 1 and iters is not None and iters != maxit:
        _fail(case, f"status 1 with iters = {iters}, maxit = {maxit}")
    if status == 0 and iters is not None and not 0 < iters <= maxit:
        _fail(case, f"status 0 with iters = {iters}")
    if status == 0:
        if tol < 0:
            out["values"] = check_values(case, k, lam, tol)
        elif U is not None:
            out["strict"] = check_strict(case, k, p, lam, U, tol, subspace, res)
    if U is not None:
        out["orth"] = check_orthonormality(case, U)
        check_signs(case, U)
        if status == 0 and tol >= 0:
            out["subspace"] = check_subspace(case, k, lam, U, res)
    return out
