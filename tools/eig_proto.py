"""CPU prototype (NumPy) of the factored bootstrap's eigen-iteration at the C3
shape, to explore warm starts and filter schedules before touching kernels:
block p = 16, Rayleigh-Ritz with CholQR, Chebyshev filter on [0, theta_p],
the eigenvalue (Kato-Temple) stopping rule of decide_converged (1e-12).
Reports loop steps and G-products per replicate, the worst relative error of
the retired eigenvalues against LAPACK and the worst column-normalised
condition number of the block the step after the first filter orthonormalises
(r / w schedules also: the largest theta_p / theta_k of the first step, the
level at which filter_end's guard branch would bind).
  python tools/eig_proto.py [nrep] [schedule ...]   schedule e.g. "r8:2,2" "w16:2,2" "w16:3,2"
Schedules: <start><kw>[@beta]:<deg0>,<deg1>
  r / w  warm start of kw base eigenvectors + raw random guards, a
         Rayleigh-Ritz step first; @beta: first interval end max(theta_p, beta theta_k)
  f      the same start with the guards orthonormalised against the warm
         vectors and each other, and NO first Rayleigh-Ritz step: step 0 is the
         degree-deg0 filter alone on [0, beta lambda_k(base fit)] (a constant
         of the model); g: the same with raw guards
Environment: P (block), SHAPE=c1|c2|small (small: T = 120, N = 300, R = 8),
R, TOL, STRICT=1, JACOBI=n (model eig_small's n threshold-Jacobi sweeps per
Rayleigh-Ritz step instead of LAPACK's eigh; JACOBI_FIRST: the sweeps of the
f / g schedules' first Rayleigh-Ritz step, which no earlier step has
pre-rotated); F32=n (f / g schedules): the first n products of the filter-only
step 0 apply the idiosyncratic part E* E*' of G* = (G* - E* E*') + E* E*' as
float32(E* E*') @ float32(S) (sgemm, fp32 accumulation) — the GPU's fp32
middle products, which round H and Z and keep the factor part in fp64;
NOISE=x: Gaussian noise of x 6e-8 ||column|| / sqrt(T) per entry added to that
part (the margin over fp32 rounding); TERMS=t1,t2,... (with F32): how step 0's
product 1, 2, ... applies that part instead of sgemm — 6, 3 or 1: as that many
bf16 plane pairs of (E* E*' / hmax) and S, the GPU's split products
(tests/test_bf16_split_model.py: split3 and split_matmul's fp32 accumulation
per 16-deep stage; 3 = (m,h) (h,m) (h,h), 1 = (h,h)); M >= 8: both operands
rounded to M significand bits, the product in fp64.  Products past the list
stay sgemm.  NOISE applies on top as before."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamicfactormodels.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import host  # noqa: E402
from test_bf16_split_model import SIX, split_matmul  # noqa: E402

T, N, R = 500, 2000, 8
P = int(os.environ.get("P", "16"))
JACOBI = int(os.environ.get("JACOBI", "0"))
JACOBI_FIRST = int(os.environ.get("JACOBI_FIRST", str(JACOBI)))   # f / g: sweeps of the first Rayleigh-Ritz step
F32 = int(os.environ.get("F32", "0"))          # f / g: step 0's first F32 products with the E* E*' part in float32
NOISE = float(os.environ.get("NOISE", "0"))    # ... plus this many times fp32's rounding noise
TERMS = [int(v) for v in os.environ.get("TERMS", "").split(",") if v]   # ... per product: plane pairs, or bits
PAIRS = {6: SIX, 3: ((1, 0), (0, 1), (0, 0)), 1: ((0, 0),)}


def shifted_cheb(d):
    t0, t1 = np.zeros(d + 1), np.zeros(d + 1)
    t0[0] = 1.0
    if d == 0:
        return t0
    t1[0], t1[1] = -1.0, 2.0
    for _ in range(1, d):
        t2 = -2.0 * t1 - t0
        t2[1:] += 4.0 * t1[:-1]
        t0, t1 = t1, t2
    return t1


def jacobi(H, sweeps):
    """eig_small's parallel cyclic Jacobi: circle-method rounds of disjoint
    pairs, a pair rotated only while |h_ab| > 4 eps sqrt(|h_aa h_bb|), the
    sweep loop ending at the first sweep that rotates nothing.  Returns the
    diagonal (NOT sorted) and the accumulated rotations."""
    p = H.shape[0]
    n = p + (p & 1)
    H = H.copy()
    V = np.eye(p)
    order = list(range(n))
    for _ in range(sweeps):
        rotated = False
        for _ in range(n - 1):
            J = np.eye(p)
            for i in range(n // 2):
                a, b = sorted((order[i], order[n - 1 - i]))
                if b >= p:
                    continue
                hab, haa, hbb = H[a, b], H[a, a], H[b, b]
                if abs(hab) > 1e-300 and hab * hab > 7.921e-31 * abs(haa * hbb):
                    zeta = (hbb - haa) / (2.0 * hab)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = t * c
                    J[a, a] = J[b, b] = c
                    J[a, b], J[b, a] = s, -s
                    rotated = True
            H = J.T @ H @ J
            V = V @ J
            order = [order[0], order[-1]] + order[1:-1]
        if not rotated:
            break
    return np.diag(H).copy(), V


def colcond(Q):
    return np.linalg.cond(Q / np.linalg.norm(Q, axis=0))


def round_bits(x, m):
    """x rounded to m significand bits (round to nearest even)."""
    f, e = np.frexp(x)
    return np.ldexp(np.rint(np.ldexp(f, m)), e - m)


def lowp_product(G, Hs, S, nrng, sp=0):
    """G S with the part Hs S (Hs = E* E*') in float32: rounded operands, fp32 accumulation, optional noise.
    sp (1-based) picks the product's entry of TERMS, if it has one."""
    t = TERMS[sp - 1] if 0 < sp <= len(TERMS) else 0
    if t in PAIRS:
        hmax = Hs.diagonal().max()
        W = hmax * split_matmul(Hs / hmax, S, PAIRS[t])
    elif t >= 8:
        W = round_bits(Hs, t) @ round_bits(S, t)
    elif t:
        raise ValueError(f"TERMS: {t} (6, 3, 1 plane pairs or >= 8 bits)")
    else:
        W = (Hs.astype(np.float32) @ S.astype(np.float32)).astype(np.float64)
    if NOISE > 0.0:
        W = W + nrng.standard_normal(W.shape) * (NOISE * 6e-8 * np.linalg.norm(W, axis=0) / np.sqrt(W.shape[0]))
    return (G - Hs) @ S + W


def solve(G, Q0, degs, k=R, tol=1e-12, maxit=30, beta=0.0, strict=False, bfix=0.0, Hs=None, nrng=None):
    """-> (loop steps, products, Rayleigh-Ritz steps, theta[:k] at retirement, cond after the first filter,
    theta_p / theta_k of a Rayleigh-Ritz step on the start block: filter_end's guard branch binds when it exceeds beta)"""
    Q = Q0.copy()
    tr = np.trace(G)
    prods = 0
    it0 = 0
    cond = 0.0
    gratio = 0.0
    if bfix > 0.0:   # step 0: the filter alone, S_d = a_d Q0, S_i = G S_{i+1} / b + a_i Q0
        a = shifted_cheb(degs[0])
        S = a[degs[0]] * Q0
        for i in range(degs[0] - 1, -1, -1):
            low = Hs is not None and prods < F32
            S = (lowp_product(G, Hs, S, nrng, prods + 1) if low else G @ S) / bfix + a[i] * Q0
            prods += 1
        Q = S
        it0 = 1
    th = np.zeros(P)
    for it in range(it0, maxit):
        if it == 1:
            cond = colcond(Q)
        Y = G @ Q
        prods += 1
        L = np.linalg.cholesky(Q.T @ Q)
        Li = np.linalg.inv(L)
        Hm = Li @ (Q.T @ Y) @ Li.T
        Hm = 0.5 * (Hm + Hm.T)
        if JACOBI:
            th, V = jacobi(Hm, JACOBI_FIRST if it0 and it == 1 else JACOBI)
        else:
            th, V = np.linalg.eigh(Hm)
        o = np.argsort(-th, kind="stable")
        th, V = th[o], V[:, o]
        if it == 0:
            gratio = th[P - 1] / th[k - 1]
        A = Li.T @ V
        U = Q @ A
        Res = Y @ A - U * th
        res2 = np.sum(Res ** 2, axis=0)
        gap = np.full(P, np.inf)
        gap[1:] = np.minimum(gap[1:], np.abs(th[1:] - th[:-1]))
        gap[:-1] = np.minimum(gap[:-1], np.abs(th[:-1] - th[1:]))
        if strict:   # subspace rule: res_j <= tol |theta_j - theta_k|
            res = np.sqrt(res2[:k])
            if np.all((res <= tol * np.abs(th[:k] - th[k])) | (res <= 2e-14 * th[0])):
                return it + 1, prods, it + 1 - it0, th[:k], cond, gratio
        else:
            bnd = res2[:k] / (0.5 * gap[:k])
            ok = np.all((bnd <= tol * np.abs(th[:k])) | (np.sqrt(res2[:k]) <= 2e-14 * th[0]))
            vnum = max(abs(tr - th[:k].sum()), 1e-6 * abs(tr))
            if ok and bnd.sum() <= tol * vnum:
                return it + 1, prods, it + 1 - it0, th[:k], cond, gratio
        ZZ = A.T @ (Y.T @ Y) @ A
        L2 = np.linalg.cholesky(0.5 * (ZZ + ZZ.T))
        Bm = A @ np.linalg.inv(L2).T
        d = degs[min(it, len(degs) - 1)]
        b = th[P - 1]
        if it == 0 and beta > 0:   # first filter: interval end from the wanted Ritz values
            b = max(b, beta * th[k - 1])
        a = shifted_cheb(d)
        K = Q @ Bm                       # K_0
        X = a[0] * K
        Kn = Y @ Bm                      # K_1 = G K_0
        X = X + (a[1] / b) * Kn
        for s in range(2, d + 1):
            Kn = G @ Kn
            prods += 1
            X = X + (a[s] / b ** s) * Kn
        Q = X
    return maxit, prods, maxit - it0, th[:k], cond, gratio


def main():
    nrep = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    scheds = sys.argv[2:] or ["r8:2", "w16:2", "w16:3,2", "w16:4,2", "w24:2"]
    global T, N, R
    c2 = os.environ.get("SHAPE") in ("c2", "c1")
    c1 = os.environ.get("SHAPE") == "c1"
    strict = c2 or os.environ.get("STRICT") == "1"
    if c1:   # tools/bench_configs.py c1: T = 200, N = 100, r = 3 (the fit itself: one Gram)
        T, N = 200, 100
        rng = np.random.default_rng(20261015 + 1)
        y, x, *_ = host.factor_model_DGP(T, N, 3, rng=rng)
        R = 3
    elif c2:   # tools/bench_configs.py c2: T = 600, N = 130, Breitung-Eickmeier DGP, r = 4 (ICp2)
        T, N = 600, 130
        rng = np.random.default_rng(20261015 + 2)
        y, x, *_ = host.factor_model_DGP(T, N, 3, model="Breitung_Eickmeier_2011", b=0.5, rng=rng)
        R = int(os.environ.get("R", "4"))
    elif os.environ.get("SHAPE") == "small":   # the GPU tests' small shape
        T, N = 120, 300
        R = int(os.environ.get("R", "8"))
        rng = np.random.default_rng(8180)
        y, x, *_ = host.factor_model_DGP(T, N, R, rng=rng)
    else:
        rng = np.random.default_rng(20261015 + 3)
        y, x, *_ = host.factor_model_DGP(T, N, R, rng=rng)
    x = host.normalize(x)
    if c2:   # T >= N: the N x N Gram, eigenvectors = loadings directions
        x = x.T
        T, N = N, T
    G0 = x @ x.T
    lam, Uall = np.linalg.eigh(G0)
    lam, Uall = lam[::-1], Uall[:, ::-1]
    F = np.sqrt(T) * Uall[:, :R]
    Lb = x.T @ F / T
    C = F @ Lb.T
    E = x - C
    Tr = x.shape[1] if c2 else T   # rows resampled: the panel's time dimension
    idx, eta = host.draw_wild_fast(1_000_003, nrep, Tr)
    hrng = np.random.default_rng(5)
    rnd = hrng.uniform(-1, 1, size=(T, P))

    def gram(b):   # -> G*, and E* E*' (the part the GPU's fp32 products apply) where F32 asks for it
        if c2:   # rows of the T x N panel are columns here
            Xs = C + eta[b][None, :] * E[:, idx[b]]
            return Xs @ Xs.T, None
        Es = eta[b][:, None] * E[idx[b]]
        Xs = C + Es
        return Xs @ Xs.T, (Es @ Es.T if F32 > 0 else None)

    truth = {}
    for sc in scheds:
        start, degs = sc.split(":")
        degs = [int(v) for v in degs.split(",")]
        beta = 0.0
        if "@" in start:
            start, beta = start.split("@")
            beta = float(beta)
        kw = min(int(start[1:]), P)
        Q0 = np.hstack([Uall[:, :kw], rnd[:, kw:]])
        bfix = 0.0
        if start[0] in "fg":
            bfix, beta = beta * lam[R - 1], 0.0
        if start[0] == "f":   # guards: one projection off the warm vectors, CholQR among themselves
            W, Gd = Q0[:, :kw], Q0[:, kw:]
            Gd = Gd - W @ (W.T @ Gd)
            Gd = Gd @ np.linalg.inv(np.linalg.cholesky(Gd.T @ Gd)).T
            Q0 = np.hstack([W, Gd])
        its, prs, rrs, errs, conds, grs, fails = [], [], [], [], [], [], 0
        for b in range(nrep):
            G, Hs = gram(b)
            if b not in truth:
                truth[b] = np.linalg.eigvalsh(G)[::-1][:R]
            try:
                n, pr, rr, th, cond, gr = solve(G, Q0, degs, k=R, beta=beta, strict=strict, bfix=bfix,
                                            tol=float(os.environ.get("TOL", "1e-12")), Hs=Hs,
                                            nrng=np.random.default_rng(77_000 + b))
            except np.linalg.LinAlgError:   # a Gram matrix that is not positive definite
                fails += 1
                continue
            its.append(n)
            prs.append(pr)
            rrs.append(rr)
            conds.append(cond)
            grs.append(gr)
            errs.append(np.max(np.abs(th - truth[b]) / truth[b]))
        print(f"{sc:14s} loop steps mean {np.mean(its):.3f} max {max(its)}  hist "
              f"{dict(zip(*[v.tolist() for v in np.unique(its, return_counts=True)]))}  RR steps mean {np.mean(rrs):.3f}"
              f"  products mean {np.mean(prs):.3f}  max eigenvalue rel err {max(errs):.2e}"
              f"  cond after first filter median {np.median(conds):.2e} max {max(conds):.2e}  Cholesky failures {fails}"
              + (f"  theta_p / theta_k at step 0 max {max(grs):.4f}" if max(grs) > 0 else ""),
              flush=True)


if __name__ == "__main__":
    main()
