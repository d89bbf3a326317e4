"""The two top-k eigensolvers on matrices whose spectrum was chosen, solver by
solver, through the debug entries of csrc/dfm_eig_debug.hip: eig_run
(dfm_eig.hip) on each of its five code paths and launch_dense_eig_batched
(dfm_spec.hip).  Matrices, references and checkers: tests/eig_reference.py
(exact cases: Hadamard-block matrices whose entries, eigenvalues and
eigenspaces are exact, so a tie is a tie; rounded cases against LAPACK's
dsyevr).  tests/test_eig_checks.py shows on the CPU that the checkers reject
wrong outputs.

Paths (test_spectra[path-m], every m of the path):
  fused4    eig_fused_kernel<4, 6, true>     m = 1, 2, 3, 5, 16, 17, 63, 64      fused = 1
  fused9    eig_fused_kernel<9, 12, true>    m = 65, 143, 144                    fused = 1
  fused16   eig_fused_kernel<16, 22, false>  m = 145, 250, 256                   fused = 1
  chain16   gq / small / apply / cheb, P=16  the m above with fused = 0, and 257, 300 (nrb = 5)
  chain32   the same chain at P = 32         every m from 63 on, k = 20 (block 28), 24 (block 32)
  dense     launch_dense_eig_batched         every m from 2 on, k = 1, 4, 8, 15, 16, 33, 40, m (test_dense_spectra)

Spectrum families (eig_reference.family_vals / rounded_lams; 0-based j below):
  a   geometric 2^-j over a flat tail; a+ / a- the same times 2^+100 / 2^-100
  b   lambda_1 = lambda_2 and, from k = 8, a triple inside the wanted set; b+ / b- scaled
  c   lambda_{k-1} = lambda_k = lambda_{k+1}: an exact tie across the k | k+1 boundary
  d   a tie of p - k + 3 values from lambda_{k-1} down: more than the block's guard columns
  e   exact rank k - 2 (k <= 2: G = 0);  z: G = 0
  f   exact rank between k and p
  g   rounded, lambda_k = lambda_{k-1} (1 - 1e-6)
  h   rounded, p + 6 values within 1e-6 relative, maxit = 12: the only case that may end with status 1

Which case reaches which branch:

  branch                                               case
  ---------------------------------------------------  ------------------------------------------------------
  column_verdict: res <= tol gap with gap = 0          b, c, d under tol = 1e-14 (floor or stagnation accepts)
  column_verdict: subspace gap |theta_j - theta_k|     test_rules[*-subspace]; c: that gap is 0 for j = k - 1
  column_verdict: no right neighbour (j + 1 == p)      k = p = m (m <= 16 in fused4 and chain16)
  energy_converged: 1e-6 trace floor, bnd = 0 / 0      test_rules[*-values] on e (trace - sum theta = 0), b, c
  wave_chol_inv dead pivots (Z'Z), hash_unit re-seed   e, f, z (rank < p); z also th0 = 0 and b <= 0 (cheb: power steps)
  wave_chol_inv dead pivots (Q'Q)                      e (Q'Q singular: every filtered column in range(G)); a, a+, a- must have none
  fused kernels' edges: mpad, ng, row < m guards       m = 1, 2, 3, 5, 17, 63, 65, 143, 145, 250 (not multiples of 4 / 16)
  fused OVL (wave 3: Q'Q beside Y = G Q) on / off      fused4, fused9 on; fused16 off
  chain: nrb = 1, 2, 3, 4, 5; check_converged G = 1..8 chain16 at m = 64, 65, 144, 250, 300; chain32 likewise
  chain: the poll's early exit and the check-only pass every status-0 case; h at maxit = 12 (not a poll step)
  degree-4 schedule (warm_strict)                      nb = 1 strict, test_rules[*-warm1 / warm6]; degree 2: values, batches
  not converged: status 1, iters = maxit               h (test_spectra at maxit = 12, test_batch_invariance at 400)
  eig_final_body: Uk null, sign rule                   test_rules[*-values]; every case with vectors (check_signs)
  batch invariance (eig_init_kernel's comment)         test_batch_invariance (values, warm strict, cold strict nb 6 vs 2)
  eig_run argument check (the entry has none of its own)  test_rejections
  dense: bisection on ties, dstein's shifted shifts    dense b, c, d, e, z
  dense: inverse iteration inside a cluster            dense h (p + 6 values within 1e-6), g, d
  dense: BCGS2 across a 32-column block, CholQR2       dense k = 33, 40
  dense: k = m, m = 2 (no reflector)                   dense m = 2, 3, 5, 16
  dense argument check                                 test_rejections

What these cases found is in DESIGN.md section 9 (dead pivots of chol(Q'Q) judged against the largest diagonal
entry, null Ritz pairs passing the residual test, the filter's upper end on a tie, iters of a status-1 replicate,
the dense path on G = 0).  test_rules[*-warm6] also asserts that one matrix times 2^0 .. 2^5 gives the same Uk and
step count six times (powers of two commute with every rounding), which the largest-entry pivot test broke;
test_scaling_by_2_100_keeps_the_bits asserts the same of a and b against a+, a-, b+, b-.

The strict rule's cold start takes degree-4 filters only at nb = 1, so a
strict cold solve is compared between a batch of 6 and a batch of 2, not with
its solo run.  dfm_spec.hip claims no batch invariance for the dense path:
its batch is checked to the same bars as its solo runs.  eig_block_p clamps
the block to m, so p > m cannot be reached through the entry; k > m gives p <
k and a block of 33, p > 32.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import eig_reference as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
INVALID = 1001   # 1000 + hipErrorInvalidValue
GUARD = 64
UNSET = -77      # the int outputs' fill
TOL = 1e-14      # ctx_eig_args: min(ctx->tol, 1e-14)
VALUE_TOL = -1e-12   # dfm_ctx: tol_values = 1e-12, passed as -tol_values
MAXIT = 400      # dfm_ctx: maxit
H_MAXIT = 12

FUSED4, FUSED9, FUSED16 = [1, 2, 3, 5, 16, 17, 63, 64], [65, 143, 144], [145, 250, 256]
PATHS = {"fused4": (1, FUSED4), "fused9": (1, FUSED9), "fused16": (1, FUSED16),
         "chain16": (0, FUSED4 + FUSED9 + FUSED16 + [257, 300]), "chain32": (-1, [63, 64, 65, 143, 144, 145, 250, 256, 257, 300])}
DENSE_MS = [2, 3, 5, 16, 17, 63, 64, 65, 143, 144, 145, 250, 256, 257, 300]
ALL = ["a", "b", "c", "d", "e", "f", "z", "g", "h", "a+", "a-", "b+", "b-"]
FEW = ["a", "b", "c"]


def plan(path, m):
    """[(k, families)] of one path at one m."""
    if path == "chain32":
        return [(20, ALL), (24, ALL)]
    if path == "dense":
        ks = [k for k in (1, 4, 8, 15, 16, 33, 40) if k <= m] + ([m] if m <= 16 and m not in (1, 4, 8, 15, 16) else [])
        return [(k, ALL if k in (8, 33) or k == m else FEW) for k in ks]
    ks = [k for k in (1, 4, 8, 15, 16) if k <= m] + ([m] if m <= 16 and m not in (1, 4, 8, 15, 16) else [])
    return [(k, ALL if k in (4, 16) or k == m else FEW) for k in ks]


def test_plan_runs_every_family_on_every_path():
    """No GPU: every family exists (eig_reference.make_case is not None) somewhere on every path."""
    for path, ms in list((p, v[1]) for p, v in PATHS.items()) + [("dense", DENSE_MS)]:
        ran = set()
        for m in ms:
            for k, fams in plan(path, m):
                ran |= {f for f in fams if R.make_case(f, m, k, R.block_p(m, k)) is not None}
        assert ran == set(ALL), (path, set(ALL) - ran)


# ------------------------------------------------------------------ the entries
@functools.lru_cache(maxsize=None)
def _ctx():
    import dfm_pkg
    ctx = dfm_pkg.load().Context(0)
    L, P, I, I64, D = ctx.lib, C.c_void_p, C.c_int, C.c_int64, C.c_double
    for name, args in [("dfm_debug_eig", [P, P, I64, I64, I, I, I, I, D, I, I, P, I, I, P, P, P, P, P]),
                       ("dfm_debug_dense_eig", [P, P, I64, I64, I, I, I, P, P, P, P])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = C.c_int, args
    return ctx


def _dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(n):
    import torch
    return torch.full((int(n) + GUARD,), NAN, dtype=torch.float64, device="cuda")


def _unset(n):
    import torch
    return torch.full((int(n) + GUARD,), UNSET, dtype=torch.int32, device="cuda")


def _run(fn, *args):
    import torch
    torch.cuda.synchronize()
    ctx = _ctx()
    rc = getattr(ctx.lib, fn)(ctx.h, *args)
    if rc >= 1000 and rc != INVALID:   # a runtime error (a fault, not a wrong value): launch nothing more on this device
        pytest.exit(f"{fn}: HIP error {rc - 1000}", returncode=3)
    return rc


def _ints(buf, n, case, what):
    h = buf.cpu().numpy()
    assert (h[n:] == UNSET).all(), f"{case.name}: {what} written past its extent of {n}"
    return h[:n]


def solve(cases, k, *, dense=False, block=0, tol=TOL, maxit=MAXIT, subspace=0, warm=None, fused=-1, vectors=True):
    """One call on the nb matrices of cases (all m x m) -> (rc, [dict(lam, U, trace, status, iters)] or None).
    Every output is NaN- (int: UNSET-) filled with a guard behind it; extents are checked here."""
    nb, m = len(cases), cases[0].m
    G = np.stack([c.G for c in cases])
    dG = _dev(G)
    lam, U, tr = _nan(nb * k), (_nan(nb * m * k) if vectors else None), _nan(nb)
    st, it = _unset(nb), _unset(nb)
    stride = m * m if nb > 1 else 0
    if dense:
        rc = _run("dfm_debug_dense_eig", _ptr(dG), m, stride, m, nb, k, _ptr(lam), _ptr(U), _ptr(tr), _ptr(st))
    else:
        dW = _dev(warm)
        rc = _run("dfm_debug_eig", _ptr(dG), m, stride, m, nb, k, block, tol, maxit, subspace, _ptr(dW),
                  0 if warm is None else warm.shape[1], fused, _ptr(lam), _ptr(U), _ptr(tr), _ptr(st), _ptr(it))
    c0 = cases[0]
    if rc not in (0, 1):
        for b in (lam, U, tr):
            assert b is None or np.isnan(b.cpu().numpy()).all(), f"{c0.name}: rc {rc} and an output was written"
        assert (st.cpu().numpy() == UNSET).all() and (it.cpu().numpy() == UNSET).all()
        return rc, None
    hl, ht = lam.cpu().numpy(), tr.cpu().numpy()
    R.check_extent(hl, nb * k, c0, "lam")
    R.check_extent(ht, nb, c0, "trace")
    hs = _ints(st, nb, c0, "status")
    hi = _ints(it, 0 if dense else nb, c0, "iters")
    hu = None
    if vectors:
        hu = U.cpu().numpy()
        R.check_extent(hu, nb * m * k, c0, "Uk")
        hu = hu[:nb * m * k].reshape(nb, m, k)
    assert rc == int((hs != 0).any()), (c0.name, rc, hs)
    return rc, [dict(lam=hl[j * k:(j + 1) * k], U=None if hu is None else hu[j], trace=ht[j], status=int(hs[j]),
                     iters=None if dense else int(hi[j])) for j in range(nb)]


def judge(case, k, p, o, tol, subspace, maxit, may_fail=False):
    """All checks of one replicate -> its shares.  Only an (h) case may end with status 1."""
    if not may_fail and o["status"] != 0:
        raise AssertionError(f"{case.name}: status {o['status']} after {o['iters']} steps (maxit {maxit})")
    return R.verify(case, k, p, o["lam"], o["U"], o["trace"], o["status"], tol, subspace, o["iters"], maxit)


class Worst(dict):
    def take(self, shares):
        for n, v in shares.items():
            self[n] = max(self.get(n, 0.0), v)

    def __str__(self):
        return "  ".join(f"{n} {v:.3g}" for n, v in sorted(self.items()))


# ------------------------------------------------- every family on every path
def _spectra(path, m, dense=False, fused=-1):
    worst, its, n = Worst(), 0, 0
    for k, fams in plan(path, m):
        p = R.block_p(m, k)
        for fam in fams:
            case = R.make_case(fam, m, k, p)
            if case is None:
                continue
            maxit = H_MAXIT if fam == "h" else MAXIT
            if dense:
                rc, out = solve([case], k, dense=True)
                sh = judge(case, k, m, out[0], 0.0, 0, None)   # a direct solver: the strict bars with tol gap = 0
            else:
                rc, out = solve([case], k, tol=TOL, maxit=maxit, fused=fused)
                sh = judge(case, k, p, out[0], TOL, 0, maxit, may_fail=fam == "h")
                its = max(its, out[0]["iters"])
            print(f"ORTH {path} {fam} {m} {k} {p} {sh['orth']:.3e} status={out[0]['status']} iters={out[0]['iters']}")
            worst.take(sh)
            n += 1
    print(f"SHARES {path} m={m}: {n} cases, most steps {its}; {worst}")


@pytest.mark.parametrize("path,m", [(p, m) for p, (_, ms) in PATHS.items() for m in ms])
def test_spectra(path, m):
    """Cold start, tol = 1e-14 strict with the neighbour gap, nb = 1, maxit = 400 (h: 12): status 0 for every
    family but h, and every check of eig_reference.verify."""
    _spectra(path, m, fused=PATHS[path][0])


@pytest.mark.parametrize("m", DENSE_MS)
def test_dense_spectra(m):
    _spectra("dense", m, dense=True)


# ------------------------------------------------------------ rules and starts
RULE_SHAPES = {"fused4": [(17, 4), (64, 16), (16, 16)], "fused9": [(65, 8), (144, 16)], "fused16": [(145, 15), (256, 16)],
               "chain16": [(64, 16), (257, 8), (300, 16), (5, 5)], "chain32": [(65, 20), (300, 24)]}


@pytest.mark.parametrize("mode", ["neighbours", "subspace", "values", "warm1", "warm6"])
@pytest.mark.parametrize("path", list(PATHS))
def test_rules(path, mode):
    """Families a, b, c, e under the strict rule with both gaps, the eigenvalue rule (tol = -1e-12, Uk null) and
    warm starts (kw = k exact vectors + 1e-3 normals: the degree-4 schedule) at nb = 1 and at nb = 6 (the matrix
    times 2^0 .. 2^5: one set of start vectors serves all six)."""
    worst, its = Worst(), 0
    for m, k in RULE_SHAPES[path]:
        p = R.block_p(m, k)
        for fam in ("a", "b", "c", "e"):
            case = R.make_case(fam, m, k, p)
            if case is None:
                continue
            cases, kw = [case], dict(tol=TOL, fused=PATHS[path][0])
            if mode == "subspace":
                kw["subspace"] = 1
            elif mode == "values":
                kw.update(tol=VALUE_TOL, vectors=False)
            elif mode.startswith("warm"):
                kw["warm"] = R.warm_start(case, k)
                if mode == "warm6":
                    cases = [R.scaled(case, e) for e in range(6)]
            rc, out = solve(cases, k, **kw)
            for c, o in zip(cases, out):
                worst.take(judge(c, k, p, o, kw["tol"], kw.get("subspace", 0), MAXIT))
                its = max(its, o["iters"])
            if mode == "warm6":   # scaling by 2 commutes with every rounding: the six replicates differ by the exponent alone
                for e, o in enumerate(out):
                    assert np.array_equal(o["U"], out[0]["U"]) and np.array_equal(o["lam"], out[0]["lam"] * 2.0 ** e)
                    assert o["iters"] == out[0]["iters"]
    print(f"SHARES {path} {mode}: most steps {its}; {worst}")


@pytest.mark.parametrize("path", list(PATHS))
def test_scaling_by_2_100_keeps_the_bits(path):
    """Families a and b against a+ / a- and b+ / b- (the same integers times 2^100 and 2^-100), cold start, strict
    rule: Uk, status and iters bit-equal, lam equal after the exact rescaling.  Every threshold of the solver is
    relative and no intermediate leaves the normal range, so a power of two commutes with every rounding."""
    for m, k in RULE_SHAPES[path]:
        p = R.block_p(m, k)
        for fam in ("a", "b"):
            if R.make_case(fam, m, k, p) is None:
                continue
            outs = {}
            for sfx in ("", "+", "-"):
                rc, out = solve([R.make_case(fam + sfx, m, k, p)], k, fused=PATHS[path][0])
                assert rc == 0
                outs[sfx] = out[0]
            for sfx, e in (("+", 100), ("-", -100)):
                what = f"{fam}{sfx} m={m} k={k} on {path}"
                assert np.array_equal(outs[sfx]["U"], outs[""]["U"]), what
                assert np.array_equal(outs[sfx]["lam"], outs[""]["lam"] * 2.0 ** e), what
                assert outs[sfx]["iters"] == outs[""]["iters"], what


# --------------------------------------------------------------------- batches
BATCH = ["a", "b", "c", "e", "h", "g"]
BATCH_SHAPES = {"fused4": (64, 8), "fused9": (143, 15), "fused16": (250, 16), "chain16": (300, 16), "chain32": (257, 20)}


def _same(a, b, what):
    for f in ("lam", "U", "status", "iters"):
        assert np.array_equal(a[f], b[f]), f"{what}: {f} differs from the other call's"


@pytest.mark.parametrize("path", list(PATHS))
def test_batch_invariance(path):
    """Six spectra in one call, h among them (maxit = 400: h alone may end with status 1, iters = 400, beside
    replicates that retired long before).  Eigenvalue rule and warm strict rule: every replicate's lam, Uk,
    status and iters are those of its solo call, bit for bit.  Cold strict rule (degree 4 only at nb = 1): those
    of a batch of 2."""
    m, k = BATCH_SHAPES[path]
    p, fused = R.block_p(m, k), PATHS[path][0]
    cases = [R.make_case(f, m, k, p) for f in BATCH]
    zero = R.make_case("z", m, k, p)
    warm = R.warm_start(cases[0], k)
    worst = Worst()
    for name, kw in [("values", dict(tol=VALUE_TOL)), ("warm", dict(tol=TOL, warm=warm)), ("cold", dict(tol=TOL))]:
        rc, out = solve(cases, k, fused=fused, **kw)
        for j, (c, o) in enumerate(zip(cases, out)):
            worst.take(judge(c, k, p, o, kw["tol"], 0, MAXIT, may_fail=BATCH[j] == "h"))
            _, alone = solve([c, zero] if name == "cold" else [c], k, fused=fused, **kw)
            _same(o, alone[0], f"{c.name} {name}")
        print(f"BATCH {path} {name}: status {[o['status'] for o in out]} iters {[o['iters'] for o in out]}")
    print(f"SHARES {path} batch: {worst}")


def test_dense_batch():
    """Six spectra in one dense call, k = 33 (BCGS2 across a block): each to the bars of its solo run."""
    m, k = 145, 33
    cases = [R.make_case(f, m, k, R.block_p(m, k)) for f in BATCH]
    rc, out = solve(cases, k, dense=True)
    worst = Worst()
    for c, o in zip(cases, out):
        worst.take(judge(c, k, m, o, 0.0, 0, None))
    print(f"SHARES dense batch: {worst}")


# ------------------------------------------------------------------ rejections
def test_rejections():
    """eig_run: p < k (k > m), p > 32 (a block of 33) -> -1; the dense launcher: m < 2, k > m -> 1001.  Nothing
    is written (solve checks every output is still NaN)."""
    c5, c40, c1 = R.make_case("a", 5, 4, 5), R.make_case("a", 40, 4, 16), R.make_case("a", 1, 1, 1)
    assert solve([c5], 6)[0] == -1
    assert solve([c40], 4, block=33)[0] == -1
    assert solve([c40], 4, block=32)[0] == 0
    assert solve([c1], 1, dense=True)[0] == INVALID
    assert solve([c5], 6, dense=True)[0] == INVALID
