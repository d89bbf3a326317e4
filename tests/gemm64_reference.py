"""Inputs, references and checkers for the fp64 MFMA GEMM and Gram kernels
(tests/test_gpu_gemm64.py runs the kernels, tests/test_gemm64_checks.py feeds
the same checkers wrong outputs on the CPU).  numpy only.

Two input families, each blind where the other sees:

* integers (entries in -7..7; for the fused panel X* = C + eta E[idx], C and
  E in -3..3 and eta in {-2, -1, 1, 2}): every product and partial sum is an
  exact integer below 2^53 for K <= 5000 in any summation order, so the fp64
  numpy product is the exact answer and the comparison is np.array_equal.
  A scaling (invT, alpha) is one IEEE multiplication of the exact sum, in the
  kernel and here.  This is what tells "written and right" from "not touched
  (still NaN)" entry by entry;
* reals (standard normal, rows scaled by U(0.2, 3), columns by U(0.1, 10)):
  small integers are exact in fp32 and bf16 too, so only these see a loss of
  precision.  Reference: the double-double product (oracle/dfm_xp.py DD);
  entrywise |got - ref| <= (K + 6) 2^-53 |scale| (|A| |B|), the bound of a
  length-K fma sum in any order plus the four-way fold, the one scaling and
  the fused operand's own rounding.
"""
import numpy as np

from dfm_xp import DD

U53 = 2.0 ** -53


# ----------------------------------------------------------------- the inputs
def int_mat(rng, shape, lim=7):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def real_mat(rng, m, n):
    return rng.standard_normal((m, n)) * rng.uniform(0.2, 3.0, size=(m, 1)) * rng.uniform(0.1, 10.0, size=(1, n))


def draws(rng, nrep, rows, src_rows, rs, integers):
    """idx (nrep x rs int32, values < src_rows, with repeats) and eta (nrep x rs, both signs); the columns past
    `rows` hold valid but unused values, as a break block's stride leaves them."""
    idx = rng.integers(0, src_rows, size=(nrep, rs)).astype(np.int32)
    idx[:, 1] = idx[:, 0]   # at least one repeat per replicate
    if integers:
        eta = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(nrep, rs))
    else:
        eta = rng.standard_normal((nrep, rs))
    eta[:, 0] = -np.abs(eta[:, 0])
    eta[:, 1] = np.abs(eta[:, 1])
    return idx, eta


def round_up(x, q):
    return (x + q - 1) // q * q


def padded(A, rows, ld, fill=0.0):
    """A in the top-left corner of a rows x ld array of `fill`."""
    P = np.full((rows, ld), fill)
    P[:A.shape[0], :A.shape[1]] = A
    return P


# ------------------------------------------------------- the library's splits
def gram_ksplit(m, K):
    """dfm_gram.hip gram_ksplit (the batched Gram's K-split request)."""
    nt = (m + 63) // 64
    if nt * (nt + 1) // 2 < 64 or K < 4096:
        return 1
    return max(1, min(16, K // 1536))


def gram_ksplit_single(m, K):
    """dfm_gram.hip gram_ksplit_single (one plain panel on gram_dma_kernel)."""
    nt = (m + 63) // 64
    tiles = nt * (nt + 1) // 2
    slots = (3 if m >= 1024 else 2) * 256
    smax = max(1, min(32, K // 256))
    for S in range(1, smax + 1):
        items = tiles * S
        rounds = (items + slots - 1) // slots
        if items >= 4 * slots and items * 10 >= rounds * slots * 9:
            return S
    if tiles * smax <= slots:
        return smax
    best, beff = 1, 0.0
    for S in range(1, smax + 1):
        items = tiles * S
        rounds = (items + slots - 1) // slots
        eff = items / (rounds * slots)
        if items >= slots and eff > beff + 1e-9:
            beff, best = eff, S
    return best


def splits(S0, K):
    """(number of partial images, 16-deep steps per image, steps of the last image) as launch_gram_a cuts K."""
    n = (K + 15) // 16
    ks = (n + S0 - 1) // S0
    S = (n + ks - 1) // ks
    return S, ks, n - (S - 1) * ks


# ------------------------------------------------------------- the references
def fused_panel(C, E, idx, eta, exact):
    """X* = C + eta E[idx] (rows), any of C / eta / idx None; exact: fp64 (integers), else a DD."""
    X = E if idx is None else E[idx]
    if exact:
        if eta is not None:
            X = eta[:, None] * X
        return X if C is None else C + X
    X = DD(X)
    if eta is not None:
        X = DD(eta[:, None]) * X
    return X if C is None else DD(C) + X


def dd_product(A, B):
    """(reference DD, |A| |B|) of A @ B; A, B fp64 arrays or DD."""
    A, B = DD.of(A), DD.of(B)
    return A @ B, np.abs(A.f64()) @ np.abs(B.f64())


# ---------------------------------------------------------------- the checkers
def check_exact(got, ref, written=None):
    """Integer family: got == ref to the bit where `written` (default: everywhere), NaN everywhere else."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if written is None:
        written = np.ones(ref.shape, dtype=bool)
    written = np.broadcast_to(written, ref.shape)
    bad = written & ~(got == ref)
    assert not bad.any(), f"{bad.sum()} wrong entries, first at {tuple(np.argwhere(bad)[0])}"
    stray = ~written & ~np.isnan(got)
    assert not stray.any(), f"{stray.sum()} entries written where none may be, first at {tuple(np.argwhere(stray)[0])}"


def check_exact_or_untouched(got, ref):
    """Each entry either the exact value or still NaN (a column the kernel may skip)."""
    bad = ~((got == ref) | np.isnan(got))
    assert not bad.any(), f"{bad.sum()} entries neither exact nor NaN, first at {tuple(np.argwhere(bad)[0])}"


def check_bound(got, ref, absprod, K, scale=1.0):
    """Real family: |got - ref scale| <= (K + 6) 2^-53 |scale| absprod entrywise; returns the worst ratio.
    ref: DD of the unscaled product."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{(~np.isfinite(got)).sum()} non-finite entries"
    r = ref * scale if scale != 1.0 else ref
    err = np.abs((got - r.hi) - r.lo)
    bound = (K + 6) * U53 * abs(scale) * absprod
    ratio = float((err / bound).max())
    assert np.all(err <= bound), f"worst |err| / bound = {ratio:.3g}"
    return ratio


def check_pad_is_nan(full, ncol):
    """Columns ncol.. of the caller's NaN-filled buffer are untouched."""
    assert np.all(np.isnan(full[..., ncol:])), "padding columns were written"


def rep_cols(reps, pz):
    """Column numbers of the replicates' pz-column groups."""
    reps = np.asarray(reps, dtype=np.int64).reshape(-1)
    return (reps[:, None] * pz + np.arange(pz)[None, :]).reshape(-1)


def check_compacted(got, exact, clist, ccount, nb, pz, done=None):
    """A launch_gemm_zrm call with a clist: when ccount 8 < nb the listed replicates' columns hold the exact product
    and every other column (the replicates named past ccount included) is still NaN; otherwise every column is
    written.  done (nb flags): a retired replicate's columns may have been skipped (exact or NaN)."""
    compact = ccount * 8 < nb
    listed = np.zeros(nb, dtype=bool)
    listed[np.asarray(clist[:ccount])] = True
    if not compact:
        listed[:] = True
    retired = np.zeros(nb, dtype=bool) if done is None else np.asarray(done, dtype=bool)
    must = rep_cols(np.flatnonzero(listed & ~retired), pz)
    may = rep_cols(np.flatnonzero(listed & retired), pz)
    never = rep_cols(np.flatnonzero(~listed), pz)
    check_exact(got[:, must], exact[:, must])
    check_exact_or_untouched(got[:, may], exact[:, may])
    assert np.all(np.isnan(got[:, never])), "columns of replicates outside the list were written"


def check_gram(Gfull, m):
    """G (…, m, ldg) as the Gram kernels leave it: the m x m block symmetric to the bit, columns m.. untouched."""
    G = Gfull[..., :m]
    assert np.array_equal(G, np.swapaxes(G, -1, -2)), "G is not symmetric bit for bit"
    check_pad_is_nan(Gfull, m)
