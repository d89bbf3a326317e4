"""The fp64 MFMA GEMM and Gram kernels (dfm_gemm.hip, dfm_gram.hip) against
exact products, kernel by kernel, through the debug entries of
csrc/dfm_gemm_debug.hip.  Inputs, references and checkers:
tests/gemm64_reference.py (integers: bit equality with the exact product and
NaN wherever nothing may be written; reals: the derived (K + 6) 2^-53 bound
against the double-double product).  tests/test_gemm64_checks.py shows on the
CPU that the checkers reject wrong outputs.

Which case reaches which branch:

  kernel / branch                                   test (case)
  ------------------------------------------------  ---------------------------------------------------------
  ring_wait<3>: 1, 2, 3, 4, 5, 13 k-stages          test_gemm_integers, test_zrm_integers (K = T = 5..200),
    (prologue of 2, ahead = 1 / 0)                    test_gram_dma_integers (m >= 1024)
  ring_wait<4>: the same (prologue of 3,            test_loadings_integers (K = T + r), test_gram_dma_integers
    ahead = 2 / 1 / 0)                                (m < 1024)
  gemmh_kernel: row / column tile edges, clamped    test_gemm_integers (M 1..130, Nc 2..578, NaN in B's pad)
    reads, second XCD group, cb >= ncb return         (Nc = 578: 10 column blocks)
  launch_gemm argument check                        test_gemm_rejects_bad_arguments
  gemmh_zrm_kernel: tiles straddling replicates,    test_zrm_integers (pz 2..32, nb 1..64; 12 x 64 = 768 columns)
    > 8 column blocks
  clist compaction on / off, slots past ccount      test_zrm_compaction_integers (ccount 1, 7, 8),
                                                      test_zrm_compaction_keeps_the_bits
  col_done: a tile all done, a tile mixed           test_zrm_col_done (plain and compacted)
  batch invariance, bits of gemmh_kernel            test_zrm_batch_invariance, test_zrm_bits_of_row_major_kernel
  gemm_loadings_kernel: rp 2..16, odd r, nrb8       test_loadings_integers (N = 513: 9 row blocks), NaN guard
  gram_dma_kernel<4,2> / <3,3>                      test_gram_dma_integers (m 64..130 / 1024, 1030; 1023 is <4,2>)
  gram_ksplit_single = 1, 2, 19; short last split;  test_gram_dma_integers, test_gram_plain_scaled
    gram_splitk_sum_kernel with alpha
  launch_gram_plain_scaled argument check           test_gram_plain_scaled_rejects
  gram_kernel, ten instantiations                   test_gram_kernel_integers / _reals (orient x five sources)
  COLS gather staged in LDS (kpre) / per stage      test_gram_cols_gather_depth (K = 600 / 2100)
  batched split-K (gram_ksplit 2, 3), both orients  test_gram_batched_split_k
  batch invariance of a replicate's Gram            test_gram_replicate_alone_has_the_same_bits
  one summation order in both Gram kernels          test_plain_and_gathering_gram_kernels_give_the_same_bits
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gemm64_reference as R

pytestmark = pytest.mark.gpu
NAN = float("nan")
INVALID = 1001   # 1000 + hipErrorInvalidValue
KS = [5, 16, 17, 33, 49, 65, 200]   # 1, 1, 2, 3, 4, 5 and 13 sixteen-deep k-stages


# ------------------------------------------------------------------ the entries
@functools.lru_cache(maxsize=None)
def _ctx():
    import dfm_pkg
    ctx = dfm_pkg.load().Context(0)
    L, P, I, I64, D = ctx.lib, C.c_void_p, C.c_int, C.c_int64, C.c_double
    for name, args in [("dfm_debug_gemm", [P, P, I64, P, I64, P, I64, I, I, I]),
                       ("dfm_debug_gemm_zrm", [P, P, I64, I, P, I, I, P, I64, P, P, P]),
                       ("dfm_debug_gemm_loadings", [P, P, P, I, I, I, I, D, P]),
                       ("dfm_debug_gram", [P, I, I, P, P, I64, P, P, I64, I, I, I, I, P, I64, I64, D])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = C.c_int, args
    return ctx


def _dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()   # (a writable copy)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(n):
    import torch
    return torch.full((int(n),), NAN, dtype=torch.float64, device="cuda")


def _run(fn, *args):
    import torch
    torch.cuda.synchronize()
    ctx = _ctx()
    rc = getattr(ctx.lib, fn)(ctx.h, *args)
    if rc >= 1000 and rc != INVALID:   # a runtime error (a fault, not a wrong value): launch nothing more on this device
        pytest.exit(f"{fn}: HIP error {rc - 1000}", returncode=3)
    return rc


def gemm(Ap, Bp, M, Nc, K, ldc):
    """launch_gemm on the padded operands Ap (M x lda), Bp (round_up(K, 16) x ldb) -> (rc, C as M x ldc)."""
    dA, dB, out = _dev(Ap), _dev(Bp), _nan(M * ldc)
    rc = _run("dfm_debug_gemm", _ptr(dA), Ap.shape[1], _ptr(dB), Bp.shape[1], _ptr(out), ldc, M, Nc, K)
    return rc, out.cpu().numpy().reshape(M, ldc)


def gemm_zrm(Hp, Z, nb, pz, ldc, done=None, clist=None, ccount=None):
    """H Z with Z (T x nb pz, plain) packed by the entry -> C as T x ldc."""
    T = Hp.shape[0]
    dH, dZ, out = _dev(Hp), _dev(Z), _nan(T * ldc)
    dd, dl = _dev(done, np.int32), _dev(clist, np.int32)
    dc = None if ccount is None else _dev(np.array([ccount]), np.int32)
    rc = _run("dfm_debug_gemm_zrm", _ptr(dH), Hp.shape[1], T, _ptr(dZ), nb, pz, _ptr(out), ldc, _ptr(dd), _ptr(dl),
              _ptr(dc))
    assert rc == 0, rc
    return out.cpu().numpy().reshape(T, ldc)


GUARD = 64


def loadings(A, B, invT):
    """A (K x N), B (nrep x K x r) -> Lout (nrep x N x r) and the NaN guard behind it."""
    K, N = A.shape
    nrep, _, r = B.shape
    dA, dB, out = _dev(A), _dev(B), _nan(nrep * N * r + GUARD)
    rc = _run("dfm_debug_gemm_loadings", _ptr(dA), _ptr(dB), N, nrep, K, r, invT, _ptr(out))
    assert rc == 0, rc
    o = out.cpu().numpy()
    return o[:nrep * N * r].reshape(nrep, N, r), o[nrep * N * r:]


def gram(orient, Cp, Ep, idx, eta, nrep, m, K, mode=0, alpha=1.0, ldg=None, expect=0):
    """launch_gram (mode 0) or launch_gram_plain_scaled (mode 1) on padded panels -> G as nrep x m x ldg; the
    strideG - m ldg doubles between two images must stay NaN."""
    ldg = m + 3 if ldg is None else ldg
    stride = m * ldg + 5
    dC, dE, dI, dH, out = _dev(Cp), _dev(Ep), _dev(idx, np.int32), _dev(eta), _nan(nrep * stride)
    rs = 0 if idx is None and eta is None else (idx if idx is not None else eta).shape[1]
    rc = _run("dfm_debug_gram", mode, orient, _ptr(dC), _ptr(dE), Ep.shape[1], _ptr(dI), _ptr(dH), rs, nrep, m, K,
              m if orient == 0 else K, _ptr(out), ldg, stride, alpha)
    assert rc == expect, rc
    o = out.cpu().numpy().reshape(nrep, stride)
    assert np.all(np.isnan(o[:, m * ldg:])), "the gap between two Gram images was written"
    return o[:, :m * ldg].reshape(nrep, m, ldg)


def _report(kernel, case, ratio):
    print(f"{kernel} {case}: worst |err| / bound = {ratio:.4f}")


# ---------------------------------------------------------------- gemmh_kernel
def _gemm_operands(M, Nc, K, integers):
    """A (M x K), B (K x Nc) and their padded images: lda = round_up(K, 16) + 2 with zero k-padding, ldb = Nc + 6
    with NaN in the columns past Nc (the kernel clamps its column reads to Nc - 2), zero rows K..round_up(K, 16)."""
    rng = np.random.default_rng([6500, M, Nc, K, int(integers)])
    A, B = (R.int_mat(rng, (M, K)), R.int_mat(rng, (K, Nc))) if integers else (R.real_mat(rng, M, K), R.real_mat(rng, K, Nc))
    Kp = R.round_up(K, 16)
    Bp = R.padded(B, Kp, Nc + 6)
    Bp[:, Nc:] = NAN
    return A, B, R.padded(A, M, Kp + 2), Bp


MN = [(1, 2), (63, 62), (64, 64), (65, 66), (130, 130), (1, 578), (65, 578), (130, 62), (64, 2)]


@pytest.mark.parametrize("K", KS)
def test_gemm_integers(K):
    """Every (M, Nc) of MN — M = 1 and 63 .. 65 and 130 (row tile edges, more than one row block), Nc = 2 (a
    single pair), 62 .. 66 (column tile edges), 130, 578 (10 column blocks: the XCD map's second group and the
    cb >= ncb return) — at each k-stage count: bit-equal to the exact product, finite although B's padding is
    NaN, and C's columns Nc .. ldc - 1 untouched."""
    for M, Nc in MN:
        A, B, Ap, Bp = _gemm_operands(M, Nc, K, True)
        rc, Cf = gemm(Ap, Bp, M, Nc, K, Nc + 3)
        assert rc == 0, (rc, M, Nc)
        R.check_exact(Cf[:, :Nc], A @ B)
        R.check_pad_is_nan(Cf, Nc)


@pytest.mark.parametrize("M,Nc,K", [(130, 130, 200), (65, 66, 17), (1, 2, 5), (63, 62, 33), (64, 64, 49),
                                    (65, 578, 65), (130, 66, 16)])
def test_gemm_reals(M, Nc, K):
    A, B, Ap, Bp = _gemm_operands(M, Nc, K, False)
    rc, Cf = gemm(Ap, Bp, M, Nc, K, Nc + 3)
    assert rc == 0, rc
    ref, ap = R.dd_product(A, B)
    _report("gemmh_kernel", (M, Nc, K), R.check_bound(Cf[:, :Nc], ref, ap, K))
    R.check_pad_is_nan(Cf, Nc)


def test_gemm_rejects_bad_arguments():
    """launch_gemm: odd Nc, lda < round_up(K, 16), odd ldb -> hipErrorInvalidValue, and nothing is written."""
    M, Nc, K = 65, 66, 17
    A, B, Ap, Bp = _gemm_operands(M, Nc, K, True)
    for ap, bp, nc in [(Ap, Bp, Nc - 1), (Ap[:, :30], Bp, Nc), (Ap, Bp[:, :Nc + 5], Nc)]:
        rc, Cf = gemm(np.ascontiguousarray(ap), np.ascontiguousarray(bp), M, nc, K, Nc + 3)
        assert rc == INVALID
        assert np.all(np.isnan(Cf))


# ------------------------------------------------------------ gemmh_zrm_kernel
NB_MAX = 64


@functools.lru_cache(maxsize=None)
def _zrm_operands(T, pz, integers):
    """H (T x T, not symmetric: a transposed read would show) with ldH = round_up(T, 16) and Z (T x 64 pz)."""
    rng = np.random.default_rng([6600, T, pz, int(integers)])
    H, Z = (R.int_mat(rng, (T, T)), R.int_mat(rng, (T, NB_MAX * pz))) if integers else \
        (R.real_mat(rng, T, T), R.real_mat(rng, T, NB_MAX * pz))
    Hp = R.padded(H, T, R.round_up(T, 16))
    for a in (H, Z, Hp):
        a.setflags(write=False)
    return H, Z, Hp


# nb pz = 2 and 32 (less than a tile), 56, 84 and 88 (a tile and a few columns), 126, 198, 352 (tiles straddling
# replicates), 128 (whole tiles), 768 (12 column blocks)
PZNB = [(2, 1), (32, 1), (8, 7), (12, 7), (8, 11), (18, 7), (18, 11), (32, 11), (2, 64), (12, 64)]


@pytest.mark.parametrize("T", [5, 15, 16, 17, 33, 49, 65, 120, 121, 200])
def test_zrm_integers(T):
    """M = K = T: 15 / 16 / 17 the chunk and stage edge, 33, 49, 65 three to five stages, 120 / 121 / 200 more than
    one row block with and without a k tail; every (pz, nb) of PZNB."""
    for pz, nb in PZNB:
        H, Z, Hp = _zrm_operands(T, pz, True)
        Zc = Z[:, :nb * pz]
        Cf = gemm_zrm(Hp, Zc, nb, pz, nb * pz + 2)
        R.check_exact(Cf[:, :nb * pz], H @ Zc)
        R.check_pad_is_nan(Cf, nb * pz)


@functools.lru_cache(maxsize=None)
def _zrm_real(T, pz, nb):
    H, Z, Hp = _zrm_operands(T, pz, False)
    Cf = gemm_zrm(Hp, Z[:, :nb * pz], nb, pz, nb * pz)
    Cf.setflags(write=False)
    return Cf


@pytest.mark.parametrize("T,pz,nb", [(121, 12, 11), (200, 18, 7), (17, 2, 1), (65, 8, 7), (120, 32, 11), (121, 12, 64)])
def test_zrm_reals(T, pz, nb):
    H, Z, _ = _zrm_operands(T, pz, False)
    ref, ap = R.dd_product(H, Z[:, :nb * pz])
    _report("gemmh_zrm_kernel", (T, pz, nb), R.check_bound(_zrm_real(T, pz, nb), ref, ap, T))


CT, CPZ = 121, 12   # the compaction cases: nb = 64, pz = 12


def _clist(ccount):
    """A permutation of 0 .. 63: the first ccount entries are the list, the rest valid replicates outside it."""
    return np.random.default_rng(6700 + ccount).permutation(NB_MAX).astype(np.int32)


@pytest.mark.parametrize("ccount", [1, 7, 8])
def test_zrm_compaction_integers(ccount):
    """ccount = 1: the smallest list; 7 (7 x 8 < 64): 84 compact columns, a tile and 20; 8 (8 x 8 >= 64): the
    list is ignored and every column written.  Listed replicates' columns are exact, all others still NaN."""
    H, Z, Hp = _zrm_operands(CT, CPZ, True)
    cl = _clist(ccount)
    Cf = gemm_zrm(Hp, Z, NB_MAX, CPZ, NB_MAX * CPZ, clist=cl, ccount=ccount)
    R.check_compacted(Cf, H @ Z, cl, ccount, NB_MAX, CPZ)


@pytest.mark.parametrize("ccount", [1, 7])
def test_zrm_compaction_keeps_the_bits(ccount):
    """Real inputs: the columns a compacted launch writes are those of the full launch, bit for bit."""
    H, Z, Hp = _zrm_operands(CT, CPZ, False)
    full = _zrm_real(CT, CPZ, NB_MAX)
    cl = _clist(ccount)
    Cf = gemm_zrm(Hp, Z, NB_MAX, CPZ, NB_MAX * CPZ, clist=cl, ccount=ccount)
    cols = R.rep_cols(cl[:ccount], CPZ)
    assert np.array_equal(Cf[:, cols], full[:, cols])
    rest = np.setdiff1d(np.arange(NB_MAX * CPZ), cols)
    assert np.all(np.isnan(Cf[:, rest]))


@pytest.mark.parametrize("compact", [False, True])
def test_zrm_col_done(compact):
    """pz = 12: tile 0 covers replicates (list slots) 0 .. 5, tile 1 slots 5 .. 10.  Slots 0 .. 5 and 8 done: tile 0
    is all done, tile 1 mixed.  Compacted, the list has 7 slots (tile 1 = slots 5, 6: one done, one not).
    Columns of replicates that are not done are exact, those of done ones exact or untouched."""
    H, Z, Hp = _zrm_operands(CT, CPZ, True)
    exact = H @ Z
    done = np.zeros(NB_MAX, dtype=np.int32)
    if compact:
        cl = _clist(7)
        done[cl[:6]] = 1
        done[cl[40]] = 1   # a replicate outside the list
        Cf = gemm_zrm(Hp, Z, NB_MAX, CPZ, NB_MAX * CPZ, done=done, clist=cl, ccount=7)
        R.check_compacted(Cf, exact, cl, 7, NB_MAX, CPZ, done)
    else:
        done[[0, 1, 2, 3, 4, 5, 8]] = 1
        Cf = gemm_zrm(Hp, Z, NB_MAX, CPZ, NB_MAX * CPZ, done=done)
        R.check_compacted(Cf, exact, np.arange(NB_MAX), NB_MAX, NB_MAX, CPZ, done)
    skipped = int(np.isnan(Cf).all(axis=0).sum())
    print(f"compact={compact}: {skipped} columns left untouched")


def test_zrm_batch_invariance():
    """Replicates 0, 10 and 21 (columns straddling a tile edge at pz = 12), and 63, run alone: the bits of their
    columns in the 64-replicate call."""
    H, Z, Hp = _zrm_operands(CT, CPZ, False)
    full = _zrm_real(CT, CPZ, NB_MAX)
    for j in (0, 10, 21, 63):
        alone = gemm_zrm(Hp, Z[:, j * CPZ:(j + 1) * CPZ], 1, CPZ, CPZ)
        assert np.array_equal(alone, full[:, j * CPZ:(j + 1) * CPZ]), j
    assert np.array_equal(_zrm_real(CT, CPZ, 11), full[:, :11 * CPZ])


def test_zrm_bits_of_row_major_kernel():
    """dfm_gemm.hip: "the fragments hold the same elements as with a row-major Z in gemmh_kernel, so HZ has the
    same bits" — T = 121, pz = 12, nb = 11, the same Z row-major through gemmh_kernel."""
    T, pz, nb = 121, 12, 11
    H, Z, Hp = _zrm_operands(T, pz, False)
    rc, Cf = gemm(Hp, R.padded(Z[:, :nb * pz], R.round_up(T, 16), nb * pz), T, nb * pz, T, nb * pz)
    assert rc == 0
    assert np.array_equal(Cf, _zrm_real(T, pz, nb))


# -------------------------------------------------------- gemm_loadings_kernel
def _loadings_operands(r, N, nrep, T, integers):
    rng = np.random.default_rng([6800, r, N, nrep, T, int(integers)])
    K = T + r
    if integers:
        return R.int_mat(rng, (K, N)), R.int_mat(rng, (nrep, K, r))
    return R.real_mat(rng, K, N), np.stack([R.real_mat(rng, K, r) for _ in range(nrep)])


# r = 1 .. 16: rp = 2, 2, 4, 6, 8, 14, 16 (6 and 14: tiles straddle replicates; odd r: the zero column);
# N = 1, 63 .. 65, 130, 513 (9 row blocks: the nrb8 map's second round); nrep 1 .. 40; K = T + r
LOADINGS = [(1, 1, 1, 5), (2, 63, 7, 16), (3, 64, 11, 17), (5, 65, 40, 33), (8, 130, 7, 49), (13, 513, 11, 65),
            (16, 130, 40, 200), (1, 513, 40, 17), (5, 513, 1, 5), (13, 63, 40, 49), (3, 65, 7, 200), (2, 1, 11, 33)]


@pytest.mark.parametrize("invT", [1.0, 1.0 / 121])
@pytest.mark.parametrize("r,N,nrep,T", LOADINGS)
def test_loadings_integers(r, N, nrep, T, invT):
    """Lout = (A' B_rep) invT: bit-equal to exact * invT (one multiplication, as in the kernel), exactly
    nrep N r values written (the NaN guard behind them intact)."""
    A, B = _loadings_operands(r, N, nrep, T, True)
    got, guard = loadings(A, B, invT)
    R.check_exact(got, np.einsum("kn,jkr->jnr", A, B) * invT)
    assert np.all(np.isnan(guard))


@pytest.mark.parametrize("r,N,nrep,T,invT", [(5, 65, 7, 33, 1.0 / 33), (13, 130, 11, 65, 1.0), (3, 64, 11, 200, 1.0 / 121),
                                             (16, 63, 7, 17, 1.0 / 17), (1, 130, 40, 49, 1.0 / 121)])
def test_loadings_reals(r, N, nrep, T, invT):
    A, B = _loadings_operands(r, N, nrep, T, False)
    got, guard = loadings(A, B, invT)
    worst = 0.0
    for j in range(nrep):
        ref, ap = R.dd_product(A.T, B[j])
        worst = max(worst, R.check_bound(got[j], ref, ap, T + r, invT))
    _report("gemm_loadings_kernel", (r, N, nrep, T), worst)
    assert np.all(np.isnan(guard))


# ------------------------------------------------------------- gram_dma_kernel
def _plain_panel(m, K, integers):
    rng = np.random.default_rng([6900, m, K, int(integers)])
    X = R.int_mat(rng, (m, K)) if integers else R.real_mat(rng, m, K)
    return X, R.padded(X, m, R.round_up(K, 16))


# (m, K, gram_ksplit_single): <4,2> at 1, 1, 2, 3, 4, 5, 13 stages; <3,3> (m >= 1024) at 1 .. 4 and 13 stages;
# m = 1023 the last <4,2>; K = 520: two splits of 17 and 16 steps; (70, 5003): 19 splits, the last of 7 steps
GRAM_DMA = [(64, 5, 1), (65, 16, 1), (130, 17, 1), (64, 33, 1), (65, 49, 1), (130, 65, 1), (130, 200, 1),
            (1023, 50, 1), (1024, 5, 1), (1024, 17, 1), (1030, 33, 1), (1024, 50, 1), (1030, 49, 1), (1024, 200, 1),
            (130, 520, 2), (1030, 520, 2), (70, 5003, 19)]


@pytest.mark.parametrize("m,K,S", GRAM_DMA)
def test_gram_dma_integers(m, K, S):
    assert R.gram_ksplit_single(m, K) == S
    X, Xp = _plain_panel(m, K, True)
    G = gram(0, None, Xp, None, None, 1, m, K)
    R.check_exact(G[0, :, :m], X @ X.T)
    R.check_gram(G, m)


@pytest.mark.parametrize("alpha", [0.25, 1.0 / 7])
@pytest.mark.parametrize("m,K,S", [(65, 49, 1), (130, 520, 2), (1024, 50, 1), (70, 5003, 19)])
def test_gram_plain_scaled(m, K, S, alpha):
    """alpha in gram_dma_kernel's epilogue (S = 1) or in gram_splitk_sum_kernel (S > 1): exact * alpha."""
    assert R.gram_ksplit_single(m, K) == S
    X, Xp = _plain_panel(m, K, True)
    G = gram(0, None, Xp, None, None, 1, m, K, mode=1, alpha=alpha)
    R.check_exact(G[0, :, :m], (X @ X.T) * alpha)
    R.check_gram(G, m)


def test_gram_plain_scaled_rejects():
    """m < 64 and ld % 16 != 0 -> hipErrorInvalidValue, nothing written."""
    X, Xp = _plain_panel(63, 64, True)
    assert np.all(np.isnan(gram(0, None, Xp, None, None, 1, 63, 64, mode=1, alpha=0.5, expect=INVALID)))
    X, Xp = _plain_panel(64, 64, True)
    assert np.all(np.isnan(gram(0, None, R.padded(X, 64, 72), None, None, 1, 64, 64, mode=1, alpha=0.5, expect=INVALID)))


@pytest.mark.parametrize("m,K,alpha", [(130, 200, 1.0), (65, 17, 1.0 / 7), (130, 520, 1.0), (70, 5003, 1.0 / 7)])
def test_gram_dma_reals(m, K, alpha):
    X, Xp = _plain_panel(m, K, False)
    G = gram(0, None, Xp, None, None, 1, m, K, mode=1, alpha=alpha)
    ref, ap = R.dd_product(X, X.T)
    _report("gram_dma_kernel", (m, K, alpha), R.check_bound(G[0, :, :m], ref, ap, K, alpha))
    R.check_gram(G, m)


# ----------------------------------------------------------------- gram_kernel
SOURCES = {"C+eta*E[idx]": (1, 1, 1), "C+E[idx]": (1, 0, 1), "E": (0, 0, 0), "eta*E[idx]": (0, 1, 1), "E[idx]": (0, 0, 1)}


def _gram_case(orient, source, m, K, nrep, integers):
    """Panels, draws and the per-replicate X* of one case.  ROWS: X* is m x K (G = X* X*'), COLS: K x m
    (G = X*' X*); ld = the column count rounded up to 16, rs = rows + 3."""
    hc, he, hx = SOURCES[source]
    rows, cols = (m, K) if orient == 0 else (K, m)
    rng = np.random.default_rng([7000, orient, hc, he, hx, m, K, nrep, int(integers)])
    mk = (lambda: R.int_mat(rng, (rows, cols), 3)) if integers else (lambda: R.real_mat(rng, rows, cols))
    E, Cm = mk(), (mk() if hc else None)
    idx, eta = R.draws(rng, nrep, rows, rows, rows + 3, integers)
    idx, eta = (idx if hx else None), (eta if he else None)
    ld = R.round_up(cols, 16)
    Xs = [R.fused_panel(Cm, E, None if idx is None else idx[j, :rows], None if eta is None else eta[j, :rows], integers)
          for j in range(nrep)]
    return (None if Cm is None else R.padded(Cm, rows, ld)), R.padded(E, rows, ld), idx, eta, Xs


def _gram_of(X, orient):
    return X @ X.T if orient == 0 else X.T @ X


# m = 5 (one partial tile), 63 .. 65 (the tile edge), 130 (six lower tiles); K = 5 .. 200 (1 .. 13 stages, a k tail
# in all but two); nrep 1 and 3.  (m >= 64 at nrep = 1 without a gather is gram_dma_kernel's: those run nrep = 3.)
GRAM_SHAPES = [(5, 5, 1), (63, 17, 3), (64, 33, 3), (65, 49, 3), (130, 200, 3), (130, 65, 1), (64, 16, 3), (5, 200, 1)]


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("orient", [0, 1])
def test_gram_kernel_integers(orient, source):
    for m, K, nrep in GRAM_SHAPES:
        if source == "E" and orient == 0 and nrep == 1 and m >= 64:
            nrep = 3
        Cp, Ep, idx, eta, Xs = _gram_case(orient, source, m, K, nrep, True)
        G = gram(orient, Cp, Ep, idx, eta, nrep, m, K)
        for j in range(nrep):
            R.check_exact(G[j, :, :m], _gram_of(Xs[j], orient))
        R.check_gram(G, m)


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("orient", [0, 1])
def test_gram_kernel_reals(orient, source):
    worst = 0.0
    for m, K, nrep in [(130, 200, 1 if source != "E" else 3), (65, 49, 3), (5, 17, 1)]:
        Cp, Ep, idx, eta, Xs = _gram_case(orient, source, m, K, nrep, False)
        G = gram(orient, Cp, Ep, idx, eta, nrep, m, K)
        for j in range(nrep):
            X = R.DD.of(Xs[j])
            ref, ap = R.dd_product(X, X.T) if orient == 0 else R.dd_product(X.T, X)
            worst = max(worst, R.check_bound(G[j, :, :m], ref, ap, K))
        R.check_gram(G, m)
    _report("gram_kernel", ("ROWS", "COLS")[orient] + " " + source, worst)


@pytest.mark.parametrize("source", ["C+eta*E[idx]", "C+E[idx]", "eta*E[idx]", "E[idx]"])
@pytest.mark.parametrize("K", [600, 2100])
def test_gram_cols_gather_depth(K, source):
    """COLS with a gather: K = 600 stages eta / idx in LDS (kpre), K = 2100 > 2048 loads them per stage."""
    m, nrep = 65, 3
    Cp, Ep, idx, eta, Xs = _gram_case(1, source, m, K, nrep, True)
    G = gram(1, Cp, Ep, idx, eta, nrep, m, K)
    for j in range(nrep):
        R.check_exact(G[j, :, :m], _gram_of(Xs[j], 1))
    R.check_gram(G, m)


@pytest.mark.parametrize("orient,source,K,nrep,S", [(0, "C+eta*E[idx]", 4100, 2, 2), (1, "eta*E[idx]", 4100, 2, 2),
                                                    (0, "E[idx]", 4620, 1, 3), (1, "E", 4620, 2, 3)])
def test_gram_batched_split_k(orient, source, K, nrep, S):
    """m = 650 (66 lower tiles): gram_ksplit = 2 at K = 4100 (257 steps: 129 + 128) and 3 at K = 4620 (289 steps:
    97 + 97 + 95, with a k tail), partial images summed by gram_splitk_sum_kernel."""
    m = 650
    assert R.gram_ksplit(m, K) == S
    Cp, Ep, idx, eta, Xs = _gram_case(orient, source, m, K, nrep, True)
    G = gram(orient, Cp, Ep, idx, eta, nrep, m, K)
    for j in range(nrep):
        R.check_exact(G[j, :, :m], _gram_of(Xs[j], orient))
    R.check_gram(G, m)


@pytest.mark.parametrize("orient", [0, 1])
def test_gram_replicate_alone_has_the_same_bits(orient):
    m, K, nrep = 65, 49, 3
    Cp, Ep, idx, eta, _ = _gram_case(orient, "C+eta*E[idx]", m, K, nrep, False)
    G = gram(orient, Cp, Ep, idx, eta, nrep, m, K)
    for j in range(nrep):
        alone = gram(orient, Cp, Ep, idx[j:j + 1], eta[j:j + 1], 1, m, K)
        assert np.array_equal(alone[0], G[j], equal_nan=True), j


def test_plain_and_gathering_gram_kernels_give_the_same_bits():
    """dfm_tile.h: "every kernel sums a tile's products in the same order"; dfm_gram.hip: "the result bits do not
    depend on which kernel ran".  Where neither splits K (K < 512): gram_dma_kernel against gram_kernel, forced by
    an identity idx, on a real panel (m = 130, K = 200)."""
    m, K = 130, 200
    X, Xp = _plain_panel(m, K, False)
    plain = gram(0, None, Xp, None, None, 1, m, K)
    ident = np.arange(m + 3, dtype=np.int32).reshape(1, -1) % m
    gathered = gram(0, None, Xp, ident, None, 1, m, K)
    assert np.array_equal(plain, gathered, equal_nan=True)
