"""The checkers of tests/gemm64_reference.py on the CPU: each is fed a numpy-
made output with one of the faults a tiled MFMA kernel can have and must
reject it, and must accept the right answer.  This is the evidence that
tests/test_gpu_gemm64.py fails on a subtly wrong kernel, without a wrong
kernel in the library."""
import numpy as np
import pytest

import gemm64_reference as R

M, K, N = 65, 49, 66
PZ, NB = 6, 11   # N = NB PZ: the columns as 11 replicates of 6


def _ints():
    rng = np.random.default_rng(6401)
    A, B = R.int_mat(rng, (M, K)), R.int_mat(rng, (K, N))
    return A, B, A @ B


def _reals():
    rng = np.random.default_rng(6402)
    A, B = R.real_mat(rng, M, K), R.real_mat(rng, K, N)
    ref, ap = R.dd_product(A, B)
    return A, B, ref, ap


def _rejected(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_right_answers_pass():
    A, B, exact = _ints()
    R.check_exact(exact.copy(), exact)
    A, B, ref, ap = _reals()
    ratio = R.check_bound(A @ B, ref, ap, K)
    print(f"numpy fp64 product: {ratio:.3f} of the bound")
    assert ratio < 0.5
    s = 1.0 / 121
    assert R.check_bound((A @ B) * s, ref, ap, K, s) < 0.5


@pytest.mark.parametrize("shape", [(130, 200, 132), (65, 17, 66)])
def test_bound_has_room_for_any_fp64_order_and_none_for_fp32(shape):
    """The numpy product sits well inside the bound; a product accumulated in fp32 is > 10^5 times outside."""
    m, k, n = shape
    rng = np.random.default_rng(6403 + k)
    A, B = R.real_mat(rng, m, k), R.real_mat(rng, k, n)
    ref, ap = R.dd_product(A, B)
    assert R.check_bound(A @ B, ref, ap, k) < 0.5
    f32 = (A.astype(np.float32) @ B.astype(np.float32)).astype(np.float64)
    err = np.abs((f32 - ref.hi) - ref.lo)
    assert (err / ((k + 6) * R.U53 * ap)).max() > 1e5


def test_dropped_last_k_term():
    A, B, exact = _ints()
    _rejected(R.check_exact, A[:, :-1] @ B[:-1], exact)
    A, B, ref, ap = _reals()
    wrong = A[:, :-1] @ B[:-1]
    err = np.abs((wrong - ref.hi) - ref.lo)
    assert np.all(err > (K + 6) * R.U53 * ap)   # every entry is outside
    _rejected(R.check_bound, wrong, ref, ap, K)


def test_fp32_operands_need_the_real_family():
    """Operands rounded to fp32: invisible to the integers, far outside the bound for the reals."""
    A, B, exact = _ints()
    R.check_exact(A.astype(np.float32).astype(np.float64) @ B.astype(np.float32).astype(np.float64), exact)
    A, B, ref, ap = _reals()
    _rejected(R.check_bound, A.astype(np.float32).astype(np.float64) @ B.astype(np.float32).astype(np.float64), ref, ap, K)


def test_transposed_fragment():
    A, B, exact = _ints()
    got = exact.copy()
    got[60:64, 32:36] = exact[60:64, 32:36].T
    assert not np.array_equal(got, exact)
    _rejected(R.check_exact, got, exact)
    A, B, ref, ap = _reals()
    got = A @ B
    got[60:64, 32:36] = got[60:64, 32:36].T.copy()
    _rejected(R.check_bound, got, ref, ap, K)


def test_column_pair_swapped_across_a_replicate_boundary():
    A, B, exact = _ints()
    got = exact.copy()
    got[:, [PZ - 1, PZ]] = got[:, [PZ, PZ - 1]]
    _rejected(R.check_exact, got, exact)
    A, B, ref, ap = _reals()
    got = A @ B
    got[:, [PZ - 1, PZ]] = got[:, [PZ, PZ - 1]]
    _rejected(R.check_bound, got, ref, ap, K)


def test_written_where_nan_is_required_and_nan_where_a_value_is():
    A, B, exact = _ints()
    written = np.ones(exact.shape, dtype=bool)
    written[:, N - 2:] = False
    ok = np.where(written, exact, np.nan)
    R.check_exact(ok, exact, written)
    stray = ok.copy()
    stray[M - 1, N - 1] = exact[M - 1, N - 1]   # the right value in a place nobody may write
    _rejected(R.check_exact, stray, exact, written)
    hole = ok.copy()
    hole[17, 5] = np.nan
    _rejected(R.check_exact, hole, exact, written)
    full = R.padded(exact, M, N + 3, np.nan)
    R.check_pad_is_nan(full, N)
    full[3, N] = 0.0
    _rejected(R.check_pad_is_nan, full, N)
    A, B, ref, ap = _reals()
    got = A @ B
    got[17, 5] = np.nan
    _rejected(R.check_bound, got, ref, ap, K)
    wrong = exact.copy()
    wrong[2, 2] += 1.0
    _rejected(R.check_exact_or_untouched, wrong, exact)
    R.check_exact_or_untouched(hole, exact)


def _compacted(exact, clist, ccount, src=None):
    """What a compacted launch leaves: the listed replicates' columns (from replicate src[i]'s product), NaN elsewhere."""
    got = np.full(exact.shape, np.nan)
    src = clist if src is None else src
    for i in range(ccount):
        got[:, R.rep_cols(clist[i], PZ)] = exact[:, R.rep_cols(src[i], PZ)]
    return got


def test_wrong_clist_indirection():
    A, B, exact = _ints()
    clist = [7, 2, 9, 0, 1, 3, 4, 5, 6, 8, 10]   # ccount = 1: 8 < 11, compaction on
    R.check_compacted(_compacted(exact, clist, 1), exact, clist, 1, NB, PZ)
    # replicate clist[i + 1]'s columns in place of clist[i]'s
    _rejected(R.check_compacted, _compacted(exact, clist, 1, src=clist[1:]), exact, clist, 1, NB, PZ)
    # the right product stored at the next entry's columns
    got = np.full(exact.shape, np.nan)
    got[:, R.rep_cols(clist[1], PZ)] = exact[:, R.rep_cols(clist[1], PZ)]
    _rejected(R.check_compacted, got, exact, clist, 1, NB, PZ)
    # one replicate past ccount written as well
    got = _compacted(exact, clist, 2)
    _rejected(R.check_compacted, got, exact, clist, 1, NB, PZ)
    # ccount 8 >= nb: no compaction, every column is due
    _rejected(R.check_compacted, _compacted(exact, clist, 2), exact, clist, 2, NB, PZ)
    R.check_compacted(exact.copy(), exact, clist, 2, NB, PZ)
    # a retired replicate may be skipped or written, but not written wrongly
    done = np.zeros(NB, dtype=bool)
    done[7] = True
    R.check_compacted(np.full(exact.shape, np.nan), exact, clist, 1, NB, PZ, done)
    R.check_compacted(_compacted(exact, clist, 1), exact, clist, 1, NB, PZ, done)
    _rejected(R.check_compacted, _compacted(exact, clist, 1, src=clist[1:]), exact, clist, 1, NB, PZ, done)


def test_gram_symmetry_and_padding():
    rng = np.random.default_rng(6404)
    X = R.real_mat(rng, 20, 30)
    G = R.padded(X @ X.T, 20, 23, np.nan)
    G[:, :20] = np.tril(G[:, :20]) + np.tril(G[:, :20], -1).T
    R.check_gram(G, 20)
    H = G.copy()
    H[3, 11] = np.nextafter(H[3, 11], np.inf)
    _rejected(R.check_gram, H, 20)
    H = G.copy()
    H[5, 21] = 1.0
    _rejected(R.check_gram, H, 20)


def test_fused_panel_families_agree():
    """X* = C + eta E[idx]: the DD form rounds to the fp64 form on integers."""
    rng = np.random.default_rng(6405)
    C, E = R.int_mat(rng, (9, 12), 3), R.int_mat(rng, (9, 12), 3)
    idx, eta = R.draws(rng, 2, 9, 9, 11, True)
    assert len(set(idx[0, :9])) < 9 and eta[0, :9].min() < 0 < eta[0, :9].max()
    for c, e, x in [(C, eta, idx), (C, None, idx), (None, None, None), (None, eta, idx), (None, None, idx)]:
        i0 = None if x is None else x[0, :9]
        e0 = None if e is None else e[0, :9]
        a = R.fused_panel(c, E, i0, e0, True)
        b = R.fused_panel(c, E, i0, e0, False)
        assert np.array_equal(a, b.f64()) and np.all(b.lo == 0)


def test_split_rules_at_the_shapes_the_gpu_tests_use():
    assert R.gram_ksplit_single(70, 5003) == 19 and R.splits(19, 5003) == (19, 17, 7)
    assert R.gram_ksplit_single(130, 200) == 1
    assert R.gram_ksplit_single(130, 520) == 2 and R.splits(2, 520) == (2, 17, 16)
    assert R.gram_ksplit(650, 4100) == 2 and R.gram_ksplit(650, 4620) == 3 and R.gram_ksplit(130, 4620) == 1
