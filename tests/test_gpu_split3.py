"""The warm filter's early middle products as three bf16 MFMA terms (round 21:
dfm_gemm.hip gemmh_zrm_split_kernel<false, 3>, dfm_fact_plan.h note (7) and
FilterPlan::terms / z0_planes / mid_planes, DFM_FACT_SPLIT3).

* the kernel against its definition — the plane products (m,h) (h,m) (h,h) of
  the operands split by the rule of dfm_internal.h, rebuilt in numpy
  (tests/test_bf16_split_model.py) — on an H packed by the library's own split
  code and a Z packed with two planes by the solver's own store
  (dfm_debug_hz_split3), at the bound of a length-3K fp32 sum;
* plane l of neither operand is read: NaNs there change no byte;
* no term missing and none extra: the error against the exact product lies
  between the two-term and the six-term model's and near the three-term one's;
* batch invariance;
* the path by default, with DFM_FACT_SPLIT3=0, DFM_FACT_SPLIT=0 and
  DFM_FACT_F32=0, with the new counter beside the old two, on the shapes,
  models and cached oracle rows of tests/test_gpu_f32_filter.py and
  tests/test_gpu_warm_filter.py and on a panel with one dominant factor, whose
  filter has degree 3 (one three-term product);
* shards and lanes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_bf16_split as bf16
from test_bf16_split_model import SIX, split3, split_matmul
from test_gpu_f32_filter import (CASES, NB_MAX, _base_d0, _boot, _ctx, _d0, _draws, _env, _model, _off_case,
                                 _operands)
from test_gpu_warm_filter import _case, _check, _stats, N, B

pytestmark = pytest.mark.gpu
THREE = ((1, 0), (0, 1), (0, 0))   # (H plane, Z plane), the kernel's order


# ----------------------------------------------------------------- the kernel
def _hz_split3(Zcols, H, pz, poison=False):
    """double(C32) of the three-term kernel for the given T x nb pz block, and hmax."""
    import torch
    import dfm_pkg
    dfm = dfm_pkg.load()
    ctx = _ctx(dfm)
    fn = ctx.lib.dfm_debug_hz_split3
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                   C.POINTER(C.c_double), C.c_int]
    T = H.shape[0]
    ldH = (T + 15) // 16 * 16
    Hp = np.zeros((T, ldH))
    Hp[:, :T] = H
    nb = Zcols.shape[1] // pz
    dH = torch.from_numpy(Hp).cuda()
    dZ = torch.from_numpy(np.array(Zcols, order="C")).cuda()
    out = torch.full((T, nb * pz), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hmax = C.c_double()
    ctx.check(fn(ctx.h, dH.data_ptr(), ldH, T, dZ.data_ptr(), nb, pz, out.data_ptr(), C.byref(hmax), int(poison)))
    return out.cpu().numpy(), hmax.value


@functools.lru_cache(maxsize=None)
def _split3_case(T, pz, nb):
    H, Z = _operands(T, pz)
    got, hmax = _hz_split3(Z[:, :nb * pz], H, pz)
    got.setflags(write=False)
    return got, hmax


@functools.lru_cache(maxsize=None)
def _reference(T, pz):
    """(sum of the three plane products, sum of their absolute products) for the
    shape's 64 replicates, in fp64; a smaller batch is a column prefix."""
    H, Z = _operands(T, pz)
    Hp, Zp = split3(H / H.diagonal().max()), split3(Z)
    ref = sum(Hp[i] @ Zp[j] for i, j in THREE)
    mag = sum(np.abs(Hp[i]) @ np.abs(Zp[j]) for i, j in THREE)
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


@pytest.mark.parametrize("nb", [1, 7, 11, 64])
@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_split3_gemm_matches_its_definition(T, pz, nb):
    """C32 against the sum over the three pairs of double(H_i) @ double(Z_j),
    entrywise within 3 (T + 2) 2^-24 sum |H_i| |Z_j| — the bound of a
    length-3K fp32 sum in any order (test_gpu_bf16_split's, from six terms to
    three).  T = 121, 200: row tile edges and k not a multiple of 16; pz = 18:
    the 32-column instances' width; nb pz = 8, 84, 132, 768 (pz = 12): less
    than a tile, a tile plus four columns, whole tiles."""
    H, _ = _operands(T, pz)
    got, hmax = _split3_case(T, pz, nb)
    assert hmax == H.diagonal().max()
    ref, mag = _reference(T, pz)
    ref, bound = ref[:, :nb * pz], 3 * (T + 2) * 2.0 ** -24 * mag[:, :nb * pz]
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = np.abs(got - ref)
    print(f"T={T} pz={pz} nb={nb}: max err / bound = {(err / bound).max():.4f}")
    assert np.all(err <= bound)


def test_l_planes_are_not_read():
    """With plane l of the packed H and of every Z chunk filled with bf16 NaNs
    the result is finite and the same to the byte (T = 121, pz = 12, nb = 11)."""
    T, pz, nb = 121, 12, 11
    H, Z = _operands(T, pz)
    clean, _ = _split3_case(T, pz, nb)
    poisoned, _ = _hz_split3(Z[:, :nb * pz], H, pz, poison=True)
    assert np.all(np.isfinite(poisoned))
    assert poisoned.tobytes() == clean.tobytes()


def test_no_term_is_missing_and_none_extra():
    """Against the exact (H / hmax) Z at T = 200, pz = 12, nb = 64: the relative
    Frobenius error lies between the numpy model's with six terms and with two
    (either pair of the three), and within a factor 2 of the model's with
    the three."""
    T, pz = 200, 12
    H, Z = _operands(T, pz)
    Hn = H / H.diagonal().max()
    exact = Hn @ Z

    def rel(a):
        return np.linalg.norm(a - exact) / np.linalg.norm(exact)

    e_gpu = rel(_split3_case(T, pz, NB_MAX)[0])
    e6, e3 = rel(split_matmul(Hn, Z, SIX)), rel(split_matmul(Hn, Z, THREE))
    e2 = min(rel(split_matmul(Hn, Z, ((1, 0), (0, 0)))), rel(split_matmul(Hn, Z, ((0, 1), (0, 0)))))
    print(f"relative Frobenius error: kernel {e_gpu:.3e}; model six {e6:.3e}, three {e3:.3e}, two {e2:.3e}")
    assert e6 < e_gpu < e2
    assert 0.5 * e3 <= e_gpu <= 2.0 * e3


@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_split3_gemm_is_batch_invariant(T, pz):
    """As test_split_gemm_is_batch_invariant: replicates 0, 10, 21 and 63 run
    alone are bit-identical to their columns of the 64-replicate call, and the
    1-, 7- and 11-replicate calls are prefixes of it."""
    H, Z = _operands(T, pz)
    full, _ = _split3_case(T, pz, NB_MAX)
    for nb in (1, 7, 11):
        assert np.array_equal(_split3_case(T, pz, nb)[0], full[:, :nb * pz])
    for j in (0, 10, 21, 63):
        alone, _ = _hz_split3(Z[:, j * pz:(j + 1) * pz], H, pz)
        assert np.array_equal(alone, full[:, j * pz:(j + 1) * pz]), j


# ------------------------------------------------------------------- the path
# (121, 8): pad rows; (120, 5): the non-staged loaders; (120, 13): P = 32 at pz = 18
PATH_CASES = [(121, 8, "wild"), (120, 5, "wild"), (120, 13, "wild")]
assert set(PATH_CASES) <= set(CASES)


@functools.lru_cache(maxsize=None)
def _switch_off_case(T, r, kind):
    """(rows, iterations, eig_stats) of _case's job with DFM_FACT_SPLIT3=0."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, kind)
    with _env("DFM_FACT_SPLIT3", "0"):
        got, es = _boot(dfm, ctx, g, kind, _stats(dfm, r), idx, eta)
    got.setflags(write=False)
    return got[:, :-1], got[:, -1], es


@pytest.mark.parametrize("T,r,kind", PATH_CASES)
def test_default_path_runs_three_terms_and_matches_oracle(T, r, kind):
    """By default: the oracle's V, ICp2 and eigenvalues at 1e-10; products
    1 .. d0 - 2 of every replicate counted as three-term ones, the fp32 and
    split-last counts unchanged."""
    rows, its, ref, es = _case(T, r, kind)
    _check(rows, its, ref)
    d0 = _base_d0(T, r)
    assert d0 >= 3
    assert es["gemm_products_split3"] == (d0 - 2) * B
    assert es["gemm_products_f32"] == (d0 - 1) * B
    assert es["gemm_products_split_last"] == B


@pytest.mark.parametrize("T,r,kind", PATH_CASES)
def test_switch_off_matches_oracle(T, r, kind):
    """DFM_FACT_SPLIT3=0 (six terms throughout): no three-term product, the
    oracle's values, the other counters as before."""
    _, _, ref, _ = _case(T, r, kind)
    rows, its, es = _switch_off_case(T, r, kind)
    _check(rows, its, ref)
    assert es["gemm_products_split3"] == 0
    assert es["gemm_products_f32"] == (_base_d0(T, r) - 1) * B
    assert es["gemm_products_split_last"] == B


@pytest.mark.parametrize("T,r,kind", PATH_CASES)
def test_no_three_terms_without_the_split_products(T, r, kind):
    """DFM_FACT_SPLIT=0 and DFM_FACT_F32=0 leave nothing to run as three terms."""
    assert bf16._split_off_case(T, r, kind)[2]["gemm_products_split3"] == 0
    assert _off_case(T, r, kind)[2]["gemm_products_split3"] == 0


@functools.lru_cache(maxsize=None)
def _dominant_case(split3_on):
    """T = 120, r = 4 with the panel's first singular component six times as
    large (lambda_1 / lambda_4 ~ 58, the spread of a panel with one dominant
    factor): the first filter has degree 3.  (rows, iterations, oracle rows,
    eig_stats, d0); the oracle rows are computed once."""
    import dfm_pkg
    import dfm_oracle as oracle
    dfm = dfm_pkg.load()
    T, r = 120, 4
    rng = np.random.default_rng(8100 + 10 * r)
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    u, s, vt = np.linalg.svd(x, full_matrices=False)
    x = x + 5.0 * s[0] * np.outer(u[:, 0], vt[0])
    w = np.ones((T, 1))
    ctx = dfm.Context(0)
    g = dfm.DynamicFactorModel(y, w, x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    idx, eta = dfm.draw_wild_fast(500 + r, B, T)
    with _env("DFM_FACT_SPLIT3", None if split3_on else "0"):
        got, es = _boot(dfm, ctx, g, "wild", _stats(dfm, r), idx, eta)
    got.setflags(write=False)
    if not split3_on:
        return got[:, :-1], got[:, -1], _dominant_case(True)[2], es, _dominant_case(True)[4]
    base = oracle.DynamicFactorModel(y, w, x, r, "ICp2")
    ref = np.empty((B, 2 + r))
    for b in range(B):
        xs = base.common_component + eta[b][:, None] * base.factor_residuals[idx[b]]
        d = oracle.DynamicFactorModel(y, w, xs, r, "ICp2")
        ref[b, 0] = oracle.factor_residual_variance(d)
        ref[b, 1] = d.number_of_factors_criterion_value
        ref[b, 2:] = d.eigenvalues[0][:r]
    ref.setflags(write=False)
    return got[:, :-1], got[:, -1], ref, es, _d0(np.asarray(base.eigenvalues[0], dtype=float), r)


@pytest.mark.parametrize("split3_on", [True, False])
def test_degree_three_filter_runs_one_three_term_product(split3_on):
    """One dominant factor: d0 = 3, so product 1 alone runs as three terms
    (none with the switch off), products 1 and 2 count as fp32 ones, product 3
    as the split last one, and the rows meet the oracle at 1e-10."""
    rows, its, ref, es, d0 = _dominant_case(split3_on)
    assert d0 == 3
    _check(rows, its, ref)
    assert es["gemm_products_split3"] == (B if split3_on else 0)
    assert es["gemm_products_f32"] == 2 * B
    assert es["gemm_products_split_last"] == B


def test_split3_path_shards_are_bit_identical(dfm, oracle):
    """As test_gpu_f32_filter.test_fp32_path_shards_are_bit_identical, with the
    three-term products on (checked by the counter): whole, halves (48 + 48),
    the 8 slowest alone."""
    T, r, nrep = 120, 8, 96
    rng = np.random.default_rng(8300)
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    ctx = dfm.Context(0)
    g = dfm.DynamicFactorModel(y, np.ones((T, 1)), x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    idx, eta = dfm.draw_wild_fast(31, nrep, T)
    stats = _stats(dfm, r)
    ctx.reset_timing()
    full = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
    ctx.synchronize()
    es = ctx.eig_stats()
    assert es["gemm_products_split3"] >= nrep and es["gemm_products_split3"] == es["gemm_products_f32"] - nrep
    assert np.all(np.isfinite(full)) and full[:, -1].min() >= 2
    lo = dfm.wild_bootstrap(g, 48, stats, idx=idx[:48], eta=eta[:48])
    hi = dfm.wild_bootstrap(g, 48, stats, idx=idx[48:], eta=eta[48:])
    assert np.array_equal(full[:48, :-1], lo[:, :-1]) and np.array_equal(full[48:, :-1], hi[:, :-1])
    slow = np.argsort(-full[:, -1], kind="stable")[:8]
    alone = dfm.wild_bootstrap(g, 8, stats, idx=idx[slow], eta=eta[slow])
    assert np.array_equal(full[slow, :-1], alone[:, :-1])


def test_split3_path_two_lanes_are_bit_identical(dfm, oracle):
    """As test_gpu_f32_filter.test_fp32_path_two_lanes_are_bit_identical: 600
    replicates as two lanes against one batch of 600, rows equal to the bit;
    both lanes' three-term counts reach the caller's context."""
    T, r, nrep = 120, 8, 600
    rng = np.random.default_rng(8400)
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    ctx = dfm.Context(0)
    g = dfm.DynamicFactorModel(y, np.ones((T, 1)), x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    idx, eta = dfm.draw_wild_fast(41, nrep, T)
    stats = _stats(dfm, r)
    ctx.reset_timing()
    lanes = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
    ctx.synchronize()
    es_lanes = ctx.eig_stats()
    g.set_batch(nrep)
    ctx.reset_timing()
    one = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
    ctx.synchronize()
    es_one = ctx.eig_stats()
    assert es_one["gemm_products_split3"] >= nrep
    assert es_one["gemm_products_split3"] == es_one["gemm_products_f32"] - nrep
    assert es_lanes["gemm_products_split3"] == es_one["gemm_products_split3"]
    assert np.all(np.isfinite(lanes)) and np.array_equal(lanes[:, :-1], one[:, :-1])
