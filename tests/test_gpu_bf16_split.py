"""The warm filter's middle products as six bf16 MFMA terms (round 15:
dfm_gemm.hip gemmh_zrm_split_kernel, dfm_fact.hip eig_run_fact2_t `split`).

* the kernel against its definition — the six plane products of the operands
  split by the rule of dfm_internal.h, rebuilt in numpy
  (tests/test_bf16_split_model.py) — on operands packed by the library's own
  split code (dfm_debug_hz_split), at the bound of a length-6K fp32 sum;
* no term missing: against the exact product the kernel is as close as the
  fp32 kernel (the worst-case bound above cannot see a dropped 2^-18 term);
* batch invariance;
* the default path and DFM_FACT_SPLIT=0 against the oracle, a panel scaled by
  1e12, shards and lanes — on the shapes, models and cached oracle rows of
  tests/test_gpu_f32_filter.py and tests/test_gpu_warm_filter.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_f32_filter as f32
from test_bf16_split_model import SIX, split3
from test_gpu_f32_filter import CASES, NB_MAX, _base_d0, _boot, _ctx, _draws, _env, _model, _operands
from test_gpu_warm_filter import _case, _check, _stats, B

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- the kernel
def _hz_split(Zcols, H, pz):
    """double(C32) of gemmh_zrm_split_kernel for the given T x nb pz block, and hmax."""
    import torch
    import dfm_pkg
    dfm = dfm_pkg.load()
    ctx = _ctx(dfm)
    fn = ctx.lib.dfm_debug_hz_split
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                   C.POINTER(C.c_double)]
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
    ctx.check(fn(ctx.h, dH.data_ptr(), ldH, T, dZ.data_ptr(), nb, pz, out.data_ptr(), C.byref(hmax)))
    return out.cpu().numpy(), hmax.value


@functools.lru_cache(maxsize=None)
def _split_case(T, pz, nb):
    H, Z = _operands(T, pz)
    got, hmax = _hz_split(Z[:, :nb * pz], H, pz)
    got.setflags(write=False)
    return got, hmax


@functools.lru_cache(maxsize=None)
def _reference(T, pz):
    """(sum of the six plane products, sum of their absolute products) for the
    shape's 64 replicates, in fp64; a smaller batch is a column prefix."""
    H, Z = _operands(T, pz)
    Hp, Zp = split3(H / H.diagonal().max()), split3(Z)
    ref = sum(Hp[i] @ Zp[j] for i, j in SIX)
    mag = sum(np.abs(Hp[i]) @ np.abs(Zp[j]) for i, j in SIX)
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


@pytest.mark.parametrize("nb", [1, 7, 11, 64])
@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_split_gemm_matches_its_definition(T, pz, nb):
    """C32 against the sum over the six pairs of double(H_i) @ double(Z_j),
    entrywise within 6 (T + 2) 2^-24 sum |H_i| |Z_j| — the bound of a
    length-6K fp32 sum in any order.  T = 121, 200: row tile edges and k not a
    multiple of 16; pz = 18: the 32-column instances' width; nb pz = 8, 84,
    132, 768 (pz = 12): less than a tile, a tile plus four columns, whole tiles."""
    H, _ = _operands(T, pz)
    got, hmax = _split_case(T, pz, nb)
    assert hmax == H.diagonal().max()
    ref, mag = _reference(T, pz)
    ref, bound = ref[:, :nb * pz], 6 * (T + 2) * 2.0 ** -24 * mag[:, :nb * pz]
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = np.abs(got - ref)
    print(f"T={T} pz={pz} nb={nb}: max err / bound = {(err / bound).max():.4f}")
    assert np.all(err <= bound)


def test_no_term_is_missing():
    """Against the exact (H / hmax) Z at T = 200, pz = 12, nb = 64 the split
    kernel's relative Frobenius error is at most twice the fp32 kernel's (CPU
    model: 0.94 x; with three terms only, 12 x)."""
    T, pz = 200, 12
    H, Z = _operands(T, pz)
    exact = (H / H.diagonal().max()) @ Z
    e_split = np.linalg.norm(_split_case(T, pz, NB_MAX)[0] - exact) / np.linalg.norm(exact)
    e_f32 = np.linalg.norm(f32._hz_case(T, pz, NB_MAX)[0] - exact) / np.linalg.norm(exact)
    print(f"relative Frobenius error: split {e_split:.3e}, fp32 {e_f32:.3e}, ratio {e_split / e_f32:.3f}")
    assert e_split <= 2.0 * e_f32


@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_split_gemm_is_batch_invariant(T, pz):
    """As test_f32_gemm_is_batch_invariant: replicates 0, 10, 21 and 63 run
    alone are bit-identical to their columns of the 64-replicate call, and the
    1- and 7-replicate calls are prefixes of it."""
    H, Z = _operands(T, pz)
    full, _ = _split_case(T, pz, NB_MAX)
    for nb in (1, 7):
        assert np.array_equal(_split_case(T, pz, nb)[0], full[:, :nb * pz])
    for j in (0, 10, 21, 63):
        alone, _ = _hz_split(Z[:, j * pz:(j + 1) * pz], H, pz)
        assert np.array_equal(alone, full[:, j * pz:(j + 1) * pz]), j


# ------------------------------------------------------------------- the path
@functools.lru_cache(maxsize=None)
def _split_off_case(T, r, kind):
    """(rows, iterations, eig_stats) of _case's job with DFM_FACT_SPLIT=0."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, kind)
    with _env("DFM_FACT_SPLIT", "0"):
        got, es = _boot(dfm, ctx, g, kind, _stats(dfm, r), idx, eta)
    got.setflags(write=False)
    return got[:, :-1], got[:, -1], es


@pytest.mark.parametrize("T,r,kind", CASES)
def test_default_path_matches_oracle(T, r, kind):
    """The default (split) path: the oracle's V, ICp2 and top-r eigenvalues at
    1e-10, and the d0 - 1 middle products of every replicate counted as
    low-precision products."""
    rows, its, ref, es = _case(T, r, kind)
    _check(rows, its, ref)
    assert es["gemm_products_f32"] == (_base_d0(T, r) - 1) * B


@pytest.mark.parametrize("T,r,kind", CASES)
def test_split_off_matches_oracle(T, r, kind):
    """DFM_FACT_SPLIT=0 (the fp32 launches): the oracle's values, the same counter."""
    _, _, ref, _ = _case(T, r, kind)
    rows, its, es = _split_off_case(T, r, kind)
    _check(rows, its, ref)
    assert es["gemm_products_f32"] == (_base_d0(T, r) - 1) * B


def test_panel_scaled_by_1e12_matches_oracle():
    """The default path on the panel times 1e12 (H / hmax is split, hmax goes
    back in as an fp64 factor; Z's planes have fp32's exponent range)."""
    f32.test_panel_scaled_by_1e12_matches_oracle()


def test_split_path_shards_are_bit_identical(dfm, oracle):
    """Whole, halves and the 8 slowest alone on the default path, compared as the fp32 test compares them."""
    f32.test_fp32_path_shards_are_bit_identical(dfm, oracle)


def test_split_path_two_lanes_are_bit_identical(dfm, oracle):
    """Two lanes (the second on a clone, which rebuilds the split H on its own
    stream) against one batch on the default path, as the fp32 test compares them."""
    f32.test_fp32_path_two_lanes_are_bit_identical(dfm, oracle)
