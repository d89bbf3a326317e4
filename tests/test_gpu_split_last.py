"""The warm filter's last H.Z product as six bf16 MFMA terms (round 19:
dfm_gemm.hip gemmh_zrm_split_kernel<ROWS64>, dfm_fact.hip eig_run_fact2_t
`split_last`, DFM_FACT_SPLIT_LAST).

* the fp64 epilogue against the float one, bit for bit: dfm_debug_hz_split_rows
  must equal float64(C32) * hmax (one fp64 multiply) with C32 from
  dfm_debug_hz_split, at the shapes of tests/test_gpu_bf16_split.py — and
  nothing but the T x nb pz block of a NaN-filled, padded and guarded `out`
  may be written (T = 121 catches a missing per-row test);
* batch invariance of that epilogue;
* the path on the shapes, models and cached oracle rows of
  tests/test_gpu_f32_filter.py and tests/test_gpu_warm_filter.py: by default,
  with DFM_FACT_SPLIT_LAST=0, with DFM_FACT_SPLIT=0 / DFM_FACT_F32=0 and under
  the strict rule, with the new counter beside the fp32 one;
* no hidden cost in Rayleigh-Ritz steps against DFM_FACT_SPLIT_LAST=0.

Shards and lanes: test_gpu_f32_filter.py's and test_gpu_bf16_split.py's shard
and lane tests run the default path, which is this one, and so already cover
it (T = 120: eight pad rows in the last chunk of Z); they are not copied here.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_bf16_split as bf16
from test_gpu_f32_filter import (CASES, NB_MAX, _base_d0, _boot, _ctx, _draws, _env, _model, _off_case,
                                 _operands)
from test_gpu_warm_filter import _case, _check, _stats, B

pytestmark = pytest.mark.gpu
PAD, GUARD = 5, 8


# --------------------------------------------------------------- the epilogue
def _hz_split_rows(Zcols, H, pz):
    """The whole (T + GUARD) x (nb pz + PAD) buffer, NaN-filled before
    dfm_debug_hz_split_rows wrote its T x nb pz block into it, and hmax."""
    import torch
    import dfm_pkg
    dfm = dfm_pkg.load()
    ctx = _ctx(dfm)
    fn = ctx.lib.dfm_debug_hz_split_rows
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                   C.POINTER(C.c_double)]
    T = H.shape[0]
    ldH = (T + 15) // 16 * 16
    Hp = np.zeros((T, ldH))
    Hp[:, :T] = H
    nb = Zcols.shape[1] // pz
    ldo = nb * pz + PAD
    dH = torch.from_numpy(Hp).cuda()
    dZ = torch.from_numpy(np.array(Zcols, order="C")).cuda()
    out = torch.full((T + GUARD, ldo), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hmax = C.c_double()
    ctx.check(fn(ctx.h, dH.data_ptr(), ldH, T, dZ.data_ptr(), nb, pz, out.data_ptr(), ldo, C.byref(hmax)))
    torch.cuda.synchronize()
    return out.cpu().numpy(), hmax.value


@functools.lru_cache(maxsize=None)
def _rows_case(T, pz, nb):
    H, Z = _operands(T, pz)
    buf, hmax = _hz_split_rows(Z[:, :nb * pz], H, pz)
    buf.setflags(write=False)
    return buf, hmax


SHAPES = [(T, pz, nb) for T in (120, 121, 200) for pz in (8, 12, 18) for nb in (1, 7, 11, 64)]


@pytest.mark.parametrize("T,pz,nb", SHAPES)
def test_fp64_epilogue_equals_the_float_one(T, pz, nb):
    """hmax C32 as fp64 rows, bit for bit: the kernel's main loop is the float
    instance's, the epilogue one conversion and one fp64 multiply.  T = 121,
    200: row tile edges and k not a multiple of 16; nb pz = 8, 84, 132, 768
    (pz = 12): less than a column tile, a tile plus four columns, whole tiles."""
    buf, hmax = _rows_case(T, pz, nb)
    c32, hmax32 = bf16._split_case(T, pz, nb)
    assert hmax == hmax32 == _operands(T, pz)[0].diagonal().max()
    got = buf[:T, :nb * pz]
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, c32 * hmax)


@pytest.mark.parametrize("T,pz,nb", SHAPES)
def test_nothing_else_is_written(T, pz, nb):
    """Every pad column (row stride nb pz + 5) and the eight guard rows below
    row T are still NaN."""
    buf, _ = _rows_case(T, pz, nb)
    assert buf.shape == (T + GUARD, nb * pz + PAD)
    assert np.all(np.isnan(buf[:, nb * pz:]))
    assert np.all(np.isnan(buf[T:, :]))


@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_fp64_epilogue_is_batch_invariant(T, pz):
    """Replicates 0, 10, 21 and 63 run alone are bit-identical to their
    columns of the 64-replicate call."""
    H, Z = _operands(T, pz)
    full = _rows_case(T, pz, NB_MAX)[0][:T, :NB_MAX * pz]
    for j in (0, 10, 21, 63):
        alone, _ = _hz_split_rows(Z[:, j * pz:(j + 1) * pz], H, pz)
        assert np.array_equal(alone[:T, :pz], full[:, j * pz:(j + 1) * pz]), j


# ------------------------------------------------------------------- the path
@functools.lru_cache(maxsize=None)
def _last_off_case(T, r, kind):
    """(rows, iterations, eig_stats) of _case's job with DFM_FACT_SPLIT_LAST=0."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, kind)
    with _env("DFM_FACT_SPLIT_LAST", "0"):
        got, es = _boot(dfm, ctx, g, kind, _stats(dfm, r), idx, eta)
    got.setflags(write=False)
    return got[:, :-1], got[:, -1], es


@pytest.mark.parametrize("T,r,kind", CASES)
def test_default_path_runs_the_last_product_split(T, r, kind):
    """By default: the oracle's V, ICp2 and eigenvalues at 1e-10, every
    replicate's last filter product counted, the fp32 count unchanged."""
    rows, its, ref, es = _case(T, r, kind)
    _check(rows, its, ref)
    assert es["gemm_products_split_last"] == B
    assert es["gemm_products_f32"] == (_base_d0(T, r) - 1) * B


@pytest.mark.parametrize("T,r,kind", CASES)
def test_switch_off_matches_oracle(T, r, kind):
    """DFM_FACT_SPLIT_LAST=0 (the fp64 last product): the oracle's values, no
    split last product, the middle ones as before."""
    _, _, ref, _ = _case(T, r, kind)
    rows, its, es = _last_off_case(T, r, kind)
    _check(rows, its, ref)
    assert es["gemm_products_split_last"] == 0
    assert es["gemm_products_f32"] == (_base_d0(T, r) - 1) * B


@pytest.mark.parametrize("T,r,kind", CASES)
def test_no_split_last_without_the_split_middle_products(T, r, kind):
    """DFM_FACT_SPLIT=0 and DFM_FACT_F32=0 keep the last product in fp64."""
    assert bf16._split_off_case(T, r, kind)[2]["gemm_products_split_last"] == 0
    assert _off_case(T, r, kind)[2]["gemm_products_split_last"] == 0


def test_strict_rule_stays_fp64_bit_for_bit():
    """A statistic that needs vectors solves under the strict rule: no split
    last product, the same rows to the bit with the switch on and off."""
    T, r = 120, 8
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    S = dfm.Stat
    stats = [S.V(), S.criterion(), S.eigenvalue(1), S.eigenvalue(r), S.coefficient(1), S.iterations()]
    with _env("DFM_FACT_SPLIT_LAST", None):
        on, es_on = _boot(dfm, ctx, g, "wild", stats, idx, eta)
    with _env("DFM_FACT_SPLIT_LAST", "0"):
        off, es_off = _boot(dfm, ctx, g, "wild", stats, idx, eta)
    assert es_on["gemm_products_split_last"] == 0 and es_off["gemm_products_split_last"] == 0
    assert np.all(np.isfinite(on)) and np.array_equal(on, off)


@pytest.mark.parametrize("T,r,kind", CASES)
def test_no_hidden_cost_in_rayleigh_ritz_steps(T, r, kind):
    """At most B // 16 more Rayleigh-Ritz replicate-steps than with the fp64
    last product: the cap of the fp32 tests (the CPU model shows no change at
    these shapes; the cap keeps a regression from hiding)."""
    es = _case(T, r, kind)[3]
    es_off = _last_off_case(T, r, kind)[2]
    print(f"replicate_iterations: split last {es['replicate_iterations']}, fp64 last {es_off['replicate_iterations']}")
    assert es["replicate_iterations"] <= es_off["replicate_iterations"] + B // 16
