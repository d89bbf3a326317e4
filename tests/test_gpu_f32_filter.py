"""The fp32 middle products of a warm eigenvalue-rule solve (round 8:
dfm_gemm.hip gemmh_zrm_f32_kernel, dfm_fact.hip eig_run_fact2_t `lowp`).

* the fp32 H.Z kernel against its definition, on operands packed by the
  library (dfm_debug_hz_f32), at the standard bound of a length-K fp32 sum,
  and its batch invariance;
* the path on, off (DFM_FACT_F32=0) and under the strict rule against the
  oracle, at the warm filter's smallest shapes (tests/test_gpu_warm_filter.py,
  whose cached default-path rows and oracle rows are reused);
* shard and lane invariance on the fp32 path;
* a panel scaled by 1e12 (H32 is normalised by its largest diagonal entry).
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from test_gpu_warm_filter import _case, _check, _stats, N, B

pytestmark = pytest.mark.gpu
RTOL = 1e-10


# ----------------------------------------------------------------- the kernel
NB_MAX = 64


@functools.lru_cache(maxsize=None)
def _operands(T, pz):
    """H = E E' (positive semidefinite, T x T) and Z (T x 64 pz), fixed per shape."""
    rng = np.random.default_rng(9000 + 100 * T + pz)
    E = rng.standard_normal((T, 2 * T)) * rng.uniform(0.2, 3.0, size=(T, 1))
    H = E @ E.T
    Z = rng.standard_normal((T, NB_MAX * pz)) * rng.uniform(0.1, 10.0, size=(1, NB_MAX * pz))
    H.setflags(write=False)
    Z.setflags(write=False)
    return H, Z


def _hz_f32(Zcols, H, pz):
    """double(H32 Z32) of the library for the given T x nb pz block, and hmax."""
    import torch
    import dfm_pkg
    dfm = dfm_pkg.load()
    ctx = _ctx(dfm)
    fn = ctx.lib.dfm_debug_hz_f32
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                   C.POINTER(C.c_double)]
    T = H.shape[0]
    ldH = (T + 15) // 16 * 16
    Hp = np.zeros((T, ldH))
    Hp[:, :T] = H
    nb = Zcols.shape[1] // pz
    dH = torch.from_numpy(Hp).cuda()
    dZ = torch.from_numpy(np.array(Zcols, order="C")).cuda()   # (a writable copy of the cached block)
    out = torch.full((T, nb * pz), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    hmax = C.c_double()
    ctx.check(fn(ctx.h, dH.data_ptr(), ldH, T, dZ.data_ptr(), nb, pz, out.data_ptr(), C.byref(hmax)))
    return out.cpu().numpy(), hmax.value


@functools.lru_cache(maxsize=None)
def _ctx(dfm):
    return dfm.Context(0)


@functools.lru_cache(maxsize=None)
def _hz_case(T, pz, nb):
    H, Z = _operands(T, pz)
    got, hmax = _hz_f32(Z[:, :nb * pz], H, pz)
    got.setflags(write=False)
    return got, hmax


@pytest.mark.parametrize("nb", [1, 7, 64])
@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_f32_gemm_matches_its_definition(T, pz, nb):
    """C32 = H32 Z32 against double(H32) @ double(Z32) from the rounded
    operands, entrywise within (K + 2) 2^-24 (|H32| |Z32|) — the bound of a
    length-K fp32 fma chain in any order.  T = 121, 200: row tile edges and k
    not a multiple of 16; nb pz not a multiple of the 128-column tile."""
    H, Z = _operands(T, pz)
    got, hmax = _hz_case(T, pz, nb)
    assert hmax == H.diagonal().max()
    H32 = (H / hmax).astype(np.float32)
    Z32 = Z[:, :nb * pz].astype(np.float32)
    assert np.abs(H32).max() <= 1.0
    ref = H32.astype(np.float64) @ Z32.astype(np.float64)
    bound = (T + 2) * 2.0 ** -24 * (np.abs(H32).astype(np.float64) @ np.abs(Z32).astype(np.float64))
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    err = np.abs(got - ref)
    print(f"T={T} pz={pz} nb={nb}: max err / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("pz", [8, 12, 18])
@pytest.mark.parametrize("T", [120, 121, 200])
def test_f32_gemm_is_batch_invariant(T, pz):
    """Replicate j's columns in the 64-replicate call are bit-identical to the
    same replicate run alone (j = 0; 10 and 21, whose columns straddle a
    128-column tile edge at pz = 12 / 18; 63, the last), and the 1- and
    7-replicate calls are prefixes of the 64-replicate one."""
    H, Z = _operands(T, pz)
    full, _ = _hz_case(T, pz, NB_MAX)
    for nb in (1, 7):
        assert np.array_equal(_hz_case(T, pz, nb)[0], full[:, :nb * pz])
    for j in (0, 10, 21, 63):
        alone, _ = _hz_f32(Z[:, j * pz:(j + 1) * pz], H, pz)
        assert np.array_equal(alone, full[:, j * pz:(j + 1) * pz]), j


# ------------------------------------------------------- path on / off / strict
class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.saved = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.saved is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.saved


def _model(T, r, scale=1.0):
    """The model and draws of test_gpu_warm_filter._case(T, r, kind) (same seeds)."""
    import dfm_pkg
    import dfm_oracle as oracle
    dfm = dfm_pkg.load()
    rng = np.random.default_rng(8100 + 10 * r + (T - 120))
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x) * scale
    w = np.ones((T, 1))
    ctx = dfm.Context(0)
    g = dfm.DynamicFactorModel(y, w, x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    return dfm, oracle, ctx, g, y, w, x


def _draws(dfm, oracle, T, r, kind):
    if kind == "wild":
        return dfm.draw_wild_fast(500 + r, B, T)
    return oracle.draw_residual(np.random.default_rng(600 + r), B, T), None


def _boot(dfm, ctx, g, kind, stats, idx, eta):
    ctx.reset_timing()
    if kind == "wild":
        got = dfm.wild_bootstrap(g, B, stats, idx=idx, eta=eta)
    else:
        got = dfm.residual_bootstrap(g, B, stats, idx=idx)
    ctx.synchronize()
    return got, ctx.eig_stats()


@functools.lru_cache(maxsize=None)
def _off_case(T, r, kind):
    """(rows, iterations, eig_stats) of _case's job with DFM_FACT_F32=0."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, kind)
    with _env("DFM_FACT_F32", "0"):
        got, es = _boot(dfm, ctx, g, kind, _stats(dfm, r), idx, eta)
    got.setflags(write=False)
    return got[:, :-1], got[:, -1], es


def _d0(lam, r):
    """first_filter_degree (dfm_fact.hip) of the base fit's eigenvalues."""
    ratio = max(1.0001, 1.1 * lam[0] / lam[r - 1])
    return max(2, min(6, int(math.floor(math.log(1e6) / math.log(ratio)))))


@functools.lru_cache(maxsize=None)
def _base_d0(T, r):
    _, oracle, _, _, y, w, x = _model(T, r)
    base = oracle.DynamicFactorModel(y, w, x, r, "ICp2")
    return _d0(np.asarray(base.eigenvalues[0], dtype=float), r)


CASES = [(120, 4, "wild"), (120, 5, "wild"), (120, 8, "wild"), (120, 13, "wild"), (120, 8, "residual"),
         (121, 8, "wild")]


@pytest.mark.parametrize("T,r,kind", CASES)
def test_default_path_runs_fp32_and_matches_oracle(T, r, kind):
    """Eigenvalue statistics: the d0 - 1 middle products of every replicate
    run in fp32, and V, ICp2 and the top-r eigenvalues match the oracle."""
    rows, its, ref, es = _case(T, r, kind)
    _check(rows, its, ref)
    d0 = _base_d0(T, r)
    assert d0 >= 3
    assert es["gemm_products_f32"] == (d0 - 1) * B
    assert es["gemm_products"] >= es["gemm_products_f32"] + B + es["replicate_iterations"]


@pytest.mark.parametrize("T,r,kind", CASES)
def test_switch_off_is_fp64_and_matches_oracle(T, r, kind):
    """DFM_FACT_F32=0: no fp32 product, the oracle's values; the fp32 path
    needs at most B // 16 more Rayleigh-Ritz replicate-steps than this one
    (the CPU model shows none: the cap keeps a regression from hiding)."""
    _, _, ref, es = _case(T, r, kind)
    rows, its, es_off = _off_case(T, r, kind)
    _check(rows, its, ref)
    assert es_off["gemm_products_f32"] == 0
    print(f"replicate_iterations: fp32 {es['replicate_iterations']}, fp64 {es_off['replicate_iterations']}")
    assert es["replicate_iterations"] <= es_off["replicate_iterations"] + B // 16


def test_strict_rule_stays_fp64_bit_for_bit():
    """A statistic that needs vectors (a coefficient) solves under the strict
    rule: no fp32 product, and the rows are the same to the bit with the
    switch on and off."""
    T, r = 120, 8
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    S = dfm.Stat
    stats = [S.V(), S.criterion(), S.eigenvalue(1), S.eigenvalue(r), S.coefficient(1), S.iterations()]
    with _env("DFM_FACT_F32", None):
        on, es_on = _boot(dfm, ctx, g, "wild", stats, idx, eta)
    with _env("DFM_FACT_F32", "0"):
        off, es_off = _boot(dfm, ctx, g, "wild", stats, idx, eta)
    assert es_on["gemm_products_f32"] == 0 and es_off["gemm_products_f32"] == 0
    assert np.all(np.isfinite(on)) and np.array_equal(on, off)


# ------------------------------------------------------------------ invariance
def test_fp32_path_shards_are_bit_identical(dfm, oracle):
    """As test_gpu_warm_filter.test_shards_are_bit_identical, with the fp32
    products on (checked by the counter): whole, halves, the 8 slowest alone."""
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
    assert ctx.eig_stats()["gemm_products_f32"] >= 2 * nrep
    assert np.all(np.isfinite(full)) and full[:, -1].min() >= 2
    lo = dfm.wild_bootstrap(g, 48, stats, idx=idx[:48], eta=eta[:48])
    hi = dfm.wild_bootstrap(g, 48, stats, idx=idx[48:], eta=eta[48:])
    assert np.array_equal(full[:48, :-1], lo[:, :-1]) and np.array_equal(full[48:, :-1], hi[:, :-1])
    slow = np.argsort(-full[:, -1], kind="stable")[:8]
    alone = dfm.wild_bootstrap(g, 8, stats, idx=idx[slow], eta=eta[slow])
    assert np.array_equal(full[slow, :-1], alone[:, :-1])


def test_fp32_path_two_lanes_are_bit_identical(dfm, oracle):
    """600 replicates run as two lanes (the second on a clone, which rebuilds
    H32 on its own stream); an explicit batch of 600 keeps one lane, the path
    DFM_NO_LANES=1 forces (that switch is read once per process).  Rows equal
    to the bit, iteration column excluded; both lanes' fp32 counts reach the
    caller's context."""
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
    f32_lanes = ctx.eig_stats()["gemm_products_f32"]
    g.set_batch(nrep)
    ctx.reset_timing()
    one = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
    ctx.synchronize()
    f32_one = ctx.eig_stats()["gemm_products_f32"]
    assert f32_one >= 2 * nrep and f32_lanes == f32_one
    assert np.all(np.isfinite(lanes)) and np.array_equal(lanes[:, :-1], one[:, :-1])


# ---------------------------------------------------------------- scale safety
def test_panel_scaled_by_1e12_matches_oracle():
    """The r = 8 case with the normalised panel multiplied by 1e12: H's
    entries are ~1e26 N, H32 = H / hmax stays within [-1, 1] and hmax goes
    back in as an fp64 factor.  Finite, and the oracle's values at 1e-10."""
    T, r, scale = 120, 8, 1e12
    dfm, oracle, ctx, g, y, w, x = _model(T, r, scale)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    got, es = _boot(dfm, ctx, g, "wild", _stats(dfm, r), idx, eta)
    base = oracle.DynamicFactorModel(y, w, x, r, "ICp2")
    assert es["gemm_products_f32"] == (_d0(np.asarray(base.eigenvalues[0], dtype=float), r) - 1) * B
    ref = np.empty((B, 2 + r))
    for b in range(B):
        xs = base.common_component + eta[b][:, None] * base.factor_residuals[idx[b]]
        d = oracle.DynamicFactorModel(y, w, xs, r, "ICp2")
        ref[b, 0] = oracle.factor_residual_variance(d)
        ref[b, 1] = d.number_of_factors_criterion_value
        ref[b, 2:] = d.eigenvalues[0][:r]
    _check(got[:, :-1], got[:, -1], ref)
