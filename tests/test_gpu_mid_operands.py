"""The factored bootstrap's per-replicate passes without bytes the result does
not need (dfm_fact.hip).

Part A — DFM_FACT_PF=0: a warm solve that starts with the filter takes the
middle Horner steps' PF = P'D F from PV's rows (boot_cheb_mid_kernel's NOPF
instances; F = sqrt(T) times the warm vectors, which are Q0's first r
columns), and boot_prep_kernel neither builds nor stores PF.  Unset, PF is
stored and read as before (the default: the new form's measured gain stayed
under this project's bar, profiles/r10_c3_ab.txt).  Shapes: those of
tests/test_gpu_f32_filter.py, whose cached default rows and oracle rows are
reused — T = 120 and 121 (tile edge, pad rows), r = 4 (pz = 8, one load
round), 5 (odd r, the non-staged EL loader, pz = 10), 8 (pz = 12, one and a
half rounds), 13 (the 32-column instance, pz = 18: the stage's sizing), wild
and residual draws.  The change is one rounding per PF element, so both forms
are held against the oracle at the project's 1e-10 and against each other
only through the iteration count.

Part B — boot_ap2_kernel decides before it writes (`probe`): with
DFM_AP2_PROBE unset and =0 every row, the iteration column and every counter
are equal to the bit.
"""
import functools

import numpy as np
import pytest

from test_gpu_warm_filter import _case, _check, _stats, N, B
from test_gpu_f32_filter import CASES, _boot, _draws, _env, _model

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------- part A
@functools.lru_cache(maxsize=None)
def _nopf_case(T, r, kind):
    """(rows, iterations, eig_stats) of _case's job with DFM_FACT_PF=0 (PF from PV's rows)."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, kind)
    with _env("DFM_FACT_PF", "0"):
        got, es = _boot(dfm, ctx, g, kind, _stats(dfm, r), idx, eta)
    got.setflags(write=False)
    return got[:, :-1], got[:, -1], es


@pytest.mark.parametrize("T,r,kind", CASES)
def test_pf_from_pv_and_stored_pf_match_oracle(T, r, kind):
    """Both forms give the oracle's V, ICp2 and top-r eigenvalues, run the same
    fp32 products, and the new form needs at most B // 16 more Rayleigh-Ritz
    replicate-steps than stored PF (a rounding-level change: 0 expected)."""
    rows_pf, its_pf, ref, es_pf = _case(T, r, kind)
    _check(rows_pf, its_pf, ref)
    rows, its, es = _nopf_case(T, r, kind)
    _check(rows, its, ref)
    print(f"replicate_iterations: PF from PV {es['replicate_iterations']}, stored PF {es_pf['replicate_iterations']}; "
          f"max rel diff of the rows {np.max(np.abs(rows - rows_pf) / np.abs(rows_pf)):.3e}")
    assert es["gemm_products_f32"] == es_pf["gemm_products_f32"] > 0
    assert es["replicate_iterations"] <= es_pf["replicate_iterations"] + B // 16
    # the NOPF kernels did run at this shape: with the switch ignored (kw < r, fscale 0) both jobs would be the
    # same launches and equal to the bit, while sqrt(T) * sum(h u) and sum(h * (sqrt(T) u)) round differently in
    # some of the T * r PF elements of 64 replicates, and every row depends on all of them
    assert not np.array_equal(rows, rows_pf)


@functools.lru_cache(maxsize=None)
def _strict_ref(T, r):
    """Oracle V, ICp2, eigenvalues 1 and r and the first coefficient of _case(T, r, "wild")'s draws, and the
    largest coefficient magnitude of each refit."""
    dfm, oracle, ctx, g, y, w, x = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    base = oracle.DynamicFactorModel(y, w, x, r, "ICp2")
    ref, cmax = np.empty((B, 5)), np.empty(B)
    for b in range(B):
        d = oracle.DynamicFactorModel(y, w, base.common_component + eta[b][:, None] * base.factor_residuals[idx[b]],
                                      r, "ICp2")
        ref[b] = [oracle.factor_residual_variance(d), d.number_of_factors_criterion_value, d.eigenvalues[0][0],
                  d.eigenvalues[0][r - 1], d.coefficients[0]]
        cmax[b] = np.max(np.abs(d.coefficients))
    ref.setflags(write=False)
    return ref, cmax


def _strict_stats(dfm, r):
    S = dfm.Stat
    return [S.V(), S.criterion(), S.eigenvalue(1), S.eigenvalue(r), S.coefficient(1), S.iterations()]


def test_strict_rule_both_forms_match_oracle():
    """A statistic that needs vectors solves under the strict rule: fp64 middle
    steps (LP = 0) with and without stored PF, no fp32 product.  V, ICp2 and
    the eigenvalues at 1e-10 relative; the coefficient (the intercept, which
    may be small) at 1e-10 of the refit's largest coefficient — the norm-wise
    bar of a least-squares solution."""
    T, r = 120, 8
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    ref, cmax = _strict_ref(T, r)
    for pf in (None, "0"):
        with _env("DFM_FACT_PF", pf):
            got, es = _boot(dfm, ctx, g, "wild", _strict_stats(dfm, r), idx, eta)
        assert es["gemm_products_f32"] == 0
        _check(got[:, :4], got[:, -1], ref[:, :4])
        cerr = np.abs(got[:, 4] - ref[:, 4]) / cmax
        print(f"DFM_FACT_PF={pf}: coefficient error / largest coefficient {cerr.max():.3e}")
        assert cerr.max() < 1e-10


def test_old_first_step_keeps_its_bits():
    """DFM_FACT_STEP0=1: the middle steps follow a Rayleigh-Ritz step (PV =
    P'D (Q Bm): no identity) and read stored PF whatever DFM_FACT_PF says."""
    T, r = 120, 8
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    out = []
    with _env("DFM_FACT_STEP0", "1"):
        for pf in (None, "0"):
            with _env("DFM_FACT_PF", pf):
                out.append(_boot(dfm, ctx, g, "wild", _stats(dfm, r), idx, eta))
    assert np.all(np.isfinite(out[0][0])) and np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


def test_new_path_shards_are_bit_identical(dfm, oracle):
    """As test_gpu_f32_filter.test_fp32_path_shards_are_bit_identical on the
    path without stored PF: whole, halves, the 8 slowest alone."""
    T, r, nrep = 120, 8, 96
    rng = np.random.default_rng(8300)
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    ctx = dfm.Context(0)
    g = dfm.DynamicFactorModel(y, np.ones((T, 1)), x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    idx, eta = dfm.draw_wild_fast(31, nrep, T)
    stats = _stats(dfm, r)
    with _env("DFM_FACT_PF", "0"):
        full = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
        assert np.all(np.isfinite(full)) and full[:, -1].min() >= 2
        lo = dfm.wild_bootstrap(g, 48, stats, idx=idx[:48], eta=eta[:48])
        hi = dfm.wild_bootstrap(g, 48, stats, idx=idx[48:], eta=eta[48:])
        slow = np.argsort(-full[:, -1], kind="stable")[:8]
        alone = dfm.wild_bootstrap(g, 8, stats, idx=idx[slow], eta=eta[slow])
    assert np.array_equal(full[:48, :-1], lo[:, :-1]) and np.array_equal(full[48:, :-1], hi[:, :-1])
    assert np.array_equal(full[slow, :-1], alone[:, :-1])


def test_new_path_two_lanes_are_bit_identical(dfm, oracle):
    """The case of test_gpu_f32_filter.test_fp32_path_two_lanes_are_bit_identical:
    600 replicates as two lanes and as one explicit batch."""
    T, r, nrep = 120, 8, 600
    rng = np.random.default_rng(8400)
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    ctx = dfm.Context(0)
    g = dfm.DynamicFactorModel(y, np.ones((T, 1)), x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    idx, eta = dfm.draw_wild_fast(41, nrep, T)
    stats = _stats(dfm, r)
    with _env("DFM_FACT_PF", "0"):
        lanes = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
        g.set_batch(nrep)
        one = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
    assert np.all(np.isfinite(lanes)) and np.array_equal(lanes[:, :-1], one[:, :-1])


def test_scale_factor_does_not_depend_on_the_panels_scale():
    """The r = 8 panel times 1e12: F = sqrt(T) U whatever the panel's scale,
    so PF from PV's rows needs no other factor.  The oracle's values at 1e-10."""
    T, r, scale = 120, 8, 1e12
    dfm, oracle, ctx, g, y, w, x = _model(T, r, scale)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    with _env("DFM_FACT_PF", "0"):
        got, es = _boot(dfm, ctx, g, "wild", _stats(dfm, r), idx, eta)
    assert es["gemm_products_f32"] > 0
    base = oracle.DynamicFactorModel(y, w, x, r, "ICp2")
    ref = np.empty((B, 2 + r))
    for b in range(B):
        d = oracle.DynamicFactorModel(y, w, base.common_component + eta[b][:, None] * base.factor_residuals[idx[b]],
                                      r, "ICp2")
        ref[b, 0] = oracle.factor_residual_variance(d)
        ref[b, 1] = d.number_of_factors_criterion_value
        ref[b, 2:] = d.eigenvalues[0][:r]
    _check(got[:, :-1], got[:, -1], ref)


# ---------------------------------------------------------------------- part B
def _probe_pair(T, r, stats_of, max_iter=None):
    """The same job with DFM_AP2_PROBE unset and =0: (rows, eig_stats) of each."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    if max_iter:
        ctx.set_eig_params(max_iter=max_iter)
    idx, eta = _draws(dfm, oracle, T, r, "wild")
    out = []
    for probe in (None, "0"):
        with _env("DFM_AP2_PROBE", probe):
            out.append(_boot(dfm, ctx, g, "wild", stats_of(dfm, r), idx, eta))
    return out


def _vector_stats(dfm, r):
    S = dfm.Stat
    return [S.V(), S.criterion(), S.eigenvalue(1), S.eigenvalue(r), S.coefficient(1), S.t_stat(1), S.iterations()]


def _same(on, off):
    assert np.all(np.isfinite(on[0]))
    print(f"iterations {np.unique(on[0][:, -1], return_counts=True)}")
    assert np.array_equal(on[0], off[0])   # the iteration column included
    assert on[1] == off[1], (on[1], off[1])   # eig_stats, field by field


@pytest.mark.parametrize("T,r", [(120, 8), (121, 4)])
@pytest.mark.parametrize("stats_of", [_stats, _vector_stats], ids=["eigenvalues", "vectors"])
def test_probe_changes_no_bit(T, r, stats_of):
    """Eigenvalue statistics (the eigenvalue rule, replicates that retire
    leave without vectors) and a job with a coefficient and a t-statistic (the
    strict rule, the U = Q A loop, fact_loadings).  At T = 120, r = 8
    replicates retire over several loop steps, so the second pass runs too."""
    on, off = _probe_pair(T, r, stats_of)
    assert on[0][:, -1].max() >= 3   # some replicate went on through a probed step (the first one is loop step 2)
    _same(on, off)


def test_probe_changes_no_bit_at_the_last_launch():
    """max_iter set to the slowest replicate's iteration count: that replicate
    retires at the launch that is also the last one allowed."""
    T, r = 120, 8
    _, its, _, _ = _case(T, r, "wild")
    on, off = _probe_pair(T, r, _stats, max_iter=int(its.max()))
    assert on[0][:, -1].max() == its.max()
    _same(on, off)
