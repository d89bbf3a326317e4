"""The factored bootstrap's warm solve without a first Rayleigh-Ritz step
(dfm_fact.hip eig_run_fact2_t: the degree-d0 filter runs on the warm start Q0
itself, with the interval end a constant of the base fit, and the first
Rayleigh-Ritz step comes after it).

Smallest shapes where that path can go wrong: T = 120, N = 300, B = 64 and
r = 4 (p = 8), r = 5 (odd r: the non-staged loaders, an odd block in an even
Z width), r = 8 (p = 12, the bench's block) and r = 13 (p = 17: the
32-column template, whose middle Horner step stages a Z chunk wider than its
PF rows); T = 121 for the Z / PV chunk pad rows.  Every replicate's V, ICp2
and top-r eigenvalues are held against the oracle's refit of the same draw
(src/bootstrap.jl:21-51) at 1e-10 relative, the project's bar.  Each case's
GPU rows and oracle rows are computed once and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-10
N, B = 300, 64


def _stats(dfm, r):
    S = dfm.Stat
    return [S.V(), S.criterion()] + [S.eigenvalue(j) for j in range(1, r + 1)] + [S.iterations()]


@functools.lru_cache(maxsize=None)
def _case(T, r, kind, step0=False, block=0):
    """(GPU rows without the iteration column, iterations, oracle rows, eig_stats) of one job."""
    import os
    import dfm_pkg
    import dfm_oracle as oracle
    dfm = dfm_pkg.load()
    rng = np.random.default_rng(8100 + 10 * r + (T - 120))
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    w = np.ones((T, 1))
    ctx = dfm.Context(0)
    if block:
        ctx.set_eig_params(block=block)
    g = dfm.DynamicFactorModel(y, w, x, r, "ICp2", ctx=ctx)
    g.set_bootstrap_mode("factored")
    assert g.fact_block()[0] == (block or max(r + 4, 8))
    base = oracle.DynamicFactorModel(y, w, x, r, "ICp2")
    if kind == "wild":
        idx, eta = dfm.draw_wild_fast(500 + r, B, T)
    else:
        idx, eta = oracle.draw_residual(np.random.default_rng(600 + r), B, T), None
    saved = os.environ.get("DFM_FACT_STEP0")
    if step0:
        os.environ["DFM_FACT_STEP0"] = "1"
    try:
        ctx.reset_timing()
        if kind == "wild":
            got = dfm.wild_bootstrap(g, B, _stats(dfm, r), idx=idx, eta=eta)
        else:
            got = dfm.residual_bootstrap(g, B, _stats(dfm, r), idx=idx)
        ctx.synchronize()
        es = ctx.eig_stats()
    finally:
        if step0:
            if saved is None:
                os.environ.pop("DFM_FACT_STEP0", None)
            else:
                os.environ["DFM_FACT_STEP0"] = saved
    ref = np.empty((B, 2 + r))
    for b in range(B):
        xs = base.common_component + (base.factor_residuals[idx[b]] if eta is None
                                      else eta[b][:, None] * base.factor_residuals[idx[b]])
        d = oracle.DynamicFactorModel(y, w, xs, r, "ICp2")
        ref[b, 0] = oracle.factor_residual_variance(d)
        ref[b, 1] = d.number_of_factors_criterion_value
        ref[b, 2:] = d.eigenvalues[0][:r]
    got.setflags(write=False)
    ref.setflags(write=False)
    return got[:, :-1], got[:, -1], ref, es


def _check(rows, its, ref):
    assert np.all(np.isfinite(rows))
    err = np.abs(rows - ref) / np.maximum(np.abs(ref), 1e-300)
    worst = np.unravel_index(np.argmax(err), err.shape)
    print(f"max rel err {err.max():.3e} at {worst}, iterations {np.unique(its, return_counts=True)}")
    assert err.max() < RTOL, (worst, err.max(), its[worst[0]])


CASES = [(120, 4, "wild"), (120, 5, "wild"), (120, 8, "wild"), (120, 13, "wild"), (120, 8, "residual"),
         (121, 8, "wild")]   # T = 121: an odd row count, 7 pad rows in the last 16-row chunk


@pytest.mark.parametrize("T,r,kind", CASES)
def test_every_replicate_matches_oracle(T, r, kind):
    rows, its, ref, _ = _case(T, r, kind)
    _check(rows, its, ref)


@pytest.mark.parametrize("T,r,kind", CASES)
def test_iterations_count_the_filter_step(T, r, kind):
    """Stat.iterations counts loop steps, the filter-only step included: a
    whole number >= 2.  replicate_iterations counts the Rayleigh-Ritz steps
    actually run (one fewer per replicate), gemm_products every H.Z
    replicate-product: at least the first filter's degree (>= 3 on this path)
    plus one per Rayleigh-Ritz step."""
    _, its, _, es = _case(T, r, kind)
    assert np.all(its == np.round(its)) and its.min() >= 2 and its.max() <= 400
    assert es["replicate_iterations"] == int(its.sum()) - B
    assert es["gemm_products"] >= 3 * B + es["replicate_iterations"]


def test_requested_block_of_32_columns():
    """dfm_ctx_set_eig_params block = 32 with r = 4: 28 guard columns, the
    most the guard orthonormalisation can meet (its Gram matrix has 28 x 28
    sums, the widest block 31 x 31), on the 32-column template."""
    rows, its, ref, es = _case(120, 4, "wild", False, 32)
    _check(rows, its, ref)
    assert np.all(its == np.round(its)) and its.min() >= 2
    assert es["replicate_iterations"] == int(its.sum()) - B


def test_old_first_step_still_matches_oracle():
    """DFM_FACT_STEP0=1 restores the Rayleigh-Ritz step in front of the first
    filter — the schedule cold starts still run through the same kernels."""
    rows, its, ref, es = _case(120, 8, "wild", True)
    _check(rows, its, ref)
    assert np.all(its == np.round(its)) and its.min() >= 1
    assert es["replicate_iterations"] == int(its.sum())   # every loop step is a Rayleigh-Ritz step there


def test_shards_are_bit_identical(dfm, oracle):
    """A 96-replicate job whole, as replicates 0-47 and 48-95, and with its 8
    slowest replicates alone: the interval end and the warm start depend on
    the model only, so every row is the same to the bit (iteration column
    excluded, as in test_gpu_compaction.py)."""
    T, r, nrep = 120, 8, 96
    rng = np.random.default_rng(8300)
    y, x, *_ = oracle.factor_model_DGP(T, N, r, rng)
    x = oracle.normalize(x)
    g = dfm.DynamicFactorModel(y, np.ones((T, 1)), x, r, "ICp2")
    g.set_bootstrap_mode("factored")
    idx, eta = dfm.draw_wild_fast(31, nrep, T)
    stats = _stats(dfm, r)
    full = dfm.wild_bootstrap(g, nrep, stats, idx=idx, eta=eta)
    assert np.all(np.isfinite(full)) and full[:, -1].min() >= 2
    lo = dfm.wild_bootstrap(g, 48, stats, idx=idx[:48], eta=eta[:48])
    hi = dfm.wild_bootstrap(g, 48, stats, idx=idx[48:], eta=eta[48:])
    assert np.array_equal(full[:48, :-1], lo[:, :-1]) and np.array_equal(full[48:, :-1], hi[:, :-1])
    slow = np.argsort(-full[:, -1], kind="stable")[:8]
    alone = dfm.wild_bootstrap(g, 8, stats, idx=idx[slow], eta=eta[slow])
    assert np.array_equal(full[slow, :-1], alone[:, :-1])
