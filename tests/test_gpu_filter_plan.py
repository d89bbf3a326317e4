"""The first filter's precision rule as one table (dfm_fact_plan.h
plan_first_filter): which of a warm eigenvalue-rule solve's H.Z products run
in fp64, in fp32 or as six bf16 terms under DFM_FACT_F32, DFM_FACT_SPLIT and
DFM_FACT_SPLIT_LAST.  The test states the rule, not how the solver encodes it.

All eight settings of the three switches in {unset, "0"} fall into four
classes:

  1  F32=0                       fp64 throughout
  2  F32 on, SPLIT=0             fp32 middle products
  3  both on, SPLIT_LAST=0       split middle products, fp64 last product
  4  none set                    all split

Settings of one class must agree to the byte in rows, iterations and every
counter; the fp32 count is 0 for class 1 and (d0 - 1) B otherwise; the
split-last count is B for class 4 only; one job of each class meets the
oracle at 1e-10.

Shapes (tests/test_gpu_warm_filter.py, N = 300, B = 64): (121, 8) has pad rows
in Z's last chunk, so the zero-fill behind a split last product runs, and the
staged loaders; (120, 5) an odd r, the non-staged loaders; (120, 13) the
32-column instances at pz = 18.  The oracle rows are the cached ones of
test_gpu_warm_filter._case.
"""
import contextlib
import functools
import itertools

import numpy as np
import pytest

from test_gpu_f32_filter import _base_d0, _boot, _draws, _env, _model
from test_gpu_warm_filter import _case, _check, _stats, B

pytestmark = pytest.mark.gpu

SHAPES = [(121, 8, "wild"), (120, 5, "wild"), (120, 13, "wild")]
SWITCHES = ("DFM_FACT_F32", "DFM_FACT_SPLIT", "DFM_FACT_SPLIT_LAST")
SETTINGS = list(itertools.product((None, "0"), repeat=3))


def _class(setting):
    f32, split, split_last = setting
    if f32 == "0":
        return 1
    if split == "0":
        return 2
    if split_last == "0":
        return 3
    return 4


@functools.lru_cache(maxsize=None)
def _jobs(T, r, kind):
    """{setting: (rows with the iteration column, eig_stats)} of one shape: one
    model, one set of draws, eight jobs."""
    dfm, oracle, ctx, g, *_ = _model(T, r)
    idx, eta = _draws(dfm, oracle, T, r, kind)
    out = {}
    for setting in SETTINGS:
        with contextlib.ExitStack() as stack:
            for name, value in zip(SWITCHES, setting):
                stack.enter_context(_env(name, value))
            got, es = _boot(dfm, ctx, g, kind, _stats(dfm, r), idx, eta)
        got.setflags(write=False)
        out[setting] = (got, dict(es))
    return out


def test_the_settings_form_four_classes():
    assert sorted(_class(s) for s in SETTINGS) == [1, 1, 1, 1, 2, 2, 3, 4]


@pytest.mark.parametrize("T,r,kind", SHAPES)
def test_settings_of_one_class_agree_to_the_byte(T, r, kind):
    jobs = _jobs(T, r, kind)
    for cls in (1, 2, 3, 4):
        members = [s for s in SETTINGS if _class(s) == cls]
        rows0, es0 = jobs[members[0]]
        assert np.all(np.isfinite(rows0))
        for s in members[1:]:
            rows, es = jobs[s]
            assert rows.tobytes() == rows0.tobytes(), (cls, s)
            assert es == es0, (cls, s, es, es0)


@pytest.mark.parametrize("T,r,kind", SHAPES)
def test_counters_follow_the_class(T, r, kind):
    d0 = _base_d0(T, r)
    assert d0 >= 3
    jobs = _jobs(T, r, kind)
    for s in SETTINGS:
        es = jobs[s][1]
        cls = _class(s)
        print(f"{s}: class {cls}, f32 {es['gemm_products_f32']}, split_last {es['gemm_products_split_last']}")
        assert es["gemm_products_f32"] == (0 if cls == 1 else (d0 - 1) * B), s
        assert es["gemm_products_split_last"] == (B if cls == 4 else 0), s


@pytest.mark.parametrize("T,r,kind", SHAPES)
@pytest.mark.parametrize("cls", [1, 2, 3, 4])
def test_each_class_matches_the_oracle(T, r, kind, cls):
    ref = _case(T, r, kind)[2]
    rep = next(s for s in SETTINGS if _class(s) == cls)
    got = _jobs(T, r, kind)[rep][0]
    _check(got[:, :-1], got[:, -1], ref)
