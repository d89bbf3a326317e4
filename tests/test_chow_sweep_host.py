"""CPU checks of the sup-Chow host layer: the Stat constructors of the
DFM_STAT_SUP*_ALL kinds, the default trimmed range of candidate break periods
and the bootstrap p-value arithmetic.  No device compute."""
import math

import numpy as np
import pytest


def test_sup_stat_structs_carry_kind_and_range(dfm):
    S = dfm.Stat
    for kind, make in [(15, S.supLR_all), (16, S.supLM_all), (17, S.supWald_all)]:
        s = make(12, 47)
        assert (s.kind, s.arg0, s.arg1) == (kind, 12, 47)
    arr = dfm.api._stat_array([S.supLM_all(3, 9), S.LM_all(5)])
    assert (arr[0].kind, arr[0].arg0, arr[0].arg1, arr[0].pad) == (16, 3, 9, 0)
    assert (arr[1].kind, arr[1].arg0) == (10, 5)


def test_header_declares_the_sup_kinds():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dfm.h")).read()
    for name, val in [("DFM_STAT_SUPLR_ALL", 15), ("DFM_STAT_SUPLM_ALL", 16), ("DFM_STAT_SUPWALD_ALL", 17)]:
        assert re.search(rf"{name}\s*=\s*{val}\b", hdr), name


@pytest.mark.parametrize("T,r,trim,want", [
    (83, 1, 0.15, (13, 70)),      # ceil(12.45) = 13, floor(70.55) = 70
    (90, 3, 0.15, (14, 76)),      # ceil(13.5), floor(76.5)
    (50, 5, 0.15, (10, 40)),      # 2 r = 10 > ceil(7.5) = 8; T - 2 r = 40 < floor(42.5)
    (70, 10, 0.15, (20, 50)),     # both ends from 2 r
    (600, 3, 0.15, (90, 510)),
    (100, 2, 0.10, (10, 90)),
    (100, 2, 0.0, (4, 96)),
])
def test_default_range(dfm, T, r, trim, want):
    assert dfm.sup_chow_range(T, r, trim) == want
    lo, hi = dfm.sup_chow_range(T, r, trim)
    assert lo == max(math.ceil(trim * T), 2 * r) and hi == min(math.floor((1 - trim) * T), T - 2 * r)
    assert dfm.sup_chow_range(T, r, trim, lo=17) == (17, want[1])
    assert dfm.sup_chow_range(T, r, trim, hi=33) == (want[0], 33)
    assert dfm.sup_chow_range(T, r, trim, 21, 22) == (21, 22)


def test_sup_chow_pvalues_with_ties(dfm):
    obs = np.array([2.0, 5.0, 0.5, 3.0])
    reps = np.array([[1.0, 5.0, 0.6, 3.0],
                     [2.0, 4.0, 0.7, 3.0],      # ties count as >= (columns 0, 3)
                     [3.0, 6.0, 0.8, 2.999999],
                     [2.0, 5.0, 0.9, 3.0],
                     [0.0, 7.0, 1.0, np.inf]])
    p = dfm.sup_chow_pvalues(obs, reps)
    assert p.shape == (4,)
    assert np.array_equal(p, np.array([3 / 5, 4 / 5, 1.0, 4 / 5]))
    assert np.array_equal(dfm.sup_chow_pvalues([10.0], [[1.0], [2.0]]), [0.0])
    with pytest.raises(ValueError):
        dfm.sup_chow_pvalues(obs, reps[:, :3])
    with pytest.raises(ValueError):
        dfm.sup_chow_pvalues(obs, reps[0])
