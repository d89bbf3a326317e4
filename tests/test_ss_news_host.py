"""The news decomposition without a device: the two references of
tests/ss_news_reference.py against each other, the identity a|new - a|rev =
sum_j I_j c^j_t|T, and the new entry point's export.

Route (a) conditions the joint Gaussian and uses no Kalman recursion; route (b)
restates the header's recursion.  Both are double-precision NumPy on problems
whose solves are conditioned like 1e3 or better, so they agree to about 1e-13;
the bar here is 1e-11 of the reference array's largest magnitude, an order
below the device tests' 1e-10, so that route (a) can stand as their reference."""
import numpy as np
import pytest

import ss_news_reference as R

RTOL = 1e-11
SMALLEST = (4, 2, 0)   # 30 x 6, 30 x 9, 36 x 10 of ss_mf_reference.CASES


def big(a):
    return float(np.max(np.abs(a)))


@pytest.mark.parametrize("i", range(R.N_CASES), ids=R.CASE_IDS)
def test_recursion_weights_are_the_textbook_weights(i):
    inp, ref = R.case(i)
    rec = R.recursion(*inp, horizon=R.HORIZON)
    assert np.array_equal(rec["releases"], ref["releases"]) and len(ref["releases"]) >= 9
    fig = {"state": big(rec["weights_state"] - ref["weights_state"]) / big(ref["weights_state"]),
           "f": big(rec["weights_f"] - ref["weights_f"]) / big(ref["weights_f"])}
    if ref["weights_agg"] is not None:
        fig["agg"] = big(rec["weights_agg"] - ref["weights_agg"]) / big(ref["weights_agg"])
    print(R.CASE_IDS[i], " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < RTOL, (k, v)


@pytest.mark.parametrize("i", SMALLEST, ids=[R.CASE_IDS[i] for i in SMALLEST])
def test_news_times_weights_is_the_move_of_the_smoothed_state(i):
    """a|new conditioned directly on the new vintage against a|rev + sum_j I_j
    c^j, the weights by the recursion: every row, the forecast rows included."""
    inp, ref = R.case(i)
    Xo, Xn = inp[0], inp[1]
    a_new = R.smooth_dense(Xn, *inp[2:], horizon=R.HORIZON)
    a_rev = R.smooth_dense(R.revised(Xo, Xn), *inp[2:], horizon=R.HORIZON)
    W = R.recursion(*inp, horizon=R.HORIZON)["weights_state"]
    res = big(a_new - a_rev - np.einsum("j,jts->ts", ref["news"], W)) / big(a_new)
    print(R.CASE_IDS[i], f"identity={res:.2e}", f"move={big(a_new - a_rev) / big(a_new):.2e}")
    assert res < RTOL
    assert big(a_new - a_rev) > 1e-3 * big(a_new)   # the releases do move the path
    assert big(a_rev - ref["state_rev"]) < RTOL * big(a_rev)


def test_single_release_and_revisions():
    """J = 1 (the row-0 release): the weights are one impulse response, and the
    two revised values move a|old to a|rev."""
    inp, ref = R.case(0, True)
    assert len(ref["releases"]) == 1 and ref["releases"][0, 0] == 0
    rec = R.recursion(*inp, horizon=R.HORIZON)
    assert big(rec["weights_state"] - ref["weights_state"]) < RTOL * big(ref["weights_state"])
    assert big(ref["state_rev"] - ref["state_old"]) > 1e-3 * big(ref["state_old"])


def test_new_symbol_is_exported_and_bound(dfm):
    lib = dfm._lib.load()
    assert hasattr(lib, "dfm_ss_news") and "dfm_ss_news" in dfm._lib.exported_symbols()
    assert callable(dfm.nowcast_news) and dfm.NewsResult is not None
