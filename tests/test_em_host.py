"""CPU checks around the EM fit for panels with missing observations: the
NumPy restatement the GPU tests compare against (tests/em_reference.py), the
CSV loader's missing="nan" mode, and the C ABI's declarations and bindings."""
import os
import re

import numpy as np
import pytest

import em_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dfm.h")
ENTRY_POINTS = {"dfm_em": 14, "dfm_model_fit_em": 12, "dfm_model_em_read": 4}


@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"{T}x{N}" for T, N in R.SHAPES])
def test_reference_error_sequence_decreases(shape):
    ref = R.cached(*shape)
    errs = ref["errs"]
    assert ref["converged"] and len(errs) == ref["iterations"] >= 2
    assert all(a > b for a, b in zip(errs, errs[1:]))
    # the iteration-count assertion of tests/test_gpu_em.py needs the final err clear of tol
    assert errs[-1] < 0.99e-6 and errs[-2] > 1.01e-6


@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"{T}x{N}" for T, N in R.SHAPES])
def test_reference_fixed_point(shape):
    """One more step from a converged completed panel moves C by at most tol."""
    X, _ = R.make_panel(*shape)
    ref = R.cached(*shape)
    nxt = R.em_step(X, ref["C"], ref["mu"], ref["sd"], R.R_TRUE)
    assert nxt["err"] <= 1e-6
    assert nxt["err"] < ref["err"]


def test_reference_panels_have_the_stated_pattern():
    for T, N in R.SHAPES:
        X, full = R.make_panel(T, N)
        miss = np.isnan(X)
        assert not miss[:, 1].any()
        assert miss[T - 6:, ::5][:, np.arange(0, N, 5) != 1].all()
        assert miss[:6, 2::7].all()
        assert miss[T // 2, [j for j in range(N) if j % 3 and j != 1]].all()
        assert np.array_equal(X[~miss], full[~miss])
        assert (~miss).sum(axis=0).min() >= 2
        assert 0.15 < miss.mean() < 0.35


def test_read_panel_csv_missing(dfm, tmp_path):
    p = tmp_path / "panel.csv"
    p.write_text("date,a,b,c\n2001-01,1.5,,3\n2001-02,NA,2.25,NaN\n2001-03,4,5,6\n")
    with pytest.raises(ValueError, match="missing value in column 'b', row 2"):
        dfm.read_panel_csv(str(p))
    names, data = dfm.read_panel_csv(str(p), missing="nan")
    assert names == ["a", "b", "c"]
    want = np.array([[1.5, np.nan, 3.0], [np.nan, 2.25, np.nan], [4.0, 5.0, 6.0]])
    assert np.array_equal(data, want, equal_nan=True)
    with pytest.raises(ValueError):
        dfm.read_panel_csv(str(p), missing="zero")


def test_abi_declares_and_binds_the_em_entry_points(dfm):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    bound = {s[0]: s for s in dfm._lib.SIGNATURES}
    for name, arity in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/dfm.h"
        assert len(decl.group(1).split(",")) == arity
        assert name in bound, f"{name} is not bound in _lib.py"
        assert len(bound[name][2]) == arity
    for struct, fields in (("dfm_em_spec", ["r", "crit", "kmax", "standardize", "max_iter", "dev", "tol"]),
                           ("dfm_em_info", ["iterations", "converged", "r", "pad", "err", "n_missing"])):
        assert re.search(r"}\s*" + struct + r"\s*;", src), struct
        assert [f[0] for f in getattr(dfm._lib, struct)._fields_] == fields
    import ctypes
    assert ctypes.sizeof(dfm._lib.dfm_em_spec) == 32 and ctypes.sizeof(dfm._lib.dfm_em_info) == 32
