"""CPU checks of the drop-in boundary: the C-ABI library loads and exports
every symbol include/dfm.h declares; host arithmetic entry points
(dfm_ic_sweep) agree with the oracle.  No device compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dfm.h")


def header_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfm_[a-z_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib(dfm):
    return dfm._lib.load()


def test_library_exports_every_header_symbol(lib):
    missing = [s for s in header_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_covers_header(dfm):
    assert sorted(dfm._lib.exported_symbols()) == header_symbols()


def test_ic_sweep_host_matches_oracle(lib, oracle):
    rng = np.random.default_rng(0)
    y, x, *_ = oracle.factor_model_DGP(120, 40, 2, rng)
    x = oracle.normalize(x)
    w = np.ones((120, 1))
    ev = np.linalg.eigvalsh(x.T @ x)[::-1].copy()
    out = np.zeros(7 * 6)
    rc = lib.dfm_ic_sweep(ev.ctypes.data_as(C.POINTER(C.c_double)), len(ev), 6, float(np.sum(x * x)),
                          120, 40, -1.0, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    ref = oracle.ic_sweep_values(y, w, x, 6)
    assert np.allclose(out.reshape(7, 6), ref, rtol=1e-11)


def test_ic_sweep_rejects_bad_args(lib):
    out = np.zeros(7)
    ev = np.ones(1)
    assert lib.dfm_ic_sweep(ev.ctypes.data_as(C.POINTER(C.c_double)), 1, 2, 1.0, 10, 10, 0.0,
                            out.ctypes.data_as(C.POINTER(C.c_double))) < 0


def test_context_creation_fails_cleanly_without_gpu(dfm):
    """A context on a device that is not there raises DFMError: device 0 on a
    host without a GPU, the first index past the visible ones on a host with
    some (whatever HIP_VISIBLE_DEVICES says, the count is the runtime's)."""
    import torch
    with pytest.raises(dfm.DFMError):
        dfm.Context(torch.cuda.device_count())


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dynamicfactormodels.jl_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "dfm_oracle" not in txt and "import oracle" not in txt, f
