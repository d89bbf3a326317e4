"""The reference of the factor blocks (tests/ss_blocks_reference.py) checked on
the CPU: the log-likelihood rises on every case, one all-member block is the
unrestricted reference, the restricted M-step is a maximum of the expected
complete-data log-likelihood over the feasible set, and the panels the device
tests rely on have the margins they are chosen for (the stopping rule's
margins of the batch, the eigengaps of the fit's principal components)."""
import numpy as np
import pytest

import ss_blocks_reference as R
import ss_em_reference as EM
import ss_mf_reference as MF


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_the_reference_path_rises_and_keeps_the_zeros(i):
    T, N, sizes, p, w, mixed, everyone = R.CASES[i]
    X, start, low, member, ref = R.em_case(i)
    gains = np.diff(ref["path"])
    print(R.CASE_IDS[i], "gains", gains)
    assert len(ref["path"]) == R.EM_ITER + 1 and (gains > 0).all()
    assert (ref["L"][~R.free_matrix(sizes, member)] == 0.0).all()
    assert (ref["A"][~R.same_block(sizes, p)] == 0.0).all() and (ref["Q"][~R.same_block(sizes)] == 0.0).all()
    assert (ref["sigma2"] > 0).all() and np.linalg.eigvalsh(ref["Q"]).min() > 0
    # the start holds zeros where the restriction does
    assert (start[0][~R.free_matrix(sizes, member)] == 0.0).all() and (start[2][~R.same_block(sizes, p)] == 0.0).all()


def test_the_unrestricted_estimator_differs_visibly():
    T, N, sizes, p, w, _, _ = R.CASES[0]
    X, start, low, member, ref = R.em_case(0)
    free = MF.em(X, *start, low, w, tol=0.0, max_iter=R.EM_ITER)
    assert np.abs(free["L"][~R.free_matrix(sizes, member)]).max() > 0.1
    assert free["path"][-1] > ref["path"][-1]   # the larger model fits at least as well from the same start


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mf"])
def test_one_all_member_block_is_the_unrestricted_reference(mixed):
    i = 0 if mixed else 4
    T, N, sizes, p, w, _, _ = R.CASES[i]
    X, start, low, _ = R.start_of(i)
    r = sum(sizes)
    one = R.em(X, *start, (r,), R.all_members(N, (r,)), low, w, tol=0.0, max_iter=3, horizon=2)
    old = MF.em(X, *start, low, w, tol=0.0, max_iter=3, horizon=2) if mixed else \
        EM.em(X, *start, tol=0.0, max_iter=3, horizon=2)
    for k in ("L", "sigma2", "A", "Q", "a0", "P0", "path", "filtered", "smoothed", "smoothed_cov"):
        assert np.max(np.abs(one[k] - old[k])) <= 1e-12 * np.max(np.abs(old[k])), k


@pytest.mark.parametrize("i", [0, 1, 4], ids=[R.CASE_IDS[k] for k in (0, 1, 4)])
def test_the_restricted_m_step_beats_feasible_perturbations(i):
    T, N, sizes, p, w, mixed, _ = R.CASES[i]
    X, start, low, member = R.start_of(i)
    L0, sg0, A0, Q0 = start
    r = sum(sizes)
    s = r * MF.lags(p, w if mixed else R.PLAIN_W)
    a0 = np.zeros(s)
    import ss_reference as S
    P0 = S.stationary_kron(MF.padded_A(A0, s // r), Q0)
    ww = w if mixed else R.PLAIN_W
    es = MF.e_step(X, L0, sg0, A0, Q0, low, ww, a0, P0)
    L, sigma2, A, Q, _, _ = R.m_step(X, es, sizes, member, low, ww, p, True, a0, P0)
    best = R.expected_loglik(X, es, low, ww, L, sigma2, A, Q)
    free, inside = R.free_matrix(sizes, member), R.same_block(sizes, p)
    rng = np.random.Generator(np.random.PCG64(41 + i))
    for _ in range(10):
        dL = 0.05 * rng.standard_normal(L.shape) * free
        dA = 0.05 * rng.standard_normal(A.shape) * inside
        assert R.expected_loglik(X, es, low, ww, L + dL, sigma2, A, Q) < best
        assert R.expected_loglik(X, es, low, ww, L, sigma2, A + dA, Q) < best
    # and an infeasible move can do better: the restriction binds
    Lu, _, Au, Qu, _, _ = MF.m_step(X, es, low, ww, p, True, a0, P0)
    assert R.expected_loglik(X, es, low, ww, Lu, sigma2, A, Q) > best


def test_the_batch_stops_at_different_times_with_safe_margins():
    its = [R.batch_case(k)[4]["iterations"] for k in range(len(R.BATCH_SEEDS))]
    margins = R.batch_margins()
    print("iterations", its, "smallest margin", margins.min())
    assert len(set(its)) > 1 and all(R.batch_case(k)[4]["converged"] for k in range(len(R.BATCH_SEEDS)))
    assert margins.min() >= 0.02


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mf"])
@pytest.mark.parametrize("sizes", R.FIT_SIZES, ids=["b111", "b211"])
def test_the_fit_panels_have_their_eigengaps_and_the_chain_rises(sizes, mixed):
    two = R.fit_case(sizes, mixed, "two-step")
    ml = R.fit_case(sizes, mixed, "ml")
    print(sizes, mixed, "eigengaps", two["gaps"])
    assert two["gaps"].min() >= 0.3
    assert (np.diff(ml["res"]["path"]) > 0).all()
    member = two["member"]
    assert (ml["L"][~R.free_matrix(sizes, member)] == 0.0).all()
    # the start's loadings are dfm_pca's at T >= the members' count: L_g'L_g / n_g = I on the members' rows
    off = R.offsets(sizes)
    for g in range(len(sizes)):
        Lg = two["start_L"][member[:, g], off[g]:off[g + 1]]
        assert np.allclose(Lg.T @ Lg / Lg.shape[0], np.eye(Lg.shape[1]), atol=1e-12)


def test_python_checks_come_before_the_device(dfm):
    N = 6
    with pytest.raises(ValueError):
        dfm.api._ss_blocks(None, np.ones((N, 1)), N)
    with pytest.raises(ValueError):
        dfm.api._ss_blocks((1.5, 1), None, N)
    with pytest.raises(dfm.DFMError) as e:
        dfm.api._ss_blocks((1, 2), None, N, 4)
    assert e.value.code == -2 and "sum" in str(e.value)
    with pytest.raises(dfm.DFMError):
        dfm.api._ss_blocks((1, 1), np.ones((N, 3), dtype=bool), N)
    with pytest.raises(ValueError):
        dfm.api._ss_blocks((1, 1), np.ones((N, 2)) * 0.5, N)
    sizes, mem = dfm.api._ss_blocks((2, 1), None, N, 3)
    assert sizes.dtype == np.int32 and mem.dtype == np.uint8 and mem.flags.f_contiguous and mem.all()
    sizes, mem = dfm.api._ss_blocks([1, 1], np.array([[1, 0]] * N), N)
    assert mem[:, 0].all() and not mem[:, 1].any()
