"""The checkers of tests/eig_reference.py on the CPU: each is fed the exact
answer with one of the faults an eigensolver can have and must reject it, and
must accept the exact answer and LAPACK's.  This is the evidence that
tests/test_gpu_eig.py fails on a subtly wrong solver, without a wrong solver
in the library."""
import numpy as np
import pytest
import scipy.linalg as sla

import eig_reference as R

M, K = 65, 8
P = R.block_p(M, K)
TOL = 1e-14


def _canon(U):
    U = np.array(U, dtype=np.float64)
    for j in range(U.shape[1]):
        if U[np.argmax(np.abs(U[:, j])), j] < 0:
            U[:, j] = -U[:, j]
    return U


def _exact(fam="b", m=M, k=K):
    case = R.make_case(fam, m, k, R.block_p(m, k))
    return case, case.lam[:k].astype(np.float64), _canon(case.V[:, :k]), float(case.trace)


def _verify(case, lam, U, tr, tol=TOL, subspace=0, status=0, k=K, p=P):
    return R.verify(case, k, p, lam, U, tr, status, tol, subspace, iters=5, maxit=400)


def _rejected(fn, *a, **kw):
    with pytest.raises(AssertionError) as e:
        fn(*a, **kw)
    return str(e.value)


def test_spectra_are_what_they_claim():
    """Every family at a few sizes: G is symmetric, G V = V diag(lam) to longdouble rounding, V'V = I, the ties
    are where the family puts them, and LAPACK finds the same values."""
    for m, k in [(5, 4), (17, 8), (65, 16), (144, 15), (257, 24), (300, 16), (16, 16), (3, 1), (1, 1)]:
        p = R.block_p(m, k)
        for fam in (R.EXACT_FAMILIES + R.ROUNDED_FAMILIES) if m < 200 else ["a", "c", "g"]:
            case = R.make_case(fam, m, k, p)
            if case is None:
                continue
            G, V, L = case.G.astype(R.LD), case.V, case.lam
            assert np.array_equal(case.G, case.G.T)
            scale = max(float(abs(L[0])), 1e-300)
            tol = 4 * 2.0 ** -63 if case.tie == 0 else m * 2.0 ** -50
            assert float(np.abs(G @ V - V * L).max()) <= tol * m * scale, case.name
            assert float(np.abs(V.T @ V - np.eye(m)).max()) <= max(tol, 2.0 ** -60) * m, case.name
            assert np.all(np.diff(L.astype(np.float64)) <= 0)
            w = sla.eigvalsh(case.G)[::-1]
            assert np.abs(w - L.astype(np.float64)).max() <= m * 2.0 ** -50 * scale, case.name
    L = R.make_case("b", 65, 8, 16).lam
    assert L[1] == L[2] and L[3] == L[4] == L[5] and L[0] > L[1] and L[2] > L[3] and L[5] > L[6]
    L = R.make_case("c", 65, 8, 16).lam
    assert L[7] == L[8] == L[9] and L[6] > L[7] and L[9] > L[10]
    L = R.make_case("d", 65, 8, 16).lam
    assert L[7] == L[17] and L[17] > L[18] and L[6] > L[7]
    L = R.make_case("e", 65, 8, 16).lam
    assert L[5] > 0 and L[6] == 0
    L = R.make_case("f", 65, 8, 16).lam
    assert L[11] > 0 and L[12] == 0
    assert not R.make_case("z", 65, 8, 16).G.any()
    assert R.make_case("a+", 17, 4, 16).lam[0] == 2.0 ** 100 and R.make_case("a-", 17, 4, 16).lam[0] == 2.0 ** -100


@pytest.mark.parametrize("fam", R.EXACT_FAMILIES + ["g"])
def test_exact_answers_pass(fam):
    case, lam, U, tr = _exact(fam)
    for subspace in (0, 1):
        out = _verify(case, lam, U, tr, subspace=subspace)
        assert out["always"] <= 1.0 and out["orth"] < 1e-14
    out = R.verify(case, K, P, lam, None, tr, 0, -1e-12, 0, iters=3, maxit=400)
    assert out["values"] < 0.1
    # not converged: only the "always" checks, and iters must be maxit
    R.verify(case, K, P, lam, U, tr, 1, TOL, 0, iters=400, maxit=400)
    assert "iters" in _rejected(R.verify, case, K, P, lam, U, tr, 1, TOL, 0, iters=0, maxit=400)


def test_lapack_passes_on_a_rounded_cluster():
    """dsyevr's own vectors of the (h) cluster: every check but the cluster's subspace (it crosses k)."""
    case = R.make_case("h", M, K, P)
    _verify(case, case.lam[:K].astype(np.float64), _canon(case.V[:, :K]), float(case.trace))
    assert R.lapack_orthonormality(case, K) < 1e-13


def test_rotated_vector():
    """Column 0 rotated 1e-9 towards the last eigenvector: the strict residual bound rejects it."""
    case, lam, U, tr = _exact()
    U[:, 0] = _canon((case.V[:, 0] + 1e-9 * case.V[:, M - 1])[:, None])[:, 0]
    assert "|r_0|" in _rejected(_verify, case, lam, U, tr)
    # inside the tied pair a rotation stays in the eigenspace and passes
    case, lam, U, tr = _exact()
    c, s = np.cos(0.3), np.sin(0.3)
    U[:, 1], U[:, 2] = _canon((c * case.V[:, 1] + s * case.V[:, 2])[:, None])[:, 0], \
        _canon((c * case.V[:, 2] - s * case.V[:, 1])[:, None])[:, 0]
    _verify(case, lam, U, tr)


def test_vector_from_the_wrong_eigenspace():
    """Column 0 replaced by the (k+1)-th eigenvector.  With lam kept the residual rejects it (Davis-Kahan is a
    theorem: given that residual it allows the angle, so the subspace check alone does not); with its own
    eigenvalue beside it the pair is exact, and the subspace check rejects it for lying outside the cluster."""
    case, lam, U, tr = _exact()
    U[:, 0] = _canon(case.V[:, 8:9])[:, 0]
    assert "|r_0|" in _rejected(R.check_strict, case, K, P, lam, U, TOL, 0)
    _rejected(_verify, case, lam, U, tr)
    lam[0] = float(case.lam[8])
    assert "from its cluster" in _rejected(R.check_subspace, case, K, lam, U)


def test_tied_columns_not_orthogonal():
    case, lam, U, tr = _exact()
    U[:, 2] = U[:, 2] + 1e-9 * U[:, 1]
    assert "U'U" in _rejected(_verify, case, lam, U, tr)
    assert R.check_strict(case, K, P, lam, U, TOL, 0) <= 1.0   # (the residuals alone do not see it)


def test_swapped_eigenvalues():
    case, lam, U, tr = _exact("a")
    lam[[3, 4]] = lam[[4, 3]]
    assert "increases" in _rejected(_verify, case, lam, U, tr)


def test_value_from_outside_the_wanted_set():
    """lam_{k-1} replaced by the (k+1)-th value: still sorted, still an eigenvalue."""
    case, lam, U, tr = _exact("a")
    lam[K - 1] = float(case.lam[K])
    assert "lam[7]" in _rejected(R.check_values, case, K, lam, -1e-12)
    _rejected(_verify, case, lam, U, tr)
    _rejected(R.verify, case, K, P, lam, None, tr, 0, -1e-12, 0)


def test_flipped_sign():
    case, lam, U, tr = _exact("e")   # the diagonal part's unit vectors: a clear largest entry
    assert R.check_signs(case, U) >= 1
    j = next(j for j in range(K) if np.sort(np.abs(U[:, j]))[-1] - np.sort(np.abs(U[:, j]))[-2] > 0.1)
    U[:, j] = -U[:, j]
    assert "not positive" in _rejected(_verify, case, lam, U, tr)


def test_stray_write_and_unwritten_column():
    case, lam, U, tr = _exact()
    nb, guard = 3, 64
    buf = np.full(nb * M * K + guard, np.nan)
    buf[:nb * M * K] = np.tile(U.ravel(), nb)
    R.check_extent(buf, nb * M * K, case, "Uk")
    bad = buf.copy()
    bad[nb * M * K] = 0.0
    assert "past its extent" in _rejected(R.check_extent, bad, nb * M * K, case, "Uk")
    bad = buf.copy()
    bad[:nb * M * K].reshape(nb, M, K)[1, :, 5] = np.nan
    assert "never written" in _rejected(R.check_extent, bad, nb * M * K, case, "Uk")
    Ub = U.copy()
    Ub[:, 5] = np.nan
    assert "not finite" in _rejected(_verify, case, lam, Ub, tr)


def test_trace_missing_a_term():
    case, lam, U, tr = _exact()
    assert "trace" in _rejected(_verify, case, lam, U, tr - float(case.G[M - 1, M - 1]))
    case, lam, U, tr = _exact("a-")
    assert "trace" in _rejected(_verify, case, lam, U, tr - float(case.G[3, 3]))
