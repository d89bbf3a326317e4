"""CPU checks of the Monte-Carlo batch's host side: dfm_mc_stats_width (pure
arithmetic through the library, no device) and host.replicate_table, the
table of the reference's driver script (src/Bai_Ng.jl:12-39), with the
selection done by the oracle."""
import numpy as np
import pytest


def width(dfm, N, stats):
    lib = dfm._lib.load()
    return int(lib.dfm_mc_stats_width(N, dfm.api._stat_array(stats), len(stats)))


def test_stats_width(dfm):
    S = dfm.Stat
    N = 37
    assert width(dfm, N, [S.V()]) == 1
    assert width(dfm, N, [S.LR_all(9)]) == N
    assert width(dfm, N, [S.supLR_all(9, 20), S.supLM_all(9, 20), S.supWald_all(9, 20)]) == 3 * N
    mixed = [S.V(), S.criterion("PCp1"), S.eigenvalue(2), S.trace(), S.LR(9, 3), S.LM(9, 3), S.Wald(9, 3),
             S.LM_all(9), S.Wald_all(9), S.supLM_all(9, 20)]
    assert width(dfm, N, mixed) == 7 + 3 * N
    assert width(dfm, N, []) == 0
    for bad in (S.coefficient(1), S.t_stat(1), S.iterations(), S.factors(), S.loadings()):
        assert width(dfm, N, [bad]) < 0
        assert width(dfm, N, [S.V(), bad]) < 0
    assert width(dfm, 0, [S.V()]) < 0


def oracle_select(oracle, calls):
    def select(panels):
        calls.append([p.copy() for p in panels])
        out = {name: [] for name in oracle.CRITERIA}
        for x in panels:
            T, N = x.shape
            kmax = int(np.ceil(min(T, N) / 2))
            ic = oracle.ic_sweep_values(np.zeros(T), np.ones((T, 1)), oracle.normalize(x), kmax)
            for name, row in zip(oracle.CRITERIA, ic):
                out[name].append(int(np.argmin(row)) + 1)
        return out
    return select


def test_replicate_table(dfm, oracle):
    tuples = [(40, 12, 1), (30, 16, 2), (24, 30, 3)]
    reps = 3
    criteria = ("PCp1", "ICp2", "BIC")
    calls = []
    table = dfm.replicate_table(tuples, reps, np.random.default_rng(11), criteria=criteria,
                                select=oracle_select(oracle, calls))
    assert table.shape == (len(tuples), len(criteria))
    # the draws: factor_model_DGP on the passed generator, tuple by tuple, repetition by repetition,
    # ONE draw per repetition (not one per criterion)
    rng = np.random.default_rng(11)
    assert len(calls) == len(tuples)
    for (T, N, r), got in zip(tuples, calls):
        assert len(got) == reps
        for x in got:
            assert np.array_equal(x, dfm.factor_model_DGP(T, N, r, rng=rng)[1])
    # the entries: means over the repetitions of the selected factor counts
    sel = oracle_select(oracle, [])
    for i, got in enumerate(calls):
        chosen = sel(got)
        for j, name in enumerate(criteria):
            assert table[i, j] == np.mean(chosen[name])
    assert np.all(table >= 1) and len(np.unique(table)) > 1
    # the same seed, the same table; the default criteria are the script's six
    again = dfm.replicate_table(tuples, reps, np.random.default_rng(11), criteria=criteria,
                                select=oracle_select(oracle, []))
    assert np.array_equal(again, table)
    six = dfm.replicate_table(tuples[:1], 2, np.random.default_rng(5), select=oracle_select(oracle, []))
    assert six.shape == (1, 6)


def test_monte_carlo_layout_repack(dfm):
    """The (M, T, N) -> dfm_mc layout marshalling (no device): a list or a C-ordered array is repacked to M
    column-major panels; an array already laid out that way is passed as it is."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3, 7, 5))
    buf, M, T, N, ldx, stride, dev = dfm.api._mc_layout(list(a))
    assert (M, T, N, ldx, stride, dev) == (3, 7, 5, 7, 35, False)
    assert np.array_equal(buf.reshape(3, 5, 7), a.transpose(0, 2, 1)) and buf.flags.c_contiguous
    raw = np.full(3 * 50, np.nan)
    view = np.lib.stride_tricks.as_strided(raw, (3, 7, 5), (8 * 50, 8, 8 * 9))
    view[...] = a
    buf, M, T, N, ldx, stride, dev = dfm.api._mc_layout(view)
    assert buf is view and (M, T, N, ldx, stride, dev) == (3, 7, 5, 9, 50, False)
    with pytest.raises(ValueError):
        dfm.api._mc_layout(np.zeros((4, 4)))
