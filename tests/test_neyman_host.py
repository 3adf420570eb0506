"""Toy-calibrated intervals without a GPU: the threshold table (ToyThresholds) on exact quantile grids, the driver
(toy_test_statistics) on the CPU-oracle likelihood with numpy toys (tests/oracle_toys_lf.py), and a table as the t_ppf of
one_parameter_interval."""
import numpy as np
import pytest
from scipy import stats

from blueice_amd import inference
from golden_util import load_case
from oracle_toys_lf import OracleToysLikelihood

N = 4000
SHAPES = dict(z0=0.1, z1=1.5)                         # the shape parameters stay fixed: the fits are over the three rates
TARGET = 's0_rate_multiplier'


def chi2_rows(kind):
    """An exact quantile grid of the large-sample law of t: chi-square (1 dof) at the probabilities (j + 1/2) / n for kind
    'central'; for the one-sided kinds its half -- P(t <= c) = Phi(sqrt(c)): zero with probability 1/2."""
    p = (np.arange(N) + 0.5) / N
    if kind == 'central':
        return stats.norm.ppf(0.5 + p / 2) ** 2
    return np.maximum(stats.norm.ppf(p), 0.0) ** 2


@pytest.mark.parametrize('kind', ['central', 'upper', 'lower'])
def test_thresholds_reproduce_wilks_on_an_exact_grid(kind):
    rows = chi2_rows(kind)
    rng = np.random.default_rng(1)
    table = inference.ToyThresholds([2.0, 1.0], np.stack([rng.permutation(rows), rng.permutation(rows)]), kind)
    for q in (0.05, 0.84, 0.95):
        want = stats.norm.ppf(q) ** 2
        level = abs(2 * q - 1) if kind == 'central' else max(q, 1 - q)
        assert table.level(q) == level
        # the conservative empirical quantile is an order statistic next to the level: the exact value lies within the gap
        # between its two neighbours
        k = int(np.searchsorted(rows, want))
        assert 1 <= k < N - 1
        gap = rows[k + 1] - rows[k - 1]
        for h in (1.0, 1.3, 2.0, 0.0, 5.0):
            assert abs(table(h, q) - want) <= gap, (kind, q, h, table(h, q), want, gap)
        assert table(1.0, q) in rows and table(1.0, q) >= np.quantile(rows, level)


def test_thresholds_interpolate_clamp_and_refuse():
    t = np.stack([np.arange(10.0), 2 * np.arange(10.0), 4 * np.arange(10.0)])
    table = inference.ToyThresholds([3.0, 1.0, 2.0], t, 'upper')                      # (rows in any order of hypotheses)
    np.testing.assert_array_equal(table.hypotheses, [1.0, 2.0, 3.0])
    q = 0.75                                                                          # 'higher': the order statistic at or above 0.75 * 9
    c1, c2, c3 = 2 * 7.0, 4 * 7.0, 7.0
    assert (table(1.0, q), table(2.0, q), table(3.0, q)) == (c1, c2, c3)
    assert table(1.25, q) == pytest.approx(0.75 * c1 + 0.25 * c2, rel=1e-15)
    assert table(2.5, q) == pytest.approx(0.5 * (c2 + c3), rel=1e-15)
    assert table(0.0, q) == c1 and table(-5.0, q) == c1 and table(3.5, q) == c3
    assert table(1.0, 0.25) == c1                                                     # one-sided: the mirror image, as norm.ppf(q)**2
    assert table(1.0, 0.9) == 2 * 9.0                                                 # level 0.9 = 1 - 1/n: the last that 10 toys resolve
    with pytest.raises(ValueError, match='more toys are needed'):
        table(1.0, 0.95)
    central = inference.ToyThresholds([1.0], t[:1], 'central')
    assert central(1.0, 0.95) == central(1.0, 0.05) == 9.0                            # level 0.9
    with pytest.raises(ValueError, match='more toys are needed'):
        central(1.0, 0.96)
    with pytest.raises(ValueError):
        inference.ToyThresholds([1.0, 2.0], t, 'upper')
    with pytest.raises(ValueError):
        inference.ToyThresholds([1.0], t[:1], 'two-sided')


@pytest.fixture(scope='module')
def lf():
    c = load_case('d2_nonuniform')
    return OracleToysLikelihood(c['model'], c['counts'], ['z0', 'z1'])


HYP, N_TOYS, SEED = (0.6, 1.0, 1.7), 4, 7


@pytest.fixture(scope='module')
def whole(lf):
    return lf.toy_test_statistics(TARGET, HYP, N_TOYS, seed=SEED, chunk=5, truth=dict(s1_rate_multiplier=[1.0, 1.1, 0.9]), **SHAPES)


def test_driver_does_not_depend_on_the_chunking_and_restores_the_data(lf, whole):
    data = lf.counts.copy()
    before = lf(**SHAPES)
    restored = lf.n_restored
    one = lf.toy_test_statistics(TARGET, HYP, N_TOYS, seed=SEED, chunk=1, truth=dict(s1_rate_multiplier=[1.0, 1.1, 0.9]), **SHAPES)
    assert lf.n_restored == restored + 1 and lf.ctx.T == 1 and lf.ctx.get_param('toy_offset') == 0
    np.testing.assert_array_equal(lf.counts, data)
    assert lf(**SHAPES) == before
    assert whole.t.shape == (3, N_TOYS) and whole.kind == 'central' and list(whole.hypotheses) == list(HYP)
    # (the same toys and the same starts; a stand-in without batching effects: the same numbers)
    np.testing.assert_allclose(one.ll_free, whole.ll_free, rtol=1e-12)
    np.testing.assert_allclose(one.ll_cond, whole.ll_cond, rtol=1e-12)
    np.testing.assert_allclose(one.t, whole.t, atol=4e-12 * np.abs(whole.ll_free).max())
    assert np.all(whole.ll_free >= whole.ll_cond - 1e-9 * np.abs(whole.ll_free))
    np.testing.assert_array_equal(whole.t, 2 * (whole.ll_free - whole.ll_cond))       # raw, not clipped
    assert whole.n_failed == 0 and whole.n_converged == whole.t.size and whole.engine_calls > 0
    assert np.std(whole.t) > 0


def test_driver_numbers_its_toys_globally(lf, whole):
    """Toy j of hypothesis i is toy first_toy + i n + j: a chunk of a duck-typed likelihood holds one hypothesis, its
    toy_offset the number of its first toy; ranges and first_toy pick out the toys one call would draw."""
    lf.ctx.offsets_seen.clear()
    lf.toy_test_statistics(TARGET, HYP, N_TOYS, seed=SEED, chunk=3, **SHAPES)
    assert lf.ctx.offsets_seen == [0, 3, 4, 7, 8, 11, 0]                           # (the last: reset)
    lf.ctx.offsets_seen.clear()
    part = lf.toy_test_statistics(TARGET, HYP, N_TOYS, seed=SEED, chunk=5, toy_range=(1, 3), truth=dict(s1_rate_multiplier=[1.0, 1.1, 0.9]),
                                  **SHAPES)
    assert lf.ctx.offsets_seen == [1, 5, 9, 0] and part.t.shape == (3, 2)
    np.testing.assert_allclose(part.ll_free, whole.ll_free[:, 1:3], rtol=1e-12)
    np.testing.assert_allclose(part.ll_cond, whole.ll_cond[:, 1:3], rtol=1e-12)
    # first_toy: hypothesis 1 of a call that starts at toy 4 of the ensemble is ... hypothesis 1's toys again, when the
    # truth is the same
    lf.ctx.offsets_seen.clear()
    shifted = lf.toy_test_statistics(TARGET, [HYP[1]], N_TOYS, seed=SEED, first_toy=N_TOYS, truth=dict(s1_rate_multiplier=1.1), **SHAPES)
    assert lf.ctx.offsets_seen == [N_TOYS, 0]
    np.testing.assert_allclose(shifted.ll_free[0], whole.ll_free[1], rtol=1e-12)
    np.testing.assert_allclose(shifted.ll_cond[0], whole.ll_cond[1], rtol=1e-12)
    # ... and the toys are the stand-in's toys of those numbers
    lf.ctx.set_param('toy_offset', 5)
    lf.simulate_toys(2, seed=SEED, s0_rate_multiplier=HYP[1], s1_rate_multiplier=1.1)       # (drawn at the truth: not at what the fits fix)
    lf.ctx.set_param('toy_offset', 0)
    _, again = lf.bestfit_batched(datasets=np.arange(2), **SHAPES)
    np.testing.assert_allclose(again, whole.ll_free[1, 1:3], rtol=1e-9)
    _, again = lf.bestfit_batched(points={TARGET: np.full(2, HYP[1])}, datasets=np.arange(2), **SHAPES)
    np.testing.assert_allclose(again, whole.ll_cond[1, 1:3], rtol=1e-9)
    lf.set_binned_data(load_case('d2_nonuniform')['counts'])
    with pytest.raises(ValueError, match='toy_range'):
        lf.toy_test_statistics(TARGET, HYP, N_TOYS, toy_range=(2, 5), **SHAPES)


def test_one_sided_statistics_are_zero_on_the_far_side(lf, whole):
    up = lf.toy_test_statistics(TARGET, HYP, N_TOYS, seed=SEED, chunk=5, kind='upper', truth=dict(s1_rate_multiplier=[1.0, 1.1, 0.9]), **SHAPES)
    lo = lf.toy_test_statistics(TARGET, HYP, N_TOYS, seed=SEED, chunk=5, kind='lower', truth=dict(s1_rate_multiplier=[1.0, 1.1, 0.9]), **SHAPES)
    h = np.asarray(HYP)[:, None]
    above = whole.target_hat >= h
    assert above.any() and (~above).any()
    np.testing.assert_array_equal(up.t[above], 0.0)
    np.testing.assert_allclose(up.t[~above], whole.t[~above], atol=1e-9)
    below = whole.target_hat <= h
    np.testing.assert_array_equal(lo.t[below], 0.0)
    np.testing.assert_allclose(lo.t[~below], whole.t[~below], atol=1e-9)
    with pytest.raises(ValueError, match='kind'):
        lf.toy_test_statistics(TARGET, HYP, N_TOYS, kind='both', **SHAPES)


def test_nothing_left_to_profile_evaluates_the_hypotheses(lf):
    fixed = dict(SHAPES, s1_rate_multiplier=1.0, s2_rate_multiplier=1.0)
    st = lf.toy_test_statistics(TARGET, HYP[:2], 2, seed=SEED, **fixed)
    lf.simulate_toys(2, seed=SEED, **{TARGET: HYP[0]})
    want = lf.eval_points(dict(fixed, **{TARGET: HYP[0]}), dataset=np.arange(2))
    lf.set_binned_data(load_case('d2_nonuniform')['counts'])
    np.testing.assert_array_equal(st.ll_cond[0], want)
    assert np.all(st.t >= -1e-9)


@pytest.mark.parametrize('kind,cl', [('upper', 0.9), ('central', 0.68)])
def test_a_constant_table_gives_the_default_interval(lf, kind, cl):
    """t_ppf = a table whose every row is norm.ppf(cl)**2 is Wilks: the same limits, to the 1e-6 the project holds two
    routes to one limit to."""
    target = 's1_rate_multiplier'                       # (its best fit, 2.17, lies well inside (0.3, 5): both crossings exist)
    bound = {'upper': 5.0, 'central': (0.3, 5.0)}[kind]
    crit = stats.norm.ppf(cl if kind != 'central' else 1 - (1 - cl) / 2) ** 2
    table = inference.ToyThresholds([0.1, 10.0], np.full((2, 50), crit), kind)
    default = lf.one_parameter_interval(target, bound, confidence_level=cl, kind=kind, **SHAPES)
    toys = lf.one_parameter_interval(target, bound, confidence_level=cl, kind=kind, t_ppf=table, **SHAPES)
    np.testing.assert_allclose(toys, default, rtol=1e-6)


def test_names_are_public_and_methods(lf):
    assert 'toy_test_statistics' in inference.__all__ and 'neyman_thresholds' in inference.__all__
    from blueice_amd.likelihood import LogLikelihoodBase
    assert LogLikelihoodBase.neyman_thresholds is inference.neyman_thresholds
    st = inference.ToyStatistics([1.0], 'upper', np.array([[0.0, 1.0, 4.0]]), None, None, None, np.ones((1, 3), bool), np.zeros((1, 3), bool))
    table = inference.ToyThresholds.from_statistics(st)
    assert table.kind == 'upper' and table(1.0, 0.5) == 1.0
