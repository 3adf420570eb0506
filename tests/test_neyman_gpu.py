"""Toy-calibrated intervals on the device: toy_test_statistics draws its toys at several hypotheses per generator call
(simulate_toys_points) and fits every chunk in one engine call per fit.  Held to the route the package had before -- one
hypothesis at a time with simulate_toys and the same two fits --, to the CPU oracle's likelihood maximised by scipy on every
downloaded toy, and, as the t_ppf of one_parameter_interval, to the definition of the limit."""
import numpy as np
import pytest
from scipy.optimize import minimize

import model_zoo
from oracle_lf import OracleLikelihood

pytestmark = pytest.mark.gpu
TOL = 1e-6                              # the project's bar for two routes to one maximum (tests/test_profile_gpu.py)


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


def oracle_of(lf, counts):
    """The CPU oracle's likelihood of `counts` on the tensors the device holds: the templates at every anchor"""
    import itertools
    names = list(lf.shape_parameters)
    grids = [np.array(sorted(float(a) for a in lf.shape_parameters[n][0])) for n in names]
    if names:
        shape = tuple(len(g) for g in grids)
        ps = np.stack([lf.ctx.interpolate('ps', z) for z in itertools.product(*grids)])
        mus = np.stack([lf.ctx.interpolate('mus', z) for z in itertools.product(*grids)])
        ps, mus = ps.reshape(shape + ps.shape[1:]), mus.reshape(shape + mus.shape[1:])
    else:
        ps, mus = lf.ctx.interpolate('ps', []), lf.ctx.interpolate('mus', [])
    o = OracleLikelihood(dict(anchor_z=grids, ps=ps, mus=mus, n_model=None), counts, names)
    o.pdf_base_config = {n: lf.pdf_base_config.get(n, 0.0) for n in names}
    return o


def polished(o, start, fixed):
    """scipy's bounded minimiser on the oracle's likelihood from `start` (dict of the floating parameters) -> max ll"""
    keys = list(start)
    bounds = [o.get_bounds(k) if k in o.shape_parameters else (0, None) for k in keys]
    res = minimize(lambda v: -o(**dict(fixed, **dict(zip(keys, v)))), [start[k] for k in keys], bounds=bounds, method='L-BFGS-B',
                   options=dict(ftol=1e-15, gtol=1e-9))
    return -res.fun


def spy_on_toys(lf):
    """-> a list that collects the counts of every toy the driver draws with simulate_toys_points, in drawn order"""
    seen, real = [], lf.simulate_toys_points

    def spy(*args, **kwargs):
        out = real(*args, **kwargs)
        seen.extend(lf.ctx.download_counts(t) for t in range(lf.ctx.T))
        return out
    lf.simulate_toys_points = spy
    return seen


def per_hypothesis(lf, target, hyp, n, seed, truth=None, fit_options=None, **fixed):
    """The same ensemble the way the package offered before: a simulate_toys per hypothesis with toy_offset set, then the
    driver's two fits -> (ll_free, ll_cond [H, n], counts of every toy or None)"""
    ll_free, ll_cond, toys = [], [], []
    truth = {k: np.broadcast_to(v, (len(hyp),)) for k, v in (truth or {}).items()}
    try:
        for i, h in enumerate(hyp):
            lf.ctx.set_param('toy_offset', n * i)
            lf.simulate_toys(n, seed=seed, **dict({k: float(v[i]) for k, v in truth.items()}, **{target: h}))
            if hasattr(lf, 'simulate_toys_points'):
                toys.extend(lf.ctx.download_counts(t) for t in range(n))
            ds = np.arange(n)
            start, lc = lf.bestfit_batched(points={target: np.full(n, h)}, datasets=ds, **(fit_options or {}), **fixed)
            _, lfree = lf.bestfit_batched(datasets=ds, also_from=[dict(start, **{target: np.full(n, h)})], **(fit_options or {}), **fixed)
            ll_free.append(lfree)
            ll_cond.append(lc)
    finally:
        lf.ctx.set_param('toy_offset', 0)
    return np.stack(ll_free), np.stack(ll_cond), (np.stack(toys) if toys else None)


def test_rates_only_against_the_per_hypothesis_route_and_the_oracle(ns):
    lf, _, _ = model_zoo.d0_multi_source(ns)
    target, hyp, n, seed = 's0_rate_multiplier', (0.5, 1.0, 2.0), 6, 3
    seen = spy_on_toys(lf)
    st = lf.toy_test_statistics(target, hyp, n, seed=seed, chunk=8)               # chunks of 8 straddle the hypotheses' 6
    del lf.simulate_toys_points
    assert st.t.shape == (3, n) and st.n_failed == 0 and len(seen) == 3 * n
    ll_free, ll_cond, toys = per_hypothesis(lf, target, hyp, n, seed)
    np.testing.assert_array_equal(np.stack(seen), toys)
    np.testing.assert_allclose(st.ll_free, ll_free, rtol=1e-9)
    np.testing.assert_allclose(st.ll_cond, ll_cond, rtol=1e-9)
    top = max(np.abs(ll_free).max(), np.abs(ll_cond).max())
    assert np.all(np.abs(st.t - 2 * (ll_free - ll_cond)) <= 4e-9 * top)
    assert np.all(st.t >= -1e-9 * top) and np.std(st.t) > 0
    # independently: the oracle's likelihood of every downloaded toy, maximised by scipy (concave: the maxima are unique)
    names = [s + '_rate_multiplier' for s in lf.source_name_list]
    for i, h in enumerate(hyp):
        for j in range(n):
            o = oracle_of(lf, toys[i * n + j])
            free = polished(o, {k: 1.0 for k in names}, {})
            cond = polished(o, {k: 1.0 for k in names if k != target}, {target: h})
            assert abs(st.ll_free[i, j] - free) <= TOL * max(1.0, abs(free)), (i, j, st.ll_free[i, j], free)
            assert abs(st.ll_cond[i, j] - cond) <= TOL * max(1.0, abs(cond)), (i, j, st.ll_cond[i, j], cond)
            assert abs(st.t[i, j] - 2 * (free - cond)) <= 4 * TOL * max(1.0, abs(free)), (i, j, st.t[i, j], 2 * (free - cond))


def test_shape_parameter_with_kinks_and_the_data_come_back(ns):
    lf, _, _ = model_zoo.c1_like(ns)
    at = dict(shift=0.37, s0_rate_multiplier=1.2)
    before, before0 = lf(**at), lf()
    data = lf.ctx.download_counts(0)
    target, hyp, n = 's0_rate_multiplier', (0.8, 1.3), 8
    seen = spy_on_toys(lf)
    st = lf.toy_test_statistics(target, hyp, n, seed=5, truth=dict(shift=[0.3, -0.4]))
    del lf.simulate_toys_points
    assert st.t.shape == (2, n) and st.n_failed == 0 and list(st.best) == ['s0_rate_multiplier', 's1_rate_multiplier', 'shift']
    assert np.all(st.t >= -1e-9 * np.abs(st.ll_free))
    for i in range(2):
        for j in range(n):
            o = oracle_of(lf, seen[i * n + j])
            top = polished(o, {k: float(v[i, j]) for k, v in st.best.items()}, {})
            assert st.ll_free[i, j] >= top - TOL * max(1.0, abs(top)), (i, j, st.ll_free[i, j], top)
    # the likelihood's own data are back: the same bits
    assert lf.ctx.T == 1 and lf.ctx.get_param('toy_offset') == 0
    np.testing.assert_array_equal(lf.ctx.download_counts(0), data)
    assert lf(**at) == before and lf() == before0
    # the generator call itself: the truth of every dataset, and the refusal outside the anchor box
    methods = lf.simulate_toys_points(dict(shift=[0.3, -0.4, 1.0], s0_rate_multiplier=1.1), [1, 0, 2], seed=5)
    assert list(methods) == [0, -1, 0] and list(lf.toy_truth) == [0, 2, 2] and lf.ctx.T == 3
    with pytest.raises(ValueError, match='anchor box.*truth 1'):
        lf.simulate_toys_points(dict(shift=[0.0, 1.5]), 1)
    assert lf.ctx.T == 3


def test_beeston_barlow_goes_through_the_dense_counts(ns):
    lf, _, _ = model_zoo.bb_d2(ns)
    target, hyp, n, seed = 's1_rate_multiplier', (0.8, 1.5), 4, 6
    truth = dict(shift=0.2, stretch=0.5)
    st = lf.toy_test_statistics(target, hyp, n, seed=seed, truth=truth, s2_rate_multiplier=1.)
    assert st.n_failed == 0 and np.all(np.isfinite(st.t))
    ll_free, ll_cond, _ = per_hypothesis(lf, target, hyp, n, seed, truth=truth, s2_rate_multiplier=1.)
    np.testing.assert_allclose(st.ll_free, ll_free, rtol=1e-9)
    np.testing.assert_allclose(st.ll_cond, ll_cond, rtol=1e-9)


def test_unbinned_likelihood_takes_one_hypothesis_per_chunk(ns):
    """(histogram-pdf sources, which the device can simulate: the unbinned toy model of tests/test_unbinned_toys_gpu.py)"""
    from test_unbinned_toys_gpu import make_lf
    lf = make_lf(ns, 'b', 'linear')
    events = lf._data
    before = lf(shift=0.1)
    target, hyp, n, seed = 's0_rate_multiplier', (0.05, 0.1), 4, 9
    truth = dict(shift=0.35, s1_rate_multiplier=0.05, s2_rate_multiplier=0.05)
    offsets, real = [], lf.simulate_toys

    def spy(*args, **kwargs):
        offsets.append((lf.ctx.get_param('toy_offset'), args[0]))
        return real(*args, **kwargs)
    lf.simulate_toys = spy
    st = lf.toy_test_statistics(target, hyp, n, seed=seed, chunk=3, truth=truth)
    del lf.simulate_toys
    assert offsets == [(0, 3), (3, 1), (4, 3), (7, 1)]
    assert lf._data is events and lf.ctx.T == 1 and lf(shift=0.1) == before          # set_data of the events it held
    ll_free, ll_cond, _ = per_hypothesis(lf, target, hyp, n, seed, truth=truth)
    np.testing.assert_allclose(st.ll_free, ll_free, rtol=1e-9)
    np.testing.assert_allclose(st.ll_cond, ll_cond, rtol=1e-9)
    assert np.all(st.t >= -1e-9 * np.abs(st.ll_free)) and np.std(st.t) > 0


def test_interval_with_thresholds_from_toys(ns):
    from blueice_amd.inference import ToyThresholds
    lf, _, _ = model_zoo.d0_multi_source(ns)
    target, cl = 's0_rate_multiplier', 0.9
    best, ll = lf.bestfit_batched()
    hyp = np.linspace(max(0.25, float(best[target][0])), 4.0, 4)
    table = lf.neyman_thresholds(target, hyp, 20, seed=11, kind='upper', chunk=32)
    assert isinstance(table, ToyThresholds) and table.kind == 'upper' and table.t.shape == (4, 20)
    crit = table.critical_values(cl)
    assert np.all(crit >= 0) and np.all(crit < 10) and np.any(crit > 0)
    _, again = lf.bestfit_batched()
    assert again[0] == ll[0]                                                      # the data are back
    limit = lf.one_parameter_interval(target, bound=6., kind='upper', confidence_level=cl, t_ppf=table)
    assert best[target][0] < limit < 6.
    _, at = lf.bestfit_batched(points={target: np.array([limit])}, also_from=[{k: v[0] for k, v in best.items() if k != target}])
    assert abs(2 * (ll[0] - at[0]) - table(limit, cl)) <= 1e-6                    # t(limit) = the table's critical value there
