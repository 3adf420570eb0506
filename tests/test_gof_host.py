"""Host side of the goodness-of-fit feature, no device: the numpy oracle the device tests compare with (tests/gof_oracle.py)
against scipy's Poisson and hand-computed bins, the toy p-value, and the refusals of the likelihood classes."""
from collections import OrderedDict

import numpy as np
import pytest
from scipy import stats

import gof_oracle
import model_zoo
from blueice_amd import inference


def small_model(rng, S=2, B=17, anchors=(-1.0, 0.0, 1.0)):
    A = len(anchors)
    ps = rng.uniform(0.2, 1.0, size=(A, S, B))
    ps /= ps.sum(axis=-1, keepdims=True)
    mus = rng.uniform(20.0, 60.0, size=(A, S))
    return dict(anchor_z=[np.array(anchors)], ps=ps, mus=mus, n_model=None)


@pytest.mark.parametrize('z', [-1.0, 0.37, 1.0])
def test_oracle_deviance_is_scipys_poisson_likelihood_ratio(z):
    rng = np.random.default_rng(5)
    model = small_model(rng)
    rs = np.array([1.3, 0.6])
    s0 = gof_oracle.statistics(model, np.zeros(17), [z], rs)
    counts = rng.poisson(s0['mu']).astype(float)
    counts[3] = 0.0
    s = gof_oracle.statistics(model, counts, [z], rs)
    want = 2 * np.sum(stats.poisson.logpmf(counts, counts) - stats.poisson.logpmf(counts, s['mu']))
    assert abs(2 * s['half_deviance'] - want) <= 1e-9 * abs(want)
    assert abs(s['pearson'] - np.sum((counts - s['mu']) ** 2 / s['mu'])) <= 1e-12 * s['pearson']
    np.testing.assert_allclose(s['mu_sources'].sum(axis=0), s['mu'], rtol=1e-14)
    wide = gof_oracle.statistics(model, counts, [z], rs, dtype=np.longdouble)
    assert wide['mu'].dtype == np.longdouble and abs(float(wide['half_deviance']) - s['half_deviance']) <= 1e-12 * s['half_deviance']
    assert gof_oracle.point(model, counts, [z], rs)[:2] == (s['half_deviance'], s['pearson'])


def test_oracle_two_bin_cases_by_hand():
    model = dict(anchor_z=[], ps=np.array([[0.25, 0.75]]), mus=np.array([8.0]), n_model=None)       # mu = (2, 6)
    s = gof_oracle.statistics(model, [3.0, 6.0], [], [1.0])
    np.testing.assert_allclose(s['mu'], [2.0, 6.0], rtol=1e-15)
    np.testing.assert_allclose(s['half_terms'], [2 - 3 - 3 * np.log(2 / 3), 0.0], rtol=1e-15, atol=1e-15)
    np.testing.assert_allclose(s['pearson_terms'], [0.5, 0.0], rtol=1e-15)
    # an empty bin contributes its expectation to both; empty and nothing expected: nothing, and no 0 / 0
    empty = dict(model, ps=np.array([[1.0, 0.0]]))                                                   # mu = (8, 0)
    s = gof_oracle.statistics(empty, [0.0, 0.0], [], [1.0])
    assert list(s['half_terms']) == [8.0, 0.0] and list(s['pearson_terms']) == [8.0, 0.0]
    assert gof_oracle.point(empty, [0.0, 0.0], [], [1.0]) == (8.0, 8.0, 0)
    # an event where nothing is expected: +inf in both
    s = gof_oracle.statistics(empty, [8.0, 1.0], [], [1.0])
    assert s['half_terms'][1] == np.inf and s['pearson_terms'][1] == np.inf and s['half_terms'][0] == 0.0
    assert gof_oracle.point(empty, [8.0, 1.0], [], [1.0]) == (np.inf, np.inf, 0)
    # the screen: unphysical rates, and a negative expectation of a source that may go negative
    assert gof_oracle.point(empty, [8.0, 0.0], [], [-1.0]) == (np.inf, np.inf, gof_oracle.ST_UNPHYSICAL)
    two = dict(anchor_z=[np.array([0.0, 1.0])], ps=np.array([[[0.5, 0.5], [1.0, 0.0]]] * 2), mus=np.array([[4.0, 1.0]] * 2), n_model=None)
    assert gof_oracle.point(two, [1.0, 1.0], [1.5], [1.0, 1.0]) == (np.inf, np.inf, gof_oracle.ST_OUT_OF_BOUNDS)
    hd, pe, st = gof_oracle.point(two, [1.0, 1.0], [0.5], [1.0, -3.0], allow_negative=[False, True])    # mu = (-1, 2)
    assert np.isnan(hd) and np.isnan(pe) and st == 0


def test_toy_p_value_counts_ties_and_failed_toys_on_the_conservative_side():
    toys = np.array([1.0, 2.0, 2.0, 3.0, 5.0])
    assert inference.toy_p_value(2.0, toys) == (1 + 4) / 6                   # ties count as >=
    assert inference.toy_p_value(2.5, toys) == (1 + 2) / 6
    assert inference.toy_p_value(9.0, toys) == 1 / 6                         # never 0
    assert inference.toy_p_value(2.5, toys, failed=[True, False, False, False, True]) == (1 + 3) / 6
    assert inference.toy_p_value(2.5, toys, failed=np.ones(5, bool)) == 1.0
    assert inference.toy_p_value(2.5, [1.0, np.nan, np.inf]) == (1 + 2) / 4  # a nan statistic is not dropped either
    with pytest.raises(ValueError):
        inference.toy_p_value(1.0, [])
    with pytest.raises(ValueError):
        inference.toy_p_value(1.0, toys, failed=[True])
    res = inference.GofResult('deviance', 2.5, toys, [True, False, False, False, True], 3, OrderedDict(), OrderedDict())
    assert res.p_value == inference.toy_p_value(2.5, toys, res.failed) and res.n_failed == 2
    assert res.p_value_chi2 == stats.chi2.sf(2.5, 3)


NEW = ('expected_counts', 'expected_counts_points', 'gof_statistics', 'goodness_of_fit')


def _call(lf, name):
    if name == 'expected_counts_points':
        return getattr(lf, name)({})
    return getattr(lf, name)()


def test_names_are_public_and_methods():
    from blueice_amd.likelihood import BinnedLogLikelihood
    for name in NEW:
        assert name in inference.__all__ and getattr(BinnedLogLikelihood, name) is getattr(inference, name)


@pytest.mark.parametrize('name', NEW)
def test_refused_where_there_are_no_bins_or_they_depend_on_the_data(name):
    """Unbinned likelihoods, sums, reparametrisations, analytic terms and Beeston-Barlow raise NotImplementedError from the
    new methods -- before any device is touched (none of these likelihoods is prepared: there is no device here)."""
    ns = model_zoo.namespace_of('blueice_amd')
    unbinned = ns.UnbinnedLogLikelihood(ns.conf_for_test(events_per_day=1))
    anc = ns.LogAncillaryLikelihood(lambda values: 0.0, ['nuisance'], config=dict(nuisance=0.5))
    total = ns.LogLikelihoodSum([unbinned, anc])
    conf = ns.conf_for_test(events_per_day=1.)
    conf['sources'] = [dict(name='op0')]
    conf['np0'] = 1
    inner = ns.UnbinnedLogLikelihood(conf)
    inner.add_rate_parameter('op0')
    reparam = ns.LogLikelihoodReParam(inner, dict(np0=((0.5, 2.0), None, None),
                                                  op0_rate_multiplier=dict(params=['np0'], func=lambda a: a ** 2)))
    data, _ = ns.make_data([dict(n_events=32, x=0.5)])
    bb = ns.BinnedLogLikelihood(ns.conf_for_test(default_source_class=ns.FixedSampleSource, events_per_day=32 / 5,
                                                 analysis_space=[['x', [0, 1]]], data=data),
                                likelihood_config=dict(model_zoo.BB_LC))
    for lf in (unbinned, total, reparam, anc, bb):
        with pytest.raises(NotImplementedError):
            _call(lf, name)
        assert getattr(lf, 'ctx', None) is None
