"""Host side of the real-valued-counts feature, no device: the numpy oracle the device tests compare with
(tests/real_counts_oracle.py) against scipy (xlogy, gammaln), finite differences and hand-computed two-bin cases; the
asymptotic helpers' bookkeeping; and the refusals of the factories."""
import numpy as np
import pytest
from scipy.special import gammaln, xlogy

import model_zoo
import real_counts_oracle as rco
from blueice_amd import asimov, inference


def small_model(rng, S=2, B=17, anchors=(-1.0, 0.0, 1.0)):
    A = len(anchors)
    ps = rng.uniform(0.2, 1.0, size=(A, S, B))
    ps /= ps.sum(axis=-1, keepdims=True)
    mus = rng.uniform(20.0, 60.0, size=(A, S))
    return dict(anchor_z=[np.array(anchors)], ps=ps, mus=mus, n_model=None)


@pytest.mark.parametrize('z', [-1.0, 0.37, 1.0])
def test_oracle_half_deviance_is_the_ratio_to_the_saturated_model(z):
    """Real n: scipy's xlogy form term by term, and the difference of the two log-likelihoods with lgamma(n + 1) for log n!
    (which cancels), to the digits that difference has left."""
    rng = np.random.default_rng(5)
    model = small_model(rng)
    rs = np.array([1.3, 0.6])
    n = rco.expectation(model, [0.2], [1.0, 1.0]) * rng.uniform(0.2, 1.6, size=17)       # nothing integer about them
    n[3] = 0.0
    got = rco.point(model, n, [z], rs)
    mu = got['mu']
    assert got['status'] == 0 and np.all((n != np.floor(n)) | (n == 0))
    want = np.sum(xlogy(n, n / mu) - n + mu)
    assert abs(got['half_deviance'] - want) <= 1e-13 * abs(want)
    ll = np.sum(xlogy(n, mu) - mu - gammaln(n + 1))
    saturated = np.sum(xlogy(n, n) - n - gammaln(n + 1))
    assert abs(got['half_deviance'] - (saturated - ll)) <= 1e-11 * abs(ll)
    assert got['half_deviance'] > 0


@pytest.mark.parametrize('z', [-0.62, 0.37])
def test_oracle_gradient_is_the_slope_of_the_value(z):
    rng = np.random.default_rng(6)
    model = small_model(rng)
    rs = np.array([1.3, 0.6])
    n = rco.expectation(model, [0.1], [0.9, 1.2]) * 0.3                                  # counts inside (0, 1) mostly
    n[5] = 0.0
    got = rco.point(model, n, [z], rs)
    theta = np.concatenate([[z], rs])
    for q in range(3):
        h = 1e-6
        up, dn = theta.copy(), theta.copy()
        up[q] += h
        dn[q] -= h
        fd = (rco.point(model, n, up[:1], up[1:])['half_deviance'] - rco.point(model, n, dn[:1], dn[1:])['half_deviance']) / (2 * h)
        assert abs(got['grad'][q] - fd) <= 1e-6 * max(1.0, got['grad_cond'][q])
        assert got['grad_cond'][q] >= abs(got['grad'][q])


def test_oracle_is_exactly_zero_at_its_own_truth():
    model = small_model(np.random.default_rng(7))
    n = rco.expectation(model, [0.37], [1.3, 0.6])
    got = rco.point(model, n, [0.37], [1.3, 0.6])
    assert got['half_deviance'] == 0.0 and np.all(got['grad'] == 0.0) and np.all(got['grad_cond'] == 0.0)


def test_oracle_two_bin_cases_by_hand():
    model = dict(anchor_z=[], ps=np.array([[0.25, 0.75]]), mus=np.array([8.0]), n_model=None)       # mu = (2, 6) rs
    got = rco.point(model, [2.5, 0.0], [], [1.0])
    # bin 0: (2 - 2.5) - 2.5 log(2 / 2.5); bin 1 is empty: its expectation.  d mu / d rs = (2, 6): 2 (1 - 2.5 / 2) + 6
    assert abs(got['half_deviance'] - ((2 - 2.5) - 2.5 * np.log(2 / 2.5) + 6.0)) <= 1e-15
    np.testing.assert_allclose(got['grad'], [2 * (1 - 2.5 / 2) + 6.0], rtol=1e-15)
    np.testing.assert_allclose(got['grad_cond'], [2 * 0.25 + 6.0], rtol=1e-15)
    # a count where nothing is expected: +inf, nan slopes; nothing and nothing: 0
    empty = dict(model, ps=np.array([[1.0, 0.0]]))                                                   # mu = (8, 0)
    got = rco.point(empty, [8.0, 0.5], [], [1.0])
    assert got['half_deviance'] == np.inf and np.isnan(got['grad']).all() and got['status'] == 0
    got = rco.point(empty, [8.0, 0.0], [], [1.0])
    assert got['half_deviance'] == 0.0 and got['grad'][0] == 0.0
    # the screen, and a negative expectation of a source that may go negative
    got = rco.point(empty, [8.0, 0.0], [], [-1.0])
    assert got['half_deviance'] == np.inf and got['status'] == rco.ST_UNPHYSICAL and np.isnan(got['grad']).all()
    two = dict(anchor_z=[np.array([0.0, 1.0])], ps=np.array([[[0.5, 0.5], [1.0, 0.0]]] * 2), mus=np.array([[4.0, 1.0]] * 2), n_model=None)
    assert rco.point(two, [1.0, 1.0], [1.5], [1.0, 1.0])['status'] == rco.ST_OUT_OF_BOUNDS
    got = rco.point(two, [1.0, 1.0], [0.5], [1.0, -3.0], allow_negative=[False, True])              # mu = (-1, 2)
    assert np.isnan(got['half_deviance']) and got['status'] == 0 and np.isnan(got['grad']).all()


def test_names_are_public_and_methods():
    from blueice_amd.likelihood import BinnedLogLikelihood
    for name in ('asimov_test_statistic', 'expected_upper_limit', 'expected_discovery_significance'):
        assert name in inference.__all__ and getattr(BinnedLogLikelihood, name) is getattr(inference, name)
        assert getattr(asimov.AsimovLikelihood, name) is getattr(inference, name)
    for name in ('asimov', 'asimov_points', 'real_data'):
        assert getattr(BinnedLogLikelihood, name) is getattr(asimov, name)
    assert asimov.AsimovLikelihood.supports_hessian is False


def test_the_truth_of_an_expected_result_defaults_to_no_signal():
    class Lf:
        def _kwargs_to_settings(self):
            return [1.0], dict(shift=0.25)
    assert inference._asimov_truth(Lf(), 's0_rate_multiplier', None) == ({'s0_rate_multiplier': 0.0}, 0.0)
    assert inference._asimov_truth(Lf(), 's0_rate_multiplier', dict(shift=1.0)) == ({'s0_rate_multiplier': 1.0, 'shift': 1.0}, 1.0)
    assert inference._asimov_truth(Lf(), 'shift', dict(s0_rate_multiplier=2.0)) == ({'s0_rate_multiplier': 2.0, 'shift': 0.25}, 0.25)


@pytest.mark.parametrize('name', ['asimov', 'asimov_points', 'real_data', 'expected_upper_limit', 'expected_discovery_significance'])
def test_refused_where_there_is_no_real_valued_path(name):
    """Unbinned likelihoods, sums, reparametrisations, analytic terms and Beeston-Barlow raise NotImplementedError from the
    factories and from what is built on them -- before any device is touched (none of these is prepared: no device here)."""
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
    args = dict(asimov=(), asimov_points=({},), real_data=(np.zeros(1),), expected_upper_limit=('s0_rate_multiplier', 5.0),
                expected_discovery_significance=('s0_rate_multiplier', dict(s0_rate_multiplier=1.0)))[name]
    for lf in (unbinned, total, reparam, anc, bb):
        with pytest.raises(NotImplementedError):
            getattr(lf, name)(*args)
        assert getattr(lf, 'ctx', None) is None
