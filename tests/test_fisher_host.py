"""Host side of the expected-information feature, no device: the numpy oracle the device tests compare with
(tests/fisher_oracle.py) against an extended-precision evaluation, the chain rule to the user's parameters against central
differences of a numpy expectation, the covariance with unbounded parameters against the ordinary inverse, the closed form of a
counting experiment, and the refusals."""
import numpy as np
import pytest

import fisher_oracle as fo
import hessian_oracle as ho
import model_zoo
from blueice_amd import hessian, inference
from fisher_fixtures import FIXTURES, fixture_model, fixture_points

TOL = 1e-10


@pytest.mark.parametrize('name', FIXTURES)
def test_oracle_against_extended_precision(name):
    """The float64 sums of the oracle against the same sums in longdouble, on the fixtures and points of the device tests:
    the worst |err| / max(1, cond) must sit far inside the 1e-10 the device is held to (it is what the device's margin is
    judged against)."""
    model = fixture_model(name)
    zs, rs = fixture_points(name)
    worst = 0.0
    for z, r in zip(zs, rs):
        got, want = fo.information(model, z, r), fo.information_longdouble(model, z, r)
        assert np.array_equal(got['unbounded'], want['unbounded'])
        worst = max(worst, fo.check(got['info'], dict(info=np.asarray(want['info'], dtype=float), cond=got['cond']), name, tol=1e-13))
        assert abs(got['total'] - float(want['total'])) <= 1e-13 * max(1.0, got['total'])
        assert np.all(got['cond'] >= np.abs(got['info']) * (1 - 1e-15))
    print('%s: the oracle against longdouble, worst |err| / max(1, cond) = %.3g' % (name, worst))
    assert worst <= 1e-13


def user_information(model, x, rate_sources, L, eff_const, eff_axis, h=1e-4):
    """I over the user's parameters x = (rate multipliers of the sources `rate_sources`, then the shape parameters) from
    central differences of the numpy expectation mu(x): rate_scale_s = m_s L e_s, e_s = eff_const[s] or shape parameter
    eff_axis[s].  mu is multilinear in x inside a cell except for an efficiency that is a shape parameter (quadratic in it):
    central differences are exact for both up to their rounding, ~ 2^-52 / h relative."""
    S = len(eff_axis)
    n_rates = len(rate_sources)

    def mu(x):
        m = np.ones(S)
        m[rate_sources] = x[:n_rates]
        z = x[n_rates:]
        e = np.array([z[eff_axis[s]] if eff_axis[s] >= 0 else eff_const[s] for s in range(S)])
        return ho._mu_derivatives(model, z, m * L * e)[0]
    mu0 = mu(x)
    d = []
    for j in range(len(x)):
        e = np.zeros(len(x))
        e[j] = h
        d.append((mu(x + e) - mu(x - e)) / (2 * h))
    d = np.array(d)
    pos = mu0 > 0
    return np.einsum('qb,rb->qr', d[:, pos] / mu0[pos], d[:, pos]), np.einsum('qb,rb->qr', np.abs(d[:, pos]) / mu0[pos], np.abs(d[:, pos]))


@pytest.mark.parametrize('what', ['livetime', 'constant efficiency', 'efficiency that is a shape parameter'])
def test_chain_rule_information_against_central_differences(what):
    """J I J^T of the oracle's information over (z, rate_scale) against the information formed from central differences of
    the expectation in the user's parameters.  d = 2, S = 3, two registered rates; bound: 1e-7 max(1, cond) -- the differences'
    rounding (2^-52 / 1e-4 ~ 2e-12 relative per slope, products of two slopes) with a wide margin."""
    model = fixture_model('d2_nonuniform')
    S, d = 3, 2
    L = 2.5 if what == 'livetime' else 1.0
    eff_const = [1.0, 0.7, 1.0] if what != 'livetime' else [1.0] * S
    eff_axis = [-1, -1, 1] if what.endswith('shape parameter') else [-1] * S
    rate_sources = [0, 2]
    x = np.array([1.3, 0.8, 0.1, 1.7])                   # m_0, m_2, z_0, z_1 (z_1 doubles as the efficiency of source 2)
    mult = np.array([[1.3, 1.0, 0.8]])
    z = x[2:]
    eff = np.array([[z[eff_axis[s]] if eff_axis[s] >= 0 else eff_const[s] for s in range(S)]])
    rs = mult[0] * L * eff[0]
    theta = fo.information(model, z, rs)
    got = hessian.chain_rule_information(theta['info'][None], mult, L, eff, eff_axis, rate_sources)[0]
    want, cond = user_information(model, x, rate_sources, L, eff_const, eff_axis)
    assert got.shape == (4, 4) and np.array_equal(got, got.T)
    err = np.abs(got - want) / np.maximum(1.0, cond)
    print('%s: chain rule against differences, worst |err| / max(1, cond) = %.3g' % (what, err.max()))
    assert np.all(err <= 1e-7)
    # a prior's curvature goes on the diagonal with the other sign
    curv = np.array([[-4.0, 0.0, -0.25, 0.0]])
    with_prior = hessian.chain_rule_information(theta['info'][None], mult, L, eff, eff_axis, rate_sources, curv)[0]
    assert np.array_equal(with_prior, got + np.diag([4.0, 0.0, 0.25, 0.0]))
    # the Jacobian is chain_rule_hessian's: with gs = 0 (no second-order term) the two transforms are the same
    H = hessian.chain_rule_hessian(np.zeros((1, d)), np.zeros((1, S)), theta['info'][None], mult, L, eff, eff_axis, rate_sources)[1][0]
    np.testing.assert_allclose(H, got, rtol=1e-15, atol=0)


def test_chain_rule_unbounded_follows_the_jacobian():
    # d = 1, S = 2: source 1's efficiency is the shape parameter; unbounded on rate_scale_1 flags m_1 and the shape parameter
    unb = np.array([[0, 0, 3], [2, 0, 0], [0, 0, 0]])
    got = hessian.chain_rule_unbounded(unb, np.ones((3, 2)), 1.0, np.ones((3, 2)), [-1, 0], [0, 1])
    assert got.tolist() == [[False, True, True], [False, False, True], [False, False, False]]
    # an efficiency of 0 takes the multiplier out of the expectation: nothing moves with it
    got = hessian.chain_rule_unbounded(np.array([[5]]), np.ones((1, 1)), 1.0, np.zeros((1, 1)), [-1], [0])
    assert got.tolist() == [[False]]


def test_covariance_from_information_with_unbounded_parameters():
    """Flagged parameters: variance 0 and covariance 0 with everything, the rest the inverse of the remaining block -- the
    ordinary inverse with I_qq = 1e30 there, to 1e-12 of the largest entry (the limit's own remainder is ~ 1e-30)."""
    rng = np.random.default_rng(3)
    A = rng.normal(size=(5, 9))
    info = A @ A.T
    flags = np.array([False, True, False, False, True])
    got = hessian.covariance_from_information(info, flags)
    big = info.copy()
    big[flags, flags] = 1e30
    want = np.linalg.inv(big)
    assert np.all(got[flags] == 0.0) and np.all(got[:, flags] == 0.0)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())
    np.testing.assert_allclose(hessian.covariance_from_information(info), np.linalg.inv(info), rtol=1e-10)
    # batched, a flag row per point; singular, indefinite or nan blocks give nan
    stack = np.stack([info, info, np.ones((5, 5)), -info, np.full((5, 5), np.nan)])
    cov = hessian.covariance_from_information(stack, np.stack([flags, ~flags, flags, flags, flags]))
    assert np.array_equal(cov[0], got) and np.isfinite(cov[1]).all() and np.isnan(cov[2:]).all()
    assert np.all(cov[1][~flags] == 0.0) and np.array_equal(cov[1], cov[1].T)
    # everything flagged: all zeros
    assert np.array_equal(hessian.covariance_from_information(info, np.ones(5, bool)), np.zeros((5, 5)))


def test_closed_form_of_a_counting_experiment():
    """One bin, signal s and background b, the background fixed: sigma(signal multiplier) = sqrt(s + b) / s; floating both,
    the information s_i s_j / (s + b) is singular: nan"""
    s, b = 10.0, 50.0
    model = dict(anchor_z=[], ps=np.ones((2, 1)), mus=np.array([s, b]), n_model=None)
    theta = fo.information(model, [], [1.0, 1.0])
    assert theta['total'] == s + b and not theta['unbounded'].any()
    info = hessian.chain_rule_information(theta['info'][None], np.ones((1, 2)), 1.0, np.ones((1, 2)), [-1, -1], [0])[0]
    sigma = np.sqrt(hessian.covariance_from_information(info)[0, 0])
    assert abs(sigma - np.sqrt(s + b) / s) <= 1e-15 * sigma
    both = hessian.chain_rule_information(theta['info'][None], np.ones((1, 2)), 1.0, np.ones((1, 2)), [-1, -1], [0, 1])[0]
    np.testing.assert_allclose(both, np.outer([s, b], [s, b]) / (s + b), rtol=1e-15)
    # twice the live time: half the variance
    twice = hessian.chain_rule_information(fo.information(model, [], [2.0, 2.0])['info'][None], np.ones((1, 2)), 2.0, np.ones((1, 2)),
                                           [-1, -1], [0])[0]
    assert abs(twice[0, 0] - 2 * info[0, 0]) <= 1e-15 * twice[0, 0]
    # no signal expected: the bin still expects the background, nothing is unbounded, and the multiplier's error is sqrt(b) / s
    none = fo.information(model, [], [0.0, 1.0])
    assert not none['unbounded'].any() and abs(none['info'][0, 0] - s * s / b) <= 1e-15 * s * s / b
    # no background either: the bin expects nothing but would with a signal -- unbounded on the signal's rate
    empty = fo.information(model, [], [0.0, 0.0])
    assert empty['unbounded'].tolist() == [1, 1] and np.all(empty['info'] == 0.0)


def test_names_are_public_and_methods():
    from blueice_amd import asimov
    from blueice_amd.likelihood import BinnedLogLikelihood
    for name in ('fisher_information_points', 'fisher_information', 'expected_covariance', 'expected_errors'):
        assert name in inference.__all__ and getattr(BinnedLogLikelihood, name) is getattr(inference, name)
    assert asimov.AsimovLikelihood.supports_hessian is False


@pytest.mark.parametrize('name', ['fisher_information_points', 'fisher_information', 'expected_covariance', 'expected_errors', 'hesse'])
def test_refused_where_there_are_no_bins(name):
    """Unbinned likelihoods, sums, reparametrisations, analytic terms and Beeston-Barlow raise NotImplementedError before any
    device is touched (none of these is prepared: no device here)."""
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
            if name == 'hesse':
                lf.hesse(dict(s0_rate_multiplier=1.0), information='expected')
            elif name == 'fisher_information_points':
                lf.fisher_information_points({})
            else:
                getattr(lf, name)()
        assert getattr(lf, 'ctx', None) is None


def test_hesse_refuses_an_unknown_information():
    with pytest.raises(ValueError, match='bogus'):
        inference.hesse(object(), dict(s0_rate_multiplier=1.0), information='bogus')
