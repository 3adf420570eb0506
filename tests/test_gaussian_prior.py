"""GaussianPrior without a GPU: the closed form against scipy's frozen normal, its slope and curvature against exact
arithmetic, the opt-in of add_rate_uncertainty / add_shape_uncertainty, the closed forms on the host paths, and the two
entry points of the C ABI that take the terms into the native loops."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import stats

from blueice_amd import GaussianPrior
from blueice_amd.exceptions import InvalidParameterSpecification

EPS = np.finfo(float).eps
# (mean, sigma): unit, wide, narrow, off-centre; log(sigma) of a few units at most (the bound below is relative to the VALUE)
PARAMS = [(0.0, 1.0), (1.0, 0.3), (0.5, 0.4), (-3.25, 7.5), (21.0, 2.0), (1e3, 0.05), (-0.125, 40.0)]


@pytest.mark.parametrize('mean, sigma', PARAMS)
def test_value_is_scipys_logpdf(mean, sigma):
    """Both are -t^2 / 2 - log(sigma) - log(2 pi) / 2 with t = (x - mean) / sigma; t and t^2 / 2 round alike, and the two
    differ in the order of the two subtractions that follow: four roundings in all, each at most half an ulp of a number
    no larger than max(1, |value|) here (|log sigma| < 4) -- so they agree to 4 eps max(1, |value|)."""
    rng = np.random.default_rng(int(abs(mean) * 8 + sigma * 64))
    x = np.concatenate([mean + sigma * rng.uniform(-30, 30, 9000), mean + sigma * rng.normal(0, 1, 996),
                        mean + sigma * np.array([-30.0, 30.0, 0.0, 1e-9])])
    assert len(x) == 10 ** 4
    got, want = GaussianPrior(mean, sigma)(x), stats.norm(mean, sigma).logpdf(x)
    assert got.shape == x.shape
    assert np.all(np.abs(got - want) <= 4 * EPS * np.maximum(1.0, np.abs(want)))
    assert np.max(np.abs((x - mean) / sigma)) >= 29.9
    # scalars give scalars, and the same numbers
    for k in (0, 17, 9999):
        assert GaussianPrior(mean, sigma)(float(x[k])) == got[k]


def test_slope_and_curvature_are_exact():
    """against mpmath at 60 digits where it is installed, else against the exact rationals of dyadic inputs: the slope is two
    divisions and a subtraction (<= 1.5 ulp, 2 asserted), the curvature a square and a division (<= 1 ulp, 2 asserted)"""
    try:
        import mpmath
        mpmath.mp.dps = 60
        exact = lambda v: mpmath.mpf(float(v))
        to_float = float
    except ImportError:
        exact = lambda v: Fraction(float(v))
        to_float = float
    rng = np.random.default_rng(5)
    for mean, sigma in PARAMS + [(0.75, 0.375), (-2.0, 0.0625), (5.5, 3.0)]:
        p = GaussianPrior(mean, sigma)
        assert (p.mean, p.sigma) == (mean, sigma)
        xs = np.round((mean + sigma * rng.uniform(-30, 30, 200)) * 1024) / 1024          # dyadic
        got = p.slope(xs)
        assert got.shape == xs.shape
        for x, g in zip(xs, got):
            want = -(exact(x) - exact(mean)) / (exact(sigma) * exact(sigma))
            assert abs(exact(g) - want) <= 2 * EPS * abs(want), (mean, sigma, x)
            assert p.slope(float(x)) == g
        want = -1 / (exact(sigma) * exact(sigma))
        assert abs(exact(p.curvature) - want) <= 2 * EPS * abs(want)
        assert to_float(want) < 0
        # the slope is the derivative of the value: a central difference agrees to its own accuracy
        h = 1e-5 * sigma
        assert abs((p(mean + sigma + h) - p(mean + sigma - h)) / (2 * h) - p.slope(mean + sigma)) <= 1e-6 / sigma


@pytest.mark.parametrize('sigma', [0.0, -1.0, float('inf'), float('nan'), -float('inf'), 'wide', None])
def test_bad_sigma_raises(sigma):
    with pytest.raises(InvalidParameterSpecification):
        GaussianPrior(1.0, sigma)


def test_bad_mean_raises_and_it_is_exported():
    import blueice_amd
    from blueice_amd import priors
    with pytest.raises(InvalidParameterSpecification):
        GaussianPrior(float('nan'), 1.0)
    assert blueice_amd.GaussianPrior is priors.GaussianPrior and callable(GaussianPrior(0, 1))


def small_lf(likelihood_config=None):
    from blueice_amd.likelihood import LogLikelihoodBase
    from blueice_amd.test_helpers import conf_for_test
    return LogLikelihoodBase(conf_for_test(events_per_day=1), likelihood_config=likelihood_config, some_mode='b')


# (as in the reference, add_shape_uncertainty needs a base_value: a non-numeric setting, its anchors a dict z -> setting)
MODES = {1.0: 'a', 2.0: 'b', 3.0: 'c'}


def test_config_key_switches_what_the_uncertainty_methods_register():
    lf = small_lf(dict(gaussian_priors_on_device=True))
    name = lf.source_name_list[0]
    lf.add_rate_uncertainty(name, 0.3)
    lf.add_shape_uncertainty('some_mode', 0.25, anchor_zs=MODES, base_value=2.0)
    rate = lf.rate_parameters[name]
    anchors, shape, base = lf.shape_parameters['some_mode']
    assert isinstance(rate, GaussianPrior) and (rate.mean, rate.sigma) == (1.0, 0.3)
    assert isinstance(shape, GaussianPrior) and base == 2.0 and (shape.mean, shape.sigma) == (2.0, 0.5)
    assert anchors == MODES


@pytest.mark.parametrize('config', [None, {}, dict(gaussian_priors_on_device=False)])
def test_default_registers_scipys_bound_method(config):
    lf = small_lf(config)
    name = lf.source_name_list[0]
    lf.add_rate_uncertainty(name, 0.3)
    lf.add_shape_uncertainty('some_mode', 0.25, anchor_zs=MODES, base_value=2.0)
    for prior, frozen in ((lf.rate_parameters[name], stats.norm(1, 0.3)), (lf.shape_parameters['some_mode'][1], stats.norm(2.0, 0.5))):
        assert not isinstance(prior, GaussianPrior)
        assert getattr(prior, '__name__', None) == 'logpdf' and isinstance(prior.__self__, type(frozen))
        assert prior(1.234) == frozen.logpdf(1.234)


def test_host_helpers_take_the_closed_forms():
    """_prior_of, _prior_slope and prior_derivatives: no differences for a GaussianPrior (the results are exact where a
    difference is not), today's differences for any other callable"""
    from blueice_amd.hessian import prior_derivatives
    from blueice_amd.likelihood import DeviceLogLikelihood, _prior_of
    p, frozen = GaussianPrior(0.5, 0.4), stats.norm(0.5, 0.4).logpdf
    x = np.linspace(-1.0, 2.0, 31)
    assert np.array_equal(_prior_of(p, x), p(x))
    assert DeviceLogLikelihood._prior_slope(p, 0.9) == p.slope(0.9)
    slope, curv = prior_derivatives(p, x)
    assert np.array_equal(slope, p.slope(x)) and np.all(curv == p.curvature) and curv.shape == x.shape
    # the other callables: central differences, as before -- close to, and not equal to, the closed forms
    s2, c2 = prior_derivatives(frozen, x)
    assert np.allclose(s2, slope, rtol=1e-6, atol=1e-8) and np.allclose(c2, curv, rtol=1e-4) and not np.array_equal(s2, slope)
    h = 1e-6 * max(1.0, 0.9)
    assert DeviceLogLikelihood._prior_slope(frozen, 0.9) == (frozen(0.9 + h) - frozen(0.9 - h)) / (2 * h)


def test_gaussian_terms_split_constants_and_fixed_parameters():
    """what BatchObjective.native() hands to the native loops: mean / sigma on the floating variables, and per problem the
    normalisation constants of those plus the complete priors of the fixed parameters -- together, the prior"""
    from collections import OrderedDict
    from types import SimpleNamespace
    from blueice_amd.priors import gaussian_terms
    ps, pr = GaussianPrior(0.5, 0.4), GaussianPrior(1.0, 0.3)
    lf = SimpleNamespace(shape_parameters=OrderedDict(shift=({}, ps, None), stretch=({}, None, None)), source_name_list=['s0', 's1'],
                         rate_parameters=OrderedDict(s0=None, s1=pr))
    z = np.array([[0.1, 1.0], [0.7, 2.0]])
    mult = np.array([[1.0, 0.8], [1.0, 1.3]])
    mean, sigma, const = gaussian_terms(lf, ['s0_rate_multiplier', 's1_rate_multiplier', 'stretch'], z, mult)
    assert np.array_equal(mean, [0, 1.0, 0]) and np.array_equal(sigma, [np.inf, 0.3, np.inf])
    assert np.allclose(const, pr.log_norm + ps(z[:, 0]), rtol=1e-15)
    x = 0.9
    t = (x - mean[1]) / sigma[1]
    assert np.allclose(const - 0.5 * t * t, pr(x) + ps(z[:, 0]), rtol=1e-15)
    mean, sigma, const = gaussian_terms(lf, ['shift'], z, mult)
    assert np.array_equal(mean, [0.5]) and np.array_equal(sigma, [0.4]) and np.allclose(const, ps.log_norm + pr(mult[:, 1]), rtol=1e-15)


def test_the_two_entry_points_are_declared_exported_and_bound():
    """as tests/test_capi_loads.py: the header declares them, the library exports them, the ctypes table binds them with three
    more pointers than the entry points without terms"""
    import os
    import re
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'blueice_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(bi_[a-z_0-9]+)\s*\(', text))
    for name, plain in (('bi_fit_batched_gauss', 'bi_fit_batched'), ('bi_sample_stretch_gauss', 'bi_sample_stretch')):
        assert name in declared and plain in declared
        assert hasattr(lib, name) and hasattr(lib, plain)
        assert len(_capi.SIGNATURES[name][1]) == len(_capi.SIGNATURES[plain][1]) + 3
        assert _capi.SIGNATURES[name][0] is _capi.SIGNATURES[plain][0]
