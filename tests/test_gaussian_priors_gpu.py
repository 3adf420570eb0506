"""Gaussian constraint terms inside the native fit and sampler loops (bi_fit_batched_gauss, bi_sample_stretch_gauss): the
values against the REAL reference (tests/golden/constrained_d2.npz, made by tests/golden/make_golden_constrained.py), the
native fit against the numpy engine and the reference's per-point fits, the closed-form slopes and curvatures against the
unconstrained twin, toy fits, and every half-step of the native sampler replayed against the twin built with scipy callables
-- the host path that existed before, which knows nothing of the closed forms."""
import copy
import os
from collections import OrderedDict

import numpy as np
import pytest
from scipy import integrate, stats

import constrained_zoo as cz
import model_zoo
import sampler_oracle as so
from golden_util import GOLDEN_DIR, same

pytestmark = pytest.mark.gpu
TOL = 1e-6
FLOATING = ['s1_rate_multiplier', 'shift']                 # what floats in the profile of constrained_zoo.PROFILE_AXIS


def with_priors(lf, priors):
    """the same likelihood on the same device context with other priors: 'gaussian', 'scipy' or None"""
    from blueice_amd.priors import GaussianPrior
    twin = copy.copy(lf)
    if priors == 'gaussian':
        on_rate, on_shift = GaussianPrior(1, cz.RATE_SIGMA), GaussianPrior(cz.SHIFT_MEAN, cz.SHIFT_SIGMA)
    elif priors == 'scipy':
        on_rate, on_shift = stats.norm(1, cz.RATE_SIGMA).logpdf, stats.norm(cz.SHIFT_MEAN, cz.SHIFT_SIGMA).logpdf
    else:
        on_rate = on_shift = None
    twin.rate_parameters = OrderedDict((k, on_rate if k == 's1' else None) for k in lf.rate_parameters)
    twin.shape_parameters = OrderedDict((k, (v[0], on_shift if k == 'shift' else None, v[2])) for k, v in lf.shape_parameters.items())
    return twin


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN_DIR, 'constrained_d2.npz'))


@pytest.fixture(scope='module')
def trio(ns):
    """(constrained with GaussianPrior, the same with scipy callables, unconstrained) on one device context"""
    lf = cz.constrained_d2(ns, 'gaussian')
    return lf, with_priors(lf, 'scipy'), with_priors(lf, None)


@pytest.fixture(scope='module')
def toy_trio(ns):
    """the same three on a context of their own, which holds toy datasets"""
    lf = cz.constrained_d2(ns, 'gaussian')
    lf.simulate_toys(64, seed=3)
    return lf, with_priors(lf, 'scipy'), with_priors(lf, None)


class Spy:
    """wraps a bound method: counts the calls and keeps the keyword arguments and the counters array of the last one"""

    def __init__(self, owner, name):
        self.owner, self.name, self.inner = owner, name, getattr(owner, name)
        self.calls, self.kwargs, self.args = 0, None, None

    def __enter__(self):
        def wrapper(*args, **kwargs):
            self.calls += 1
            self.args, self.kwargs = args, kwargs
            return self.inner(*args, **kwargs)
        setattr(self.owner, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        delattr(self.owner, self.name)                     # (the wrapper was an instance attribute over the class's method)


# ------------------------------------------------------------------------------------------------------------------------
# 1. values
# ------------------------------------------------------------------------------------------------------------------------
def test_values_reproduce_the_reference(trio, golden):
    lf, lf_scipy, _ = trio
    calls = cz.calls()
    want = golden['constrained_ll']
    assert len(calls) == len(want) >= 40 and np.isinf(want).sum() >= 4
    for kw, w in zip(calls, want):
        got = lf(**kw)
        print(kw, got, w)
        assert same(got, w, 1e-10), (kw, got, w)
        assert same(lf_scipy(**kw), w, 1e-10)
    # the batched form: every call without a live time of its own, as arrays
    rows = np.flatnonzero(np.isnan(golden['call_livetime']))
    pts = {n: golden['call_z'][rows, i] for i, n in enumerate(lf.shape_parameters)}
    pts.update({'%s_rate_multiplier' % s: golden['call_mult'][rows, j] for j, s in enumerate(lf.source_name_list)})
    got = lf.eval_points(pts)
    for g, w in zip(got, want[rows]):
        assert same(g, w, 1e-10), (g, w)
    assert np.array_equal(np.isinf(got), np.isinf(want[rows]))
    # the closed form and scipy's: the same prior to a few roundings
    both = np.isfinite(got)
    assert np.all(np.abs(got - lf_scipy.eval_points(pts))[both] <= 1e-13 * np.abs(got[both]))


# ------------------------------------------------------------------------------------------------------------------------
# 2. the native fit
# ------------------------------------------------------------------------------------------------------------------------
def test_native_objective_carries_the_terms(trio):
    from blueice_amd import profile
    from blueice_amd.priors import GaussianPrior
    lf, lf_scipy, twin = trio
    name, grid = cz.PROFILE_AXIS
    nat = profile.BatchObjective(lf, FLOATING, {name: grid}, cz.PROFILE_FIXED).native()
    assert nat is not None and nat['P'] == len(grid)
    assert np.array_equal(nat['prior_mean'], [1.0, cz.SHIFT_MEAN]) and np.array_equal(nat['prior_sigma'], [cz.RATE_SIGMA, cz.SHIFT_SIGMA])
    norm = GaussianPrior(1, cz.RATE_SIGMA).log_norm + GaussianPrior(cz.SHIFT_MEAN, cz.SHIFT_SIGMA).log_norm
    assert nat['prior_const'].shape == (len(grid),) and np.allclose(nat['prior_const'], norm, rtol=1e-15)
    # a constrained parameter that is held fixed: its whole prior is a constant of the problem
    nat = profile.BatchObjective(lf, ['s0_rate_multiplier', 'shift'], {'s1_rate_multiplier': np.array([0.7, 1.2])}, cz.PROFILE_FIXED).native()
    assert np.array_equal(nat['prior_sigma'], [np.inf, cz.SHIFT_SIGMA])
    want = GaussianPrior(cz.SHIFT_MEAN, cz.SHIFT_SIGMA).log_norm + GaussianPrior(1, cz.RATE_SIGMA)(np.array([0.7, 1.2]))
    assert np.allclose(nat['prior_const'], want, rtol=1e-15)
    # no terms at all, and any other callable
    nat = profile.BatchObjective(twin, FLOATING, {name: grid}, cz.PROFILE_FIXED).native()
    assert nat is not None and np.all(np.isinf(nat['prior_sigma'])) and np.all(nat['prior_const'] == 0)
    assert profile.BatchObjective(lf_scipy, FLOATING, {name: grid}, cz.PROFILE_FIXED).native() is None


def test_native_fit_is_taken_and_agrees(trio, golden):
    from blueice_amd import profile
    lf, _, _ = trio
    name, grid = cz.PROFILE_AXIS
    assert str(golden['profile_axis_name']) == name and np.array_equal(golden['profile_axis_values'], grid)
    assert [str(x) for x in golden['profile_fixed_names']] == list(cz.PROFILE_FIXED)
    out = {}
    for engine in ('native', 'numpy'):
        profile.ENGINE = engine
        try:
            with Spy(lf, 'eval_points') as points, Spy(lf.ctx, 'fit_batched') as fit:
                out[engine] = lf.bestfit_batched(points={name: grid}, return_info=True, **cz.PROFILE_FIXED)
            if engine == 'native':
                # the C++ loop with the device objective ran, with the terms, and nothing evaluated the likelihood from Python
                assert fit.calls > 0 and fit.kwargs.get('priors') is not None
                counters = fit.args[18]
                print('bi_fit_batched_gauss: counters', counters)
                assert counters.shape == (4,) and counters[1] > 0 and counters[3] > 0
                assert points.calls == 0
            else:
                assert fit.calls == 0
        finally:
            profile.ENGINE = 'native'
    (ba, la, ia), (bb, lb, ib) = out['native'], out['numpy']
    assert list(ba) == [str(x) for x in golden['profile_float_names']] == FLOATING
    assert ia['analytic_gradient'] and not ia['failed'].any() and (ia['converged'] | ia['stalled']).all()
    print('native - numpy: ll', np.max(np.abs(la - lb) / np.abs(lb)), {k: np.max(np.abs(ba[k] - bb[k])) for k in ba})
    np.testing.assert_allclose(la, lb, rtol=1e-9)
    for k in ba:
        np.testing.assert_allclose(ba[k], bb[k], rtol=1e-5, atol=1e-6)
    # the reference's own fits, point by point: never below them, and equal wherever its tol = 1e-10 fit exists
    ref, ref_default = golden['profile_ll'], golden['profile_ll_default']
    have, have_default = np.isfinite(ref), np.isfinite(ref_default)
    assert have.sum() >= 55
    scale = np.maximum(1.0, np.abs(ref))
    print('engine - reference: largest gain %.3e, largest loss %.3e' % (np.nanmax(la - ref), np.nanmax(ref - la)))
    assert np.all((la >= ref - TOL * scale)[have])
    assert np.all((la >= ref_default - TOL * scale)[have_default])
    assert np.all((np.abs(la - ref) <= TOL * scale)[have])
    # the global fit
    best, ll = lf.bestfit_batched(**cz.PROFILE_FIXED)
    gll = float(golden['global_ll'])
    print('global fit: engine %.9f, reference %.9f' % (ll[0], gll))
    assert ll[0] >= gll - TOL * abs(gll)
    assert list(best) == [str(x) for x in golden['global_names']]


# ------------------------------------------------------------------------------------------------------------------------
# 3. gradient and Hessian
# ------------------------------------------------------------------------------------------------------------------------
def interior_points(P, seed):
    rng = np.random.default_rng(seed)
    return OrderedDict([('s0_rate_multiplier', rng.uniform(0.3, 2.0, P)), ('s1_rate_multiplier', rng.uniform(0.3, 2.0, P)),
                        ('s2_rate_multiplier', rng.uniform(0.3, 2.0, P)), ('shift', rng.uniform(-0.95, 1.95, P)),
                        ('stretch', rng.uniform(0.05, 3.95, P))])


def test_gradient_gains_the_closed_form_slope(trio):
    lf, _, twin = trio
    pts = interior_points(64, 1)
    ll, g = lf.values_and_gradients(pts)
    ll0, g0 = twin.values_and_gradients(pts)
    assert list(g) == list(g0) == list(pts) and np.all(np.isfinite(ll))
    priors = {'s1_rate_multiplier': lf.rate_parameters['s1'], 'shift': lf.shape_parameters['shift'][1]}
    for n in g:
        if n not in priors:
            assert np.array_equal(g[n].view(np.uint64), g0[n].view(np.uint64)), n
            continue
        # g = fl(g0 + slope): half an ulp of g, and half an ulp of the difference taken here
        want = priors[n].slope(pts[n])
        ulp = np.spacing(np.maximum(np.abs(g[n]), np.abs(g0[n])))
        err = np.abs((g[n] - g0[n]) - want)
        print(n, 'largest error %.2f ulp' % np.max(err / ulp))
        assert np.all(err <= 4 * ulp)
    assert np.allclose(ll - ll0, priors['shift'](pts['shift']) + priors['s1_rate_multiplier'](pts['s1_rate_multiplier']), rtol=0, atol=1e-12 * np.max(np.abs(ll)))
    # the scalar call
    kw = {k: float(v[0]) for k, v in pts.items()}
    l1, g1 = lf.value_and_gradient(**kw)
    l2, g2 = twin.value_and_gradient(**kw)
    for n, p in priors.items():
        assert abs((g1[n] - g2[n]) - p.slope(kw[n])) <= 4 * np.spacing(max(abs(g1[n]), abs(g2[n])))


def test_hessian_gains_the_closed_form_curvature(trio):
    lf, _, twin = trio
    pts = interior_points(48, 2)
    ll, g, names, H = lf.values_gradients_hessians(pts)
    ll0, g0, names0, H0 = twin.values_gradients_hessians(pts)
    assert lf.hessian_method == twin.hessian_method == 'analytic' and names == names0 == list(pts)
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(H0))
    constrained = {names.index('s1_rate_multiplier'): lf.rate_parameters['s1'], names.index('shift'): lf.shape_parameters['shift'][1]}
    other = np.ones(H.shape[1:], dtype=bool)
    for j, p in constrained.items():
        assert p.curvature == -1.0 / p.sigma ** 2
        err = np.abs((H[:, j, j] - H0[:, j, j]) - p.curvature)
        print(names[j], 'largest error %.2f ulp of the entry' % np.max(err / np.spacing(np.abs(H[:, j, j]))))
        assert np.all(err <= 2 * np.spacing(np.abs(H[:, j, j])))
        other[j, j] = False
    # every other entry saw one addition of zero
    assert np.array_equal(H[:, other].view(np.uint64), H0[:, other].view(np.uint64))


def test_minuit_errors_shrink_under_the_constraints(trio):
    lf, _, twin = trio
    res, ll = lf.bestfit_minuit(**cz.PROFILE_FIXED)
    res0, ll0 = twin.bestfit_minuit(**cz.PROFILE_FIXED)
    print(res, res0)
    for n in cz.CONSTRAINED:
        assert 0 < res[n + '_error'] < res0[n + '_error']


# ------------------------------------------------------------------------------------------------------------------------
# 4. toys
# ------------------------------------------------------------------------------------------------------------------------
def test_toy_fits_take_the_native_objective(toy_trio):
    from blueice_amd import profile
    lf, _, _ = toy_trio
    out = {}
    for engine in ('native', 'numpy'):
        profile.ENGINE = engine
        try:
            with Spy(lf.ctx, 'fit_batched') as fit:
                out[engine] = lf.bestfit_toys(**cz.PROFILE_FIXED)
            assert (fit.calls > 0 and fit.kwargs.get('priors') is not None) if engine == 'native' else fit.calls == 0
        finally:
            profile.ENGINE = 'native'
    (ba, la), (bb, lb) = out['native'], out['numpy']
    assert la.shape == lb.shape == (64,) and np.all(np.isfinite(la))
    print('toys: native - numpy ll in [%.3e, %.3e]' % (np.min(la - lb), np.max(la - lb)))
    assert np.all(la >= lb - 1e-9 * np.abs(lb))


# ------------------------------------------------------------------------------------------------------------------------
# 5. the sampler
# ------------------------------------------------------------------------------------------------------------------------
def gamma_likelihood(counts=(50.0, 20.0), **rate_priors):
    """two sources that each fill their own bin with one expected event per unit multiplier: mu_s ~ Gamma(n_s + 1, 1) x prior
    (the model of tests/test_sampler_gpu.py)"""
    from blueice_amd.likelihood import BinnedLogLikelihood
    from blueice_amd.test_helpers import FixedSampleSource
    conf = dict(analysis_space=[['x', np.array([0.0, 1.0, 2.0])]], default_source_class=FixedSampleSource, livetime_days=1.0,
                force_recalculation=True, never_save_to_cache=True, sources=[])
    for s in range(2):
        data = np.zeros(10, dtype=[('x', float), ('source', int)])
        data['x'] = s + 0.5
        conf['sources'].append(dict(name='s%d' % s, events_per_day=1.0, data=data))
    lf = BinnedLogLikelihood(conf)
    for s in range(2):
        lf.add_rate_parameter('s%d' % s, log_prior=rate_priors.get('s%d' % s))
    lf.prepare()
    lf.set_binned_data(np.array(counts))
    return lf


GUESS = {'s0_rate_multiplier': 51.0, 's1_rate_multiplier': 21.0}


def replay_against(trusted, res_chain, res_ll, names, p0, seed, ensemble=0, dataset=None):
    """sampler_oracle.replay with the oracle's own default bands; the log density is `trusted.eval_points`"""
    bounds = [trusted.get_bounds(n) for n in names]
    lo, hi = np.array([b[0] for b in bounds], dtype=float), np.array([b[1] for b in bounds], dtype=float)

    def ll_of(pts):
        more = {} if dataset is None else {'dataset': np.full(len(pts), dataset, dtype=np.int64)}
        return np.asarray(trusted.eval_points({n: pts[:, v] for v, n in enumerate(names)}, **more), dtype=float)

    return so.replay(res_chain, res_ll, p0, ll_of, lo, hi, seed=seed, a=2.0, ensemble=ensemble)


def d2_start(W, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.9, 1.1, W), rng.uniform(0.9, 1.1, W), rng.uniform(0.9, 1.1, W), rng.uniform(0.2, 0.8, W),
                     rng.uniform(1.2, 1.8, W)], axis=1)


def test_native_sampler_replays_against_the_scipy_twin(trio):
    """engine='native' on constrained likelihoods; every half-step replayed from the sampler's own previous state against the
    host path with scipy callables.  In-band decisions (|q| within 2e-10 max(1, |ll|) + ...) must stay below 1 % of all:
    with q spread over units, a decision falls inside a band of ~1e-8 about once in 1e8 -- the chosen seeds give none
    with the host engine on the CPU oracle."""
    from blueice_amd.priors import GaussianPrior
    total = band = 0
    lf = gamma_likelihood(s1=GaussianPrior(21.0, 2.0))
    trusted = gamma_likelihood(s1=stats.norm(21.0, 2.0).logpdf)
    p0 = np.random.default_rng(3).uniform(0.95, 1.05, (8, 2)) * np.array([51.0, 21.0])
    res = lf.sample_posterior(n_walkers=8, n_steps=25, seed=8, p0=p0, engine='native')
    assert res.engine == 'native' and res.chain.shape == (25, 8, 2)
    n_dec, n_band, n_acc = replay_against(trusted, res.chain, res.log_prob, res.names, p0, 8)
    print('gamma x normal: %d decisions, %d in the band, %d accepted' % (n_dec, n_band, n_acc))
    assert n_dec == 200 and n_acc == res.n_accepted.sum() == res.counters[2] > 0
    total, band = total + n_dec, band + n_band
    # without engine=: native as well
    assert lf.sample_posterior(n_walkers=8, n_steps=2, seed=8, p0=p0).engine == 'native'

    lf, lf_scipy, _ = trio
    p0 = d2_start(16, 4)
    res = lf.sample_posterior(n_walkers=16, n_steps=30, seed=9, p0=p0, engine='native')
    assert res.engine == 'native' and res.chain.shape == (30, 16, 5)
    n_dec, n_band, n_acc = replay_against(lf_scipy, res.chain, res.log_prob, res.names, p0, 9)
    print('d2 constrained: %d decisions, %d in the band, %d accepted' % (n_dec, n_band, n_acc))
    assert n_dec == 30 * 16 and n_acc == res.n_accepted.sum() > 0
    total, band = total + n_dec, band + n_band
    # two of the five held fixed, one of them constrained: its prior is a constant of the ensemble
    fixed = dict(s1_rate_multiplier=1.2, stretch=1.5)
    keep = [0, 2, 3]
    res = lf.sample_posterior(n_walkers=16, n_steps=20, seed=10, p0=p0[:, keep], engine='native', **fixed)
    assert res.engine == 'native' and res.names == ['s0_rate_multiplier', 's2_rate_multiplier', 'shift']
    bounds = [lf.get_bounds(n) for n in res.names]
    lo, hi = np.array([b[0] for b in bounds], dtype=float), np.array([b[1] for b in bounds], dtype=float)
    ll_of = lambda pts: np.asarray(lf_scipy.eval_points(dict({n: pts[:, v] for v, n in enumerate(res.names)}, **fixed)), dtype=float)
    n_dec, n_band, n_acc = so.replay(res.chain, res.log_prob, p0[:, keep], ll_of, lo, hi, seed=10, a=2.0)
    assert n_dec == 20 * 16 and n_acc > 0
    total, band = total + n_dec, band + n_band
    assert band <= 0.01 * total


def test_native_sampler_over_toys(toy_trio):
    lf, lf_scipy, _ = toy_trio
    p0 = d2_start(8, 6)
    res = lf.sample_posterior(n_walkers=8, n_steps=20, seed=11, p0=p0, datasets=np.arange(4), engine='native')
    assert res.engine == 'native' and res.chain.shape == (20, 4, 8, 5)
    for e in range(4):
        n_dec, n_band, n_acc = replay_against(lf_scipy, res.chain[:, e], res.log_prob[:, e], res.names, p0, 11, ensemble=e, dataset=e)
        print('toy %d: %d decisions, %d in the band, %d accepted' % (e, n_dec, n_band, n_acc))
        assert n_dec == 160 and n_acc == res.n_accepted[e].sum() > 0 and n_band <= 0.01 * n_dec
    assert not np.array_equal(res.chain[:, 0], res.chain[:, 1])


def test_no_terms_is_the_plain_sampler_bit_for_bit():
    lf = gamma_likelihood()
    ctx = lf.ctx
    kind, index = np.array([1, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    lo, hi, one = np.zeros(2), np.full(2, np.inf), np.ones(2)
    x0 = np.random.default_rng(0).uniform(40, 60, (2, 8, 2)) * np.array([1.0, 0.4])
    args = (8, kind, index, np.zeros(0), one, one, None, x0, lo, hi, 30)
    plain = ctx.sample_stretch(*args, seed=21)
    gauss = ctx.sample_stretch(*args, seed=21, priors=(np.zeros(2), np.full(2, np.inf), None))
    for a, b in zip(plain, gauss):
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b)
    assert plain[3][2] > 0
    # a constant alone shifts every log density by one addition and no decision... to rounding: the first rows agree
    shifted = ctx.sample_stretch(*args, seed=21, priors=(np.zeros(2), np.full(2, np.inf), np.array([0.0, 0.0])))
    assert np.array_equal(shifted[0][0], plain[0][0]) and np.array_equal(shifted[1][0], plain[1][0])


def test_posterior_mean_under_a_constraint():
    """mu_s1 ~ Gamma(21, 1) x Normal(21, 2): the mean of the chain within 5 standard errors (batch means) of the quadrature"""
    from blueice_amd.priors import GaussianPrior
    lf = gamma_likelihood(s1=GaussianPrior(21.0, 2.0))
    res = lf.sample_posterior(n_walkers=32, n_steps=1200, seed=5, guess=GUESS, engine='native')
    assert res.engine == 'native'
    dens = lambda m: np.exp(stats.gamma(21).logpdf(m) + stats.norm(21.0, 2.0).logpdf(m))
    norm = integrate.quad(dens, 0, 60, points=[21.0], epsabs=0, epsrel=1e-12)[0]
    exact = integrate.quad(lambda m: m * dens(m), 0, 60, points=[21.0], epsabs=0, epsrel=1e-12)[0] / norm
    series = res.chain[200:, :, 1].mean(axis=1)                       # the ensemble's mean after every step
    batches = series.reshape(20, 50).mean(axis=1)
    mean, se = series.mean(), batches.std(ddof=1) / np.sqrt(len(batches))
    print('mean of mu_s1: %.4f, exact %.4f, standard error %.4f (batch means)' % (mean, exact, se))
    assert 20.0 < exact < 21.5 and 0 < se < 0.2
    assert abs(mean - exact) <= 5 * se
    # the unconstrained source keeps its Gamma(51, 1)
    assert abs(res.chain[200:, :, 0].mean() - 51.0) <= 0.15 * np.sqrt(51.0)


# ------------------------------------------------------------------------------------------------------------------------
# 6. failure paths
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mean, sigma, const, why', [
    ([0.0, 21.0], [np.inf, 0.0], None, 'prior_sigma must be > 0'),
    ([0.0, 21.0], [np.inf, -2.0], None, 'prior_sigma must be > 0'),
    ([0.0, np.nan], [np.inf, 2.0], None, 'NaN in prior_mean'),
    ([0.0, 21.0], [np.nan, 2.0], None, 'NaN in prior_mean / prior_sigma'),
    ([0.0, 21.0], [np.inf, 2.0], [np.nan], 'NaN in prior_const'),
])
def test_bad_terms_are_refused_before_any_launch(mean, sigma, const, why):
    lf = gamma_likelihood()
    ctx = lf.ctx
    kind, index = np.array([1, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    lo, hi, one = np.zeros(2), np.full(2, np.inf), np.ones(2)
    x0 = np.random.default_rng(0).uniform(40, 60, (1, 8, 2)) * np.array([1.0, 0.4])
    priors = (np.array(mean), np.array(sigma), None if const is None else np.array(const))
    before = ctx.get_param('n_sampler_half_steps')
    with pytest.raises(ValueError, match='bi_sample_stretch_gauss: .*%s' % why):
        ctx.sample_stretch(8, kind, index, np.zeros(0), one, one, None, x0, lo, hi, 5, priors=priors)
    assert ctx.get_param('n_sampler_half_steps') == before
    x, f, flags, counters = np.full((1, 2), -7.0), np.full(1, -7.0), np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match='bi_fit_batched_gauss: .*%s' % why):
        ctx.fit_batched(1, 2, kind, index, None, one[None], one[None], None, x0[0, :1].copy(), lo, hi, None, None, 1e-6, 50, x, f, flags, counters,
                        priors=priors)
    assert np.all(counters == 0) and np.all(x == -7.0) and np.all(f == -7.0)
    # the context still works, with and without terms
    chain, ll, _, _ = ctx.sample_stretch(8, kind, index, np.zeros(0), one, one, None, x0, lo, hi, 3, priors=(np.array([0.0, 21.0]), np.array([np.inf, 2.0]), None))
    assert np.all(np.isfinite(ll))


def test_other_callables_still_take_the_host_engine():
    lf = gamma_likelihood(s1=lambda x: stats.norm(21.0, 2.0).logpdf(x))
    p0 = np.random.default_rng(3).uniform(0.95, 1.05, (8, 2)) * np.array([51.0, 21.0])
    assert lf.sample_posterior(n_walkers=8, n_steps=4, seed=8, p0=p0).engine == 'host'
    with pytest.raises(ValueError, match="engine='host'"):
        lf.sample_posterior(n_walkers=8, n_steps=4, p0=p0, engine='native')
