"""The device ensemble sampler (bi_sample_stretch) and what is built on it: every half-step of the native engine replayed
from the device's own previous state against the independent oracle (tests/sampler_oracle.py) and the CPU likelihood
oracle, the known posterior for both engines, reproducibility, ensembles over toy datasets, the refusals, and the
likelihoods that take the host engine."""
import numpy as np
import pytest
from scipy import stats

import sampler_oracle as so
from golden_util import load_case
from oracle import blueice_oracle as orc

pytestmark = pytest.mark.gpu


def make_ctx(c, sparse=1):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    if c['kind'] == 1 or c['name'].startswith('unb_'):
        n_ev = c['bins'][0]
        ctx.begin_model(c['model']['anchor_z'], c['S'], n_ev)
        ps = c['model']['ps'].reshape((-1, c['S'], n_ev))
        mus = c['model']['mus'].reshape((-1, c['S']))
        for a in range(len(mus)):
            ctx.set_anchor(a, ps[a], mus[a])
        ctx.end_model()
        ctx.set_unbinned(c['outlier'])
        return ctx
    ctx.set_param('sparse', sparse)
    bb = c['bb_source']
    ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'], n_model=c['model']['n_model'] if bb >= 0 else None, bb_source=bb)
    if c.get('allow_negative') is not None and any(c['allow_negative']):
        ctx.set_allow_negative([1 if a else 0 for a in c['allow_negative']])
    ctx.upload_counts(c['counts'])
    return ctx


def variables_of(c, F):
    """the first F of (rate multipliers of every source, then every shape parameter) -> kind, index, lo, hi"""
    d, S = c['d'], c['S']
    kind = np.array([1] * S + [0] * d, dtype=np.int32)[:F]
    index = np.array(list(range(S)) + list(range(d)), dtype=np.int32)[:F]
    lo = np.array([0.0] * S + [float(g[0]) for g in c['model']['anchor_z']])[:F]
    hi = np.array([np.inf] * S + [float(g[-1]) for g in c['model']['anchor_z']])[:F]
    return kind, index, lo, hi


def oracle_of(c, kind, index, z0, scale0):
    unbinned = c['name'].startswith('unb_')

    def ll_of(pts):
        z = np.tile(z0, (len(pts), 1))
        rs = np.tile(scale0, (len(pts), 1))
        for v, (k, i) in enumerate(zip(kind, index)):
            if k == 0:
                z[:, i] = pts[:, v]
            else:
                rs[:, i] = pts[:, v]
        if unbinned:
            return np.array([orc.loglikelihood_unbinned(c['model'], zz, rr, c['outlier']) for zz, rr in zip(z, rs)])
        return orc.loglikelihood_batch(c['model'], c['counts'], z, rs, bb_source=c['bb_source'] if c['bb_source'] >= 0 else None,
                                       allow_negative=c['allow_negative'])
    return ll_of


def start_of(c, kind, index, W, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for k, i in zip(kind, index):
        if k == 0:
            g = c['model']['anchor_z'][i]
            cols.append(0.5 * (g[0] + g[-1]) + (g[-1] - g[0]) * rng.uniform(-0.1, 0.1, W))
        else:
            cols.append(rng.uniform(0.9, 1.1, W))
    return np.stack(cols, axis=1)


CASES = [('d2_nonuniform', 1), ('c1_like', 1), ('d3_small', 0), ('d3_small', 2), ('unb_shape_2src', 1), ('bb_d2', 1)]


@pytest.mark.parametrize('W', [8, 64])
@pytest.mark.parametrize('name, sparse', CASES)
def test_native_engine_replays(name, sparse, W):
    """Every half-step replayed from the device's own previous state: positions bitwise the old one or the oracle's proposal,
    recorded ll within 1e-10 max(1, |ll|) of the CPU oracle, decisions the oracle's outside the band
    m = 2e-10 max(1, |ll(y)|, |ll(x)|) + 1e-12 (F - 1) |log z|; at most 0.1 % of a test's decisions inside the band."""
    from blueice_amd.exceptions import PlannerRefused
    c = load_case(name)
    ctx = make_ctx(c, sparse)
    d, S = c['d'], c['S']
    z0 = np.array([0.5 * (g[0] + g[-1]) for g in c['model']['anchor_z']], dtype=float)
    scale0 = unit = np.ones(S)
    steps = 40 if W == 8 else 6
    total = band = 0
    try:
        for F in range(1, d + S + 1):
            kind, index, lo, hi = variables_of(c, F)
            x0 = start_of(c, kind, index, W, 100 + F)
            try:
                chain, ll, n_acc, counters = ctx.sample_stretch(W, kind, index, z0, scale0, unit, None, x0[None], lo, hi, steps, a=2.0, seed=42 + F)
            except PlannerRefused as e:
                assert name == 'bb_d2' and 'exact totals' in str(e)          # the one refusal this list may meet
                continue
            assert chain.shape == (steps, 1, W, F) and counters[0] == 2 * steps and counters[1] == W + steps * W
            n_dec, n_band, n_accepted = so.replay(chain[:, 0], ll[:, 0], x0, oracle_of(c, kind, index, z0, scale0), lo, hi, seed=42 + F, a=2.0)
            print('%s sparse=%d W=%d F=%d: %d decisions, %d in the band, %d accepted' % (name, sparse, W, F, n_dec, n_band, n_accepted))
            assert n_accepted == n_acc.sum() == counters[2] and n_accepted > 0
            assert np.all((chain >= lo) & (chain <= hi))
            total += n_dec
            band += n_band
        if total == 0:
            pytest.skip('the resident planner refuses every batch of %s (exact Beeston-Barlow totals): nothing to replay' % name)
        assert band <= 1e-3 * total
        assert ctx.get_param('n_sampler_half_steps') >= (2 * steps if total else 0)
    finally:
        ctx.close()


def gamma_likelihood(counts=(50.0, 20.0), **rate_priors):
    """two sources that each fill their own bin with one expected event per unit multiplier: mu_s ~ Gamma(n_s + 1, 1)"""
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


def check_gamma(samples, counts):
    for s, n in enumerate(counts):
        mean, var = samples[:, s].mean(), samples[:, s].var()
        print('source %d: mean %.3f (want %.1f), variance %.3f' % (s, mean, n + 1, var))
        assert abs(mean - (n + 1)) <= 0.15 * np.sqrt(n + 1)
        assert 0.8 * (n + 1) <= var <= 1.2 * (n + 1)


@pytest.mark.parametrize('engine', ['native', 'host'])
def test_known_posterior(engine):
    lf = gamma_likelihood()
    res = lf.sample_posterior(n_walkers=32, n_steps=1200, seed=5, guess=GUESS, engine=engine)
    assert res.engine == engine and res.chain.shape == (1200, 32, 2)
    check_gamma(res.flat(discard=200), (50, 20))


def test_bestfit_emcee_on_the_device():
    lf = gamma_likelihood()
    kw = dict(quiet=True, n_walkers=32, n_steps=1200, n_burn_in=200, seed=3, guess=GUESS)
    best, ll, err = lf.bestfit_emcee(return_errors=True, **kw)
    best2, ll2, samples = lf.bestfit_emcee(return_samples=True, **kw)
    best3, ll3 = lf.bestfit_emcee(**kw)
    assert best == best2 == best3 and ll == ll2 == ll3 == lf(**best) and samples.shape == (32 * 1000, 2)
    for s, n in enumerate((50, 20)):
        dist, key = stats.gamma(n + 1), 's%d_rate_multiplier' % s
        lo, hi = dist.ppf(stats.norm.cdf([-1, 1]))
        assert abs(best[key] - dist.median()) <= 0.15 * np.sqrt(n + 1)
        assert 0.8 <= (err[key] / ((hi - lo) / 2)) ** 2 <= 1.2


def test_same_seed_same_chain_and_bounds():
    lf = gamma_likelihood()
    a = lf.sample_posterior(n_walkers=8, n_steps=50, seed=1, guess=GUESS)
    b = lf.sample_posterior(n_walkers=8, n_steps=50, seed=1, guess=GUESS)
    c = lf.sample_posterior(n_walkers=8, n_steps=50, seed=2, guess=GUESS)
    assert a.engine == 'native'
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_prob, b.log_prob) and not np.array_equal(a.chain, c.chain)
    # walkers started next to the lower bound of a rate: proposals below it are never stored
    low = lf.sample_posterior(n_walkers=16, n_steps=100, seed=4, p0=np.random.default_rng(0).uniform(0.01, 3.0, (16, 2)))
    assert np.all(low.chain >= 0) and np.all(np.isfinite(low.log_prob))


def test_ensembles_over_toys_equal_solo_runs():
    import model_zoo
    from collections import OrderedDict
    ns = model_zoo.namespace_of('blueice_amd')
    space = [('x', np.linspace(0, 1, 13)), ('y', np.linspace(0, 1, 9))]
    lf = model_zoo.morph_lf(ns, np.random.default_rng(8), 2, space, OrderedDict(shift=(-1., 0., 1.)), 4000, 300)
    lf.simulate_toys(3, seed=12)
    p0 = np.random.default_rng(1).uniform(0.9, 1.1, (8, 3)) * np.array([1.0, 1.0, 0.0]) + np.array([0, 0, 1]) * np.random.default_rng(2).uniform(-0.3, 0.3, (8, 1))
    joint = lf.sample_posterior(n_walkers=8, n_steps=30, seed=6, p0=p0, datasets=[0, 1, 2])
    assert joint.engine == 'native' and joint.chain.shape == (30, 3, 8, 3)
    for e in range(3):
        solo = lf.sample_posterior(n_walkers=8, n_steps=30, seed=6, p0=p0, datasets=[e], first_ensemble=e)
        assert np.array_equal(solo.chain[:, 0], joint.chain[:, e]) and np.array_equal(solo.log_prob[:, 0], joint.log_prob[:, e])
    assert not np.array_equal(joint.chain[:, 0], joint.chain[:, 1])


def test_refusals():
    lf = gamma_likelihood()
    ctx = lf.ctx
    kind, index = np.array([1, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    lo, hi, one = np.zeros(2), np.full(2, np.inf), np.ones(2)
    x0 = np.random.default_rng(0).uniform(40, 60, (1, 8, 2))
    args = lambda x: (kind, index, np.zeros(0), one, one, None, x, lo, hi)
    with pytest.raises(ValueError, match='even number of walkers'):
        ctx.sample_stretch(7, *args(x0[:, :7]), 5)
    with pytest.raises(ValueError, match='even number of walkers'):
        ctx.sample_stretch(0, *args(x0[:, :0]), 5)
    with pytest.raises(ValueError, match='must be > 1'):
        ctx.sample_stretch(8, *args(x0), 5, a=1.0)
    bad = x0.copy()
    bad[0, 3, 1] = 0.0                                                         # inside the box, likelihood zero
    with pytest.raises(ValueError, match='start walker 3 of ensemble 0 is not finite'):
        ctx.sample_stretch(8, *args(bad), 5)
    bad[0, 3, 1] = -2.0
    with pytest.raises(ValueError, match='start walker 3 of ensemble 0 lies outside'):
        ctx.sample_stretch(8, *args(bad), 5)
    with pytest.raises(ValueError, match='start walker 3 of ensemble 0 lies outside the bounds'):
        lf.sample_posterior(n_walkers=8, n_steps=5, p0=bad[0])
    lib, h = ctx._lib, ctx._h
    from blueice_amd._capi import ptr
    tiny, nacc = np.zeros(8), np.zeros(8, dtype=np.int64)
    # 2^31 steps of 8 walkers: a chain of 412 GB; refused before any buffer is touched
    assert lib.bi_sample_stretch(h, 1, 8, 2, ptr(kind), ptr(index), None, ptr(one), ptr(one), None, ptr(x0), ptr(lo), ptr(hi), 2 ** 31, 2.0, 0, 0,
                                 ptr(tiny), ptr(tiny), ptr(nacc), None) == -4
    assert b'larger than the free device memory' in lib.bi_last_error(h)
    with pytest.raises(ValueError, match='neither a shape parameter nor a rate multiplier'):
        ctx.sample_stretch(8, np.array([0, 1], dtype=np.int32), index, np.zeros(0), one, one, None, x0, lo, hi, 5)
    assert lib.bi_sample_stretch(h, 1, 8, 0, None, None, None, None, None, None, None, None, None, 5, 2.0, 0, 0, None, None, None, None) == -1
    assert b'F >= 1' in lib.bi_last_error(h)
    # the context still works
    chain, ll, n_acc, _ = ctx.sample_stretch(8, *args(x0), 5)
    assert np.all(np.isfinite(ll))


def prior_replay(lf, res, p0, seed):
    names = res.names
    bounds = [lf.get_bounds(n) for n in names]
    lo, hi = np.array([b[0] for b in bounds], dtype=float), np.array([b[1] for b in bounds], dtype=float)
    ll_of = lambda pts: np.asarray(lf.eval_points({n: pts[:, v] for v, n in enumerate(names)}), dtype=float)
    return so.replay(res.chain, res.log_prob, p0, ll_of, lo, hi, seed=seed, a=2.0, ll_rtol=0.0, band_abs=0.0, band_log=0.0)


def test_priors_and_sums_take_the_host_engine():
    """a Python prior or a sum of likelihoods sits between the parameters and the device call: host engine, replayed against
    lf.eval_points (priors included) with a band of zero"""
    from blueice_amd.likelihood import LogLikelihoodSum
    lf = gamma_likelihood(s1=stats.norm(21.0, 2.0).logpdf)
    p0 = np.random.default_rng(3).uniform(0.95, 1.05, (8, 2)) * np.array([51.0, 21.0])
    res = lf.sample_posterior(n_walkers=8, n_steps=25, seed=8, p0=p0)
    assert res.engine == 'host'
    n_dec, n_band, n_acc = prior_replay(lf, res, p0, 8)
    assert n_dec == 200 and n_band == 0 and n_acc == res.n_accepted.sum() > 0
    with pytest.raises(ValueError, match="engine='host'"):
        lf.sample_posterior(n_walkers=8, n_steps=5, p0=p0, engine='native')
    both = LogLikelihoodSum([gamma_likelihood(), gamma_likelihood((45.0, 25.0))])
    res = both.sample_posterior(n_walkers=8, n_steps=25, seed=9, p0=p0)
    assert res.engine == 'host'
    n_dec, n_band, n_acc = prior_replay(both, res, p0, 9)
    assert n_dec == 200 and n_band == 0 and n_acc > 0


def test_infinite_rate_of_a_negative_source_is_refused_and_answered_on_the_host():
    """the resident planner's other refusal: a source that may go negative at an infinite rate -- PlannerRefused from the
    device call (a ValueError, flagged by the context, not recognised by its text), the host engine from sample_posterior"""
    from blueice_amd.exceptions import PlannerRefused
    c = load_case('neg_allowed')
    assert any(c['allow_negative'])
    ctx = make_ctx(c)
    try:
        S, d = c['S'], c['d']
        neg = int(np.flatnonzero(c['allow_negative'])[0])
        floating = [s for s in range(S) if s != neg][:1]
        kind, index = np.array([1], dtype=np.int32), np.array(floating, dtype=np.int32)
        z0 = np.array([0.5 * (g[0] + g[-1]) for g in c['model']['anchor_z']], dtype=float)
        scale0 = np.ones(S)
        x0 = np.random.default_rng(0).uniform(0.9, 1.1, (1, 8, 1))
        lo, hi = np.zeros(1), np.full(1, np.inf)
        chain, ll, _, _ = ctx.sample_stretch(8, kind, index, z0, scale0, np.ones(S), None, x0, lo, hi, 4)
        assert np.all(np.isfinite(ll)) and ctx.get_param('last_plan_refused') == 0
        scale0[neg] = np.inf
        with pytest.raises(PlannerRefused, match='infinite rate') as info:
            ctx.sample_stretch(8, kind, index, z0, scale0, np.ones(S), None, x0, lo, hi, 4)
        assert isinstance(info.value, ValueError) and ctx.get_param('last_plan_refused') == 2
        with pytest.raises(ValueError, match='even number of walkers') as info:      # an ordinary refusal right after: not a planner one
            ctx.sample_stretch(7, kind, index, z0, scale0, np.ones(S), None, x0[:, :7], lo, hi, 4)
        assert not isinstance(info.value, PlannerRefused)
    finally:
        ctx.close()
