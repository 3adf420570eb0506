"""The planner, the ensemble sampler and the gridded likelihood on the event store of a source-wise model
(bi_eval_sourcewise_events_planned, bi_sample_stretch_sourcewise_events, bi_grid_reduce_sourcewise_events; the event variant of
k_sourcewise_plan in front of k_sourcewise_events).

Everything the device planner decides is compared EXACTLY: `eval_events_planned` against `eval` (bi_eval_factored on the store) in
ll and status, the sampler's chain, log densities and acceptance counters against the host engine (blueice_amd.sampler._host_engine,
one bi_eval_factored call per half-step) on the same store, the grid's outputs over one chunk against blueice_amd.grid.reduce_cells
of the planned values.  Chunks that split a cell, and the native grid against the host engine, are held to test_grid_gpu.close's
2e-10 max(1, |profile|) with identical argmax and excluded counts, as tests/test_sourcewise_grid_gpu.py holds the binned model.
The same holds through the likelihood (sample_posterior(engine='native') against engine='host'), with and without GaussianPrior
constraints.

The matrix-core scan route does not read the event store: route 1 is refused, route -1 takes route 0."""
import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_toy_cases as toy_cases
from test_grid_gpu import close
from test_sourcewise_events_gpu import CLASSES, LENGTHS, OUTLIER, event_model, uploaded
from test_sourcewise_grid_gpu import INDEX, KIND, N_KEEP, grid_points
from test_sourcewise_sampler_gpu import bits, box_of, class_case, planner_points, points_of, start_of, variable_sets

pytestmark = pytest.mark.gpu

ST_OOB, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16


def assert_planned_is_eval(ctx, z, rs, ds):
    ll, st = ctx.eval(z, rs, ds)
    ll2, st2 = ctx.eval_events_planned(z, rs, ds)
    assert np.array_equal(st2, st)
    assert np.array_equal(bits(ll2), bits(ll))
    assert np.all(ll[st != 0] == -np.inf)
    return ll, st


# ---- the planned route ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CLASSES)
def test_planned_is_eval_at_every_class_and_set_length(name):
    """one store of six sets, one of every length in LENGTHS (one tile of padding alone, one event, a few, a full tile, a tile and an
    event, two tiles and an event): points on every anchor, on and one ulp outside the box edge, nan, every kind of unphysical
    rate, dataset indices -1 and ev_T, spread over all sets in ONE call"""
    own = class_case(name)[0]['own']
    rng = np.random.default_rng(sum(name.encode()) + 9)
    T = len(LENGTHS)
    model = event_model(rng, (2, 2, 2, 2), own, sum(LENGTHS))
    ctx = uploaded(model, LENGTHS)
    try:
        z, rs, ds, _ = planner_points(model, T, 150, 5 + len(name))
        ds[:2 * T] = np.tile(np.arange(T), 2)                   # (points on anchors, at every length)
        ll, st = assert_planned_is_eval(ctx, z, rs, ds)
        assert set(np.unique(st)) == {0, ST_OOB, ST_UNPHYSICAL, ST_BAD_DATASET}
        live = st == 0
        assert np.count_nonzero(live) >= 80 and set(ds[live]) == set(range(T)) and np.all(np.isfinite(ll[live]))
        assert ctx.get_param('last_morph_nbx') == 3             # the most blocks any set of the store takes
        # NULL rate scales and datasets, single points of every set, and a repeated call
        a, b = ctx.eval_events_planned(z[:7]), ctx.eval(z[:7])
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
        for t in range(T):
            p = int(np.flatnonzero(live & (ds == t))[0])
            one, st1 = ctx.eval_events_planned(z[p:p + 1], rs[p:p + 1], ds[p:p + 1])
            assert bits(one)[0] == bits(ll)[p] and st1[0] == 0
        again, _ = ctx.eval_events_planned(z, rs, ds)
        assert np.array_equal(bits(again), bits(ll))
        assert ctx._dev._lib.bi_eval_sourcewise_events_planned(ctx._dev._h, 0, None, None, None, None, None) == 0       # P = 0
    finally:
        ctx.close()


def test_planned_set_by_set_and_a_store_of_one_set():
    """three sets of different lengths in one call: a point has the bits it has on a store that holds its set alone (the grid's
    x is then the set's own block count, not the store's)"""
    n = [3, 1200, 513]
    own = class_case('mixed')[0]['own']
    rng = np.random.default_rng(45)
    model = event_model(rng, (2, 2, 2, 2), own, sum(n))
    off = np.concatenate([[0], np.cumsum(n)])
    ctx = uploaded(model, n)
    try:
        z, rs = toy_cases.box_points(model, rng, 30)
        ds = rng.integers(0, 3, 30)
        ll, st = assert_planned_is_eval(ctx, z, rs, ds)
        assert not st.any() and ctx.get_param('last_morph_nbx') == 3
        for t in (0, 2):
            alone = {k: [p[..., off[t]:off[t + 1]] for p in v] if k == 'ps' else v for k, v in model.items()}
            solo = uploaded(alone)
            pick = np.flatnonzero(ds == t)
            got, _ = solo.eval_events_planned(z[pick], rs[pick])
            assert np.array_equal(bits(got), bits(ll[pick])) and solo.get_param('last_morph_nbx') == -(-n[t] // 512)
            solo.close()
    finally:
        ctx.close()


def test_planned_on_a_set_longer_than_the_blocks_of_an_item():
    """1026 tiles of events on the 1024 blocks of an item, a rejected point between two live ones"""
    N = 1026 * 512 - 100
    rng = np.random.default_rng(1026)
    model = event_model(rng, (2, 2), [(0,), (1,)], N, zero_quarter=())
    z, rs = toy_cases.box_points(model, rng, 3)
    z[1, 0] = model['anchor_z'][0][-1] + 1.0
    ctx = uploaded(model)
    try:
        ll, st = assert_planned_is_eval(ctx, z, rs, None)
        assert st.tolist() == [0, ST_OOB, 0] and np.isfinite(ll[[0, 2]]).all() and ctx.get_param('last_morph_nbx') == 1024
    finally:
        ctx.close()


# ---- the sampler ------------------------------------------------------------------------------------------------------------

class StoreLikelihood:
    """what blueice_amd.sampler._host_engine asks of a likelihood, over a context's event store: variables 'v0', 'v1', ... written
    into (z0, scale0, unit) as the library's variable map does, bi_eval_factored, and the constraint terms in the header's order --
    p = const of the entry; per variable with a finite sigma t = (x - mean) / sigma, p = p - 0.5 (t t); then ll + p"""

    def __init__(self, ctx, kind, index, z0, scale0, unit, priors, const_of_dataset):
        self.ctx, self.kind, self.index, self.z0, self.scale0, self.unit = ctx, kind, index, z0, scale0, unit
        self.priors, self.const_of_dataset = priors, const_of_dataset

    def eval_points(self, call, livetime_days=None, dataset=None):
        x = np.stack([call['v%d' % v] for v in range(len(self.kind))], axis=1)
        z, rs = points_of(x, self.kind, self.index, self.z0, self.scale0, self.unit)
        ll, st = self.ctx.eval(z, rs, dataset)
        if self.priors is None:
            return ll
        mean, sigma = self.priors
        p = np.array([self.const_of_dataset[int(t)] for t in dataset])
        for v in np.flatnonzero(np.isfinite(sigma)):
            t = (x[:, v] - mean[v]) / sigma[v]
            p = p - 0.5 * (t * t)
        return ll + p


@pytest.fixture(scope='module')
def sampler_store():
    """class <4, 2> over two event sets of 300 and 37 events"""
    own = class_case('s4_e2')[0]['own']
    rng = np.random.default_rng(4300)
    model = event_model(rng, (2, 2, 2, 2), own, 337)
    ctx = uploaded(model, [300, 37])
    yield model, ctx
    ctx.close()


@pytest.mark.parametrize('with_terms', [False, True])
@pytest.mark.parametrize('W', [4, 8])
def test_sampler_is_the_host_engine_on_the_store(sampler_store, W, with_terms):
    from blueice_amd.sampler import _host_engine
    model, ctx = sampler_store
    d, S = ctx.d, ctx.S
    kind, index = variable_sets(d, S)['all']
    F, steps, seed, first = len(kind), 3, 17 + W, 2
    z0 = np.array([0.5 * (g[0] + g[-1]) for g in model['anchor_z']])
    scale0, unit = np.ones(S), np.full(S, 1.25)
    lo, hi = box_of(model, kind, index)
    datasets = np.array([1, 0], dtype=np.int64)                 # two ensembles over two sets
    x0 = np.stack([start_of(model, kind, index, W, 100 + e) for e in range(2)])
    x0[:, :, kind == 1] /= 1.25
    priors = None
    const_of = {}
    if with_terms:
        mean = np.where(kind == 1, 0.8, z0[np.minimum(index, d - 1)])
        sigma = np.full(F, np.inf)
        sigma[[0, 2, S, S + 3]] = [0.2, 0.1, 0.5, 0.3]
        const = np.array([-3.25, 0.75])
        priors = (mean, sigma, const)
        const_of = {1: const[0], 0: const[1]}
    before = ctx.get_param('n_sampler_half_steps')
    chain, lp, n_acc, counters = ctx.sample_stretch_events(W, kind, index, z0, scale0, unit, datasets, x0, lo, hi, steps, a=2.0, seed=seed,
                                                           first_ensemble=first, priors=priors)
    assert chain.shape == (steps, 2, W, F) and lp.shape == (steps, 2, W) and n_acc.shape == (2, W) and len(counters) == 5
    half = W // 2
    assert counters[0] == 2 * steps and counters[1] == 2 * W + 2 * steps * 2 * half and counters[2] == n_acc.sum()
    assert counters[4] == 0                                     # the step loop waits for nothing
    assert counters[3] == 3 * (2 * steps + 1)                   # planner, event kernel, finish: one sub-batch per half-step and the start
    assert ctx.get_param('n_sampler_half_steps') == before + 2 * steps
    lf = StoreLikelihood(ctx, kind, index, z0, scale0, unit, priors and priors[:2], const_of)
    names = ['v%d' % v for v in range(F)]
    want_chain, want_lp, want_acc, _ = _host_engine(lf, names, {}, None, datasets, x0.copy(), lo, hi, steps, 2.0, seed, first)
    print('W=%d terms=%s: %d of %d moves accepted' % (W, with_terms, n_acc.sum(), 2 * W * steps))
    assert np.array_equal(bits(chain), bits(want_chain)) and np.array_equal(bits(lp), bits(want_lp)) and np.array_equal(n_acc, want_acc)
    assert n_acc.sum() > 0 and np.all(np.isfinite(lp))
    again = ctx.sample_stretch_events(W, kind, index, z0, scale0, unit, datasets, x0, lo, hi, steps, a=2.0, seed=seed, first_ensemble=first,
                                      priors=priors)
    assert np.array_equal(bits(again[0]), bits(chain)) and np.array_equal(bits(again[1]), bits(lp))
    # first_ensemble shifts the stream: ensemble 1 of the call is ensemble first + 1 of the seed's stream whatever E is
    solo = ctx.sample_stretch_events(W, kind, index, z0, scale0, unit, datasets[1:], x0[1:], lo, hi, steps, a=2.0, seed=seed,
                                     first_ensemble=first + 1, priors=None if priors is None else (priors[0], priors[1], priors[2][1:]))
    assert np.array_equal(bits(solo[0][:, 0]), bits(chain[:, 1])) and np.array_equal(bits(solo[1][:, 0]), bits(lp[:, 1]))
    other = ctx.sample_stretch_events(W, kind, index, z0, scale0, unit, datasets[1:], x0[1:], lo, hi, steps, a=2.0, seed=seed,
                                      first_ensemble=first, priors=None if priors is None else (priors[0], priors[1], priors[2][1:]))
    assert not np.array_equal(other[0][:, 0], chain[:, 1])


def unbinned_nuisance_lf(priors=False, **likelihood_config):
    """tests/test_sourcewise_sampler_gpu.nuisance_lf's model as an unbinned likelihood: eight nuisances of five anchors, four histogram
    sources of two own parameters, scored on the device"""
    from blueice_amd import GaussianPrior, SourceWiseUnbinnedLogLikelihood
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5), source_class=NuisanceHistogramSource)
    lf = SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False, **likelihood_config))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.3) if priors and s == 1 else None)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.) if priors else None)
    lf.prepare()
    np.random.seed(21)
    lf.set_datasets([lf.base_model.simulate() for _ in range(2)])
    return lf, names


@pytest.mark.parametrize('priors', [False, True])
def test_sample_posterior_native_is_host(priors):
    from blueice_amd import inference
    from blueice_amd.sampler import sample_posterior
    lf, names = unbinned_nuisance_lf(priors)
    try:
        assert type(lf.ctx).__name__ == 'SourceWiseContext' and lf.last_scoring_route == 'device'
        for W in (4, 8):
            rng = np.random.default_rng(W)
            _, free, _, _ = lf.make_objective(minus=False)
            p0 = np.array([rng.uniform(0.9, 1.1, W) if n.endswith('_rate_multiplier') else rng.uniform(-0.3, 0.3, W) for n in free]).T
            kw = dict(n_walkers=W, n_steps=3, seed=6, p0=p0, datasets=[1, 0], first_ensemble=3)
            nat = sample_posterior(lf, engine='native', **kw)
            host = sample_posterior(lf, engine='host', **kw)
            assert nat.engine == 'native' and host.engine == 'host' and nat.chain.shape == (3, 2, W, 12) and nat.counters[4] == 0
            assert sample_posterior(lf, **kw).engine == 'native'
            worst = np.abs(nat.log_prob - host.log_prob).max()
            print('priors=%s W=%d: %d accepted, worst |log_prob difference| %.3g' % (priors, W, nat.n_accepted.sum(), worst))
            assert np.array_equal(bits(nat.chain), bits(host.chain)) and np.array_equal(nat.n_accepted, host.n_accepted)
            assert np.array_equal(bits(nat.log_prob), bits(host.log_prob))
        best, value = inference.bestfit_emcee(lf, quiet=True, n_walkers=8, n_steps=6, n_burn_in=2, seed=1, p0=p0)
        assert list(best) == free and value == lf(**best)
        for name in ('sample_posterior', 'bestfit_emcee', 'grid_scan'):
            with pytest.raises(NotImplementedError, match='unbinned source-wise model'):
                getattr(lf, name)()
    finally:
        lf.ctx.close()


# ---- the grid ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def grid_case():
    """test_sourcewise_grid_gpu's grid -- 2 kept nodes x 5 x 4 reduced nodes over toy_cases' small geometry, one node of axis 0 below
    its first anchor, a prior and a weight of zero -- over two event sets of 600 and 40 events"""
    rng = np.random.default_rng(2025)
    model = event_model(rng, toy_cases.N_ANCHOR, toy_cases.OWN, 640)
    g = model['anchor_z']
    nodes = [np.array([0.7, 1.3]), np.array([g[0][0] - 0.5, g[0][0], 0.5 * (g[0][0] + g[0][1]), g[0][1], g[0][2]]),
             np.array([0.5, 0.9, 1.2, 1.6])]
    term = [rng.normal(0.0, 1.5, len(v)) for v in nodes]
    logw = [rng.normal(0.0, 1.0, len(v)) for v in nodes]
    term[2][1] = -np.inf
    logw[1][3] = -np.inf
    z0 = np.array([[0.0, 0.5 * (g[1][0] + g[1][1]), 0.3 * g[2][0] + 0.7 * g[2][2]]] * 2)
    z0[1, 2] = g[2][3]
    scale0 = np.array([[1.0, 1.0, 0.8], [1.0, 1.0, 1.1]])
    unit = np.array([[1.0, 1.1, 1.0], [0.9, 1.0, 1.0]])
    return dict(model=model, n=[600, 40], nodes=nodes, term=term, logw=logw, z0=z0, scale0=scale0, unit=unit,
                datasets=np.array([1, 0], dtype=np.int64))


def run_grid(ctx, c, route, chunk=0):
    return ctx.grid_reduce_events(KIND, INDEX, c['z0'], c['scale0'], c['unit'], c['datasets'], N_KEEP, c['nodes'], term=c['term'],
                                  logw=c['logw'], chunk=chunk, route=route)


def test_grid_route_points(grid_case):
    from blueice_amd.grid import reduce_cells
    c = grid_case
    ctx = uploaded(c['model'], c['n'])
    try:
        z, rs, ds, p, q = grid_points(c)
        ll, st = ctx.eval_events_planned(z, rs, ds)
        assert set(np.unique(st)) == {0, 1} and np.count_nonzero(st) == 2 * 2 * 4 and np.all(np.isfinite(ll[st == 0]))
        with np.errstate(invalid='ignore'):
            t = np.where((st != 0) | (ll == -np.inf) | (p == -np.inf), -np.inf, ll + p).reshape(4, 20)
        wlm, wprof, warg, wexcl = reduce_cells(t, q.reshape(4, 20))
        klm, kprof, karg = ctx._dev.selftest_grid_reduce(t, q.reshape(4, 20))
        lm, prof, arg, counters = run_grid(ctx, c, 0)
        assert lm.shape == prof.shape == arg.shape == (2, 2) and list(counters) == [1, 80, wexcl, counters[3], 0]
        assert counters[3] == 3                                 # planner, event kernel, finish
        assert wexcl == 2 * 2 * 4 + 2 * 2 * 4 and np.all(warg >= 0)
        assert np.array_equal(bits(prof.ravel()), bits(wprof)) and np.array_equal(arg.ravel(), warg)
        assert np.array_equal(bits(prof.ravel()), bits(kprof)) and np.array_equal(arg.ravel(), karg)
        assert np.array_equal(bits(lm.ravel()), bits(klm))
        assert np.array_equal(bits(lm.ravel()), bits(wlm))
        again = run_grid(ctx, c, 0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (lm, prof, arg)))
        scale = np.abs(wprof).reshape(2, 2)
        for chunk in (7, 64, 80, 1000):                         # 7 and 64 split cells of 20 points
            lm2, prof2, arg2, counters2 = run_grid(ctx, c, 0, chunk)
            assert counters2[0] == -(-80 // min(chunk, 80)) and list(counters2[1:3]) == [80, wexcl] and counters2[4] == 0
            err = np.abs(lm2 - lm) / np.maximum(1.0, scale)
            print('chunk %d: log_marginal against one chunk: max error %.3g of the bound' % (chunk, err.max() / 2e-10))
            assert close(prof2, prof, scale) and close(lm2, lm, scale) and np.array_equal(arg2, arg)
            if chunk >= 80:
                assert all(a.tobytes() == b.tobytes() for a, b in zip((lm2, prof2, arg2), (lm, prof, arg)))
        # route -1 is route 0 on an event store; route 1 does not exist for it
        auto = run_grid(ctx, c, -1)
        assert auto[3][4] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(auto[:3], (lm, prof, arg)))
        with pytest.raises(ValueError, match='bi_grid_reduce_sourcewise_events: route 1 is not available.*event store'):
            run_grid(ctx, c, 1)
        for route in (2, -2):
            with pytest.raises(ValueError, match='bi_grid_reduce_sourcewise_events: route'):
                run_grid(ctx, c, route)
        bad = dict(c, datasets=np.array([2, 0], dtype=np.int64))            # ev_T = 2
        with pytest.raises(ValueError, match='bi_grid_reduce_sourcewise_events.*dataset 2 of entry 0'):
            run_grid(ctx, bad, 0)
        assert run_grid(ctx, c, 0)[0].tobytes() == lm.tobytes()             # the context still works
    finally:
        ctx.close()


def test_grid_scan_native_is_host():
    """blueice_amd.grid.grid_scan on the unbinned class, with priors, over two event sets: the native engine against the host engine
    (eval_points in chunks, reduce_cells), and the credible limit"""
    from blueice_amd import grid
    lf, names = unbinned_nuisance_lf(priors=True)
    try:
        axes = dict(keep=[('s0_rate_multiplier', np.linspace(0.0, 3.0, 7))],
                    reduce=[(names[0], np.linspace(-2.5, 2.0, 6)), ('s1_rate_multiplier', np.linspace(0.6, 1.4, 5))], datasets=[1, 0])
        axes[names[3]] = 0.25
        host = grid.grid_scan(lf, engine='host', **axes)
        assert host.engine == 'host' and host.excluded == 2 * 7 * 5
        scale = np.abs(host.profile)
        for setting in ('auto', 'points'):
            lf.config['sourcewise_grid_route'] = setting
            for chunk in (None, 50):
                nat = grid.grid_scan(lf, engine='native', chunk=chunk, **axes)
                assert nat.engine == 'native' and nat.counters[1] == 2 * 7 * 6 * 5 and nat.counters[4] == 0
                assert nat.excluded == host.excluded and np.array_equal(nat.argmax, host.argmax)
                for what in ('profile', 'log_marginal'):
                    err = np.abs(getattr(nat, what) - getattr(host, what)) / np.maximum(1.0, scale)
                    print('%s, chunk %s, %s: max error %.3g of the bound' % (setting, chunk, what, np.nanmax(err) / 2e-10))
                assert close(nat.profile, host.profile, scale) and close(nat.log_marginal, host.log_marginal, scale)
                assert all(np.array_equal(nat.best[k], host.best[k], equal_nan=True) for k in host.best)
        got, want = nat.credible_upper_limit(0.9), host.credible_upper_limit(0.9)
        assert got.shape == (2,) and np.all(np.abs(got - want) <= 2e-10 * np.maximum(1.0, np.abs(want)))
        assert grid.grid_scan(lf, **axes).engine == 'native'
        lf.config['sourcewise_grid_route'] = 'scan'
        with pytest.raises(ValueError, match='route 1 is not available'):
            grid.grid_scan(lf, engine='native', **axes)
    finally:
        lf.ctx.close()


# ---- state ------------------------------------------------------------------------------------------------------------------

def test_state():
    """without a store, or with an open one, each of the three calls is a state error; after drop_events the binned calls work"""
    from blueice_amd._capi import ptr
    from blueice_amd.exceptions import NotPreparedException
    model, counts = class_case('mixed')
    B = fo.n_bins(model)
    rng = np.random.default_rng(8)
    z, rs = toy_cases.box_points(model, rng, 3)
    ctx = toy_cases.upload(model, counts)
    try:
        before = ctx.eval_planned(z, rs)
        calls = {
            'bi_eval_sourcewise_events_planned': (lambda: ctx.eval_events_planned(z, rs), 'bi_eval_sourcewise_planned'),
            'bi_sample_stretch_sourcewise_events': (lambda: ctx.sample_stretch_events(2, [1], [0], z[0], rs[0], np.ones(ctx.S), None,
                                                                                      np.ones((1, 2, 1)), [0.0], [4.0], 1),
                                                    'bi_sample_stretch_sourcewise'),
            'bi_grid_reduce_sourcewise_events': (lambda: ctx.grid_reduce_events([1], [0], z[0], rs[0], np.ones(ctx.S), None, 1,
                                                                                [np.array([0.5, 1.0])]), 'bi_grid_reduce_sourcewise'),
        }
        for who, (call, binned) in calls.items():
            with pytest.raises(NotPreparedException, match='no event store') as info:
                call()
            assert who in str(info.value) and binned in str(info.value), (who, str(info.value))
        dev = ctx._dev
        n_ev = np.array([3], dtype=np.int64)
        dev._check(dev._lib.bi_sourcewise_events_begin(dev._h, 1, ptr(n_ev), OUTLIER))
        for who, (call, _) in calls.items():
            with pytest.raises(NotPreparedException, match='bi_sourcewise_events_end') as info:
                call()
            assert who in str(info.value)
        ctx.drop_events()
        edges = [np.arange(B + 1, dtype=float)]
        ctx.score_events('piecewise', edges, [[rng.integers(0, B, 40) + 0.5], [rng.integers(0, B, 7) + 0.5]], OUTLIER)
        ll, st = ctx.eval_events_planned(z, rs, np.array([0, 1, 2]))
        want, wst = ctx.eval(z, rs, np.array([0, 1, 2]))
        assert st.tolist() == wst.tolist() == [0, 0, ST_BAD_DATASET] and np.array_equal(bits(ll), bits(want))
        chain, lp, n_acc, counters = ctx.sample_stretch_events(2, [1], [0], z[0], rs[0], np.ones(ctx.S), [1], np.ones((1, 2, 1)), [0.0], [4.0], 2)
        assert np.all(np.isfinite(lp)) and counters[4] == 0
        ctx.drop_events()
        after = ctx.eval_planned(z, rs)
        assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(after[1], before[1])
        chain, lp, n_acc, counters = ctx.sample_stretch(2, [1], [0], z[0], rs[0], np.ones(ctx.S), None, np.ones((1, 2, 1)), [0.0], [4.0], 2)
        assert np.all(np.isfinite(lp))
        assert ctx.grid_reduce([1], [0], z[0], rs[0], np.ones(ctx.S), None, 1, [np.array([0.5, 1.0])])[3][1] == 2
    finally:
        ctx.close()
