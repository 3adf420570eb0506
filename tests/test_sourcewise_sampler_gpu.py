"""The device point planner of source-wise models (k_sourcewise_plan) and the ensemble sampler on it
(bi_eval_sourcewise_planned, bi_sample_stretch_sourcewise):

    the planner, bitwise     eval_planned against bi_eval_factored (values only) on every class of sourcewise_walk_cases' load_forms
                             -- and on a <4, 2> model built by the same recipe, which that family lacks -- at points on every anchor,
                             one ulp outside, nan, outside on an axis nobody owns, every kind of unphysical rate, bad datasets
    seams                    one item past the gridDim.y chunk and one past FacBatch::run's sub-batch, bitwise
    the sampler replays      sampler_oracle.replay with its default bands against factored_oracle's expectation and a Poisson sum
                             in long double; every recorded log_prob bit for bit bi_eval_factored at the recorded position
    reproducibility, ensembles over toys, the device copy of lgsum after new toys, constraint terms, a known posterior, refusals

No tolerance is defined here but replay's defaults and test_sampler_gpu.check_gamma's bounds."""
import numpy as np
import pytest
from scipy.special import gammaln

import batch_seam_cases as bsc
import factored_oracle as fo
import sampler_oracle as so
import sourcewise_toy_cases as toy_cases
import sourcewise_walk_cases as wc
from test_sampler_gpu import GUESS, check_gamma

pytestmark = pytest.mark.gpu

ST_OOB, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
OWN_4_2 = [(0, 1), (2,), (), (1, 3)]          # S = 4 source slots, at most two own axes: the class load_forms has no case of
NAMES = list(wc.FAMILIES['load_forms']) + ['s4_e2']


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def class_case(name):
    """-> (model, counts [3, B]): wc.make_case('load_forms', name), or its recipe on OWN_4_2; a third dataset beside its two"""
    if name != 's4_e2':
        c = wc.make_case('load_forms', name)
        model, counts = c.model, c.counts
    else:
        rng = np.random.default_rng(4242)
        model = fo.random_model(rng, (2, 2, 2, 2), OWN_4_2, wc.LOAD_B, zero_quarter=(1,))
        centre = np.array([0.5 * (g[0] + g[-1]) for g in model['anchor_z']])
        scale = wc.PER_BIN * wc.LOAD_B / fo.expectation(model, centre, np.ones(4)).sum()
        model['mus'] = [m * scale for m in model['mus']]
        z, rs = toy_cases.box_points(model, rng, 2)
        counts = rng.poisson(np.stack([fo.expectation(model, z[t], rs[t]) for t in range(2)])).astype(float)
    assert bsc.source_class(model['own']) == dict(s4_e2=(4, 2)).get(name, bsc.source_class(model['own']))
    return model, np.vstack([counts, counts[0][::-1]])


def planner_points(model, T, n_total, seed):
    """-> (z [P, d], rs [P, S], ds [P], expected status bits present): see the module's docstring"""
    rng = np.random.default_rng(seed)
    g = [np.asarray(a, dtype=float) for a in model['anchor_z']]
    d, S = len(g), len(model['own'])
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    owned = sorted({i for o in model['own'] for i in o})
    nobody = [i for i in range(d) if i not in owned]
    pts = []

    def add(z=None, rs=None, ds=None):
        zz = lo + (hi - lo) * rng.uniform(0.02, 0.98, d)
        rr = rng.uniform(0.5, 1.6, S)
        for i, v in (z or {}).items():
            zz[i] = v
        for s, v in (rs or {}).items():
            rr[s] = v
        pts.append((zz, rr, int(rng.integers(0, T)) if ds is None else ds))

    for i in owned:                                         # exactly on every anchor, the first and the last (closed) included
        for v in g[i]:
            add(z={i: v})
    for i in range(d):                                      # one ulp outside each end, owned or not
        add(z={i: np.nextafter(lo[i], -np.inf)})
        add(z={i: np.nextafter(hi[i], np.inf)})
        add(z={i: np.nan})
    for i in nobody:
        add(z={i: hi[i] + 1.0})
    for s in range(S):
        for v in (0.0, -1.0, np.inf, np.nan):
            add(rs={s: v})
    add(ds=-1)
    add(ds=T)
    add(z={0: np.nan} if d else None, ds=-1)                 # the order of the exits: the dataset first ...
    add(z={0: hi[0] + 1.0} if d else None, rs={0: -1.0})     # ... then the box, then the rates
    add(z={i: hi[i] for i in range(d)})                      # the upper corner of the box
    add(z={i: lo[i] for i in range(d)})
    while len(pts) < n_total:
        add()
    z = np.array([p[0] for p in pts]).reshape(len(pts), d)
    return z, np.array([p[1] for p in pts]), np.array([p[2] for p in pts], dtype=np.int64), bool(nobody)


def assert_planned_is_eval(ctx, z, rs, ds):
    ll, st = ctx.eval(z if ctx.d else None, rs, ds)
    ll2, st2 = ctx.eval_planned(z if ctx.d else None, rs, ds)
    assert np.array_equal(st2, st)
    assert np.array_equal(bits(ll2), bits(ll)) and np.array_equal(ll2, ll)
    assert np.all(ll[st != 0] == -np.inf)
    return ll, st


@pytest.mark.parametrize('name', NAMES)
def test_planner_bitwise(name):
    model, counts = class_case(name)
    ctx = toy_cases.upload(model, counts)
    try:
        z, rs, ds, has_nobody = planner_points(model, 3, 240, 11 + len(name))
        assert 200 <= len(z) <= 300
        if name in ('s2_e1', 's4_e1'):                      # axes nobody owns, and a source without own axes
            assert has_nobody and any(len(o) == 0 for o in model['own'])
        ll, st = assert_planned_is_eval(ctx, z, rs, ds)
        assert set(np.unique(st)) == {0, ST_OOB, ST_UNPHYSICAL, ST_BAD_DATASET}
        assert np.count_nonzero(st == 0) >= 150 and len(set(ds[st == 0])) == 3
        # NULL rate scales and datasets, a single point, and a repeated call
        ll1, st1 = ctx.eval_planned(z[:7])
        want1, wst1 = ctx.eval(z[:7])
        assert np.array_equal(bits(ll1), bits(want1)) and np.array_equal(st1, wst1)
        live = int(np.flatnonzero(st == 0)[0])
        one, _ = ctx.eval_planned(z[live:live + 1], rs[live:live + 1], ds[live:live + 1])
        assert bits(one)[0] == bits(ll)[live]
        again, _ = ctx.eval_planned(z, rs, ds)
        assert np.array_equal(bits(again), bits(ll))
    finally:
        ctx.close()


def test_planner_without_shape_axes_and_without_counts():
    from blueice_amd.exceptions import NotPreparedException
    rng = np.random.default_rng(3)
    model = fo.random_model(rng, (), [(), (), ()], 600)
    counts = rng.poisson(fo.expectation(model, np.zeros(0), np.ones(3))).astype(float)
    ctx = toy_cases.upload(model)
    try:
        with pytest.raises(NotPreparedException, match='no counts'):
            ctx.eval_planned(None, np.ones((2, 3)))
        ctx.set_counts(np.stack([counts, counts[::-1]]))
        z, rs, ds, _ = planner_points(model, 2, 40, 5)
        ll, st = assert_planned_is_eval(ctx, None, rs, ds)
        assert set(np.unique(st)) == {0, ST_UNPHYSICAL, ST_BAD_DATASET}
        assert ctx._dev._lib.bi_eval_sourcewise_planned(ctx._dev._h, 0, None, None, None, None, None) == 0      # P = 0
    finally:
        ctx.close()


@pytest.mark.parametrize('seam', ['item_chunk', 'sub_batch'])
def test_seams(seam):
    """one item past the gridDim.y chunk of a one-tile model; one past FacBatch::run's sub-batch of a 64-tile model"""
    rng = np.random.default_rng(77)
    if seam == 'item_chunk':
        B, P = bsc.B_TILE, bsc.ITEM_CHUNK + 1
        assert bsc.padded_bins(B) == bsc.TILE and P == 65536
    else:
        B = 64 * bsc.TILE
        P = bsc.per_call(B, 1) + 1
        assert bsc.padded_bins(B) // bsc.TILE == 64 and P == 131073
    model = fo.random_model(rng, (3,), [(0,), ()], B)
    scale = wc.PER_BIN * B / fo.expectation(model, np.array([0.0]), np.ones(2)).sum()
    model['mus'] = [m * scale for m in model['mus']]
    g = model['anchor_z'][0]
    counts = rng.poisson(fo.expectation(model, np.array([0.5 * (g[0] + g[-1])]), np.ones(2))).astype(float)
    ctx = toy_cases.upload(model, np.stack([counts, counts[::-1]]))
    try:
        z = rng.uniform(g[0], g[-1], (P, 1))
        rs = rng.uniform(0.5, 1.6, (P, 2))
        ds = rng.integers(0, 2, P)
        z[P - 1] = g[-1]                                    # the item behind the seam: on the closed last anchor
        ll, st = assert_planned_is_eval(ctx, z, rs, ds)     # (every point live: the host path crosses the same seam)
        assert not st.any() and np.all(np.isfinite(ll))
        assert ctx.get_param('last_point_pieces') == (2 if seam == 'item_chunk' else 4)
    finally:
        ctx.close()


# ---- the sampler ------------------------------------------------------------------------------------------------------------

def exact_ll(model, counts):
    """-> ll_of(z [n, d], rs [n, S]): factored_oracle's expectation, the Poisson sum in long double"""
    n = np.asarray(counts, dtype=float)
    lg = gammaln(n + 1).astype(np.longdouble)
    pos = n > 0

    def ll_of(z, rs):
        out = np.empty(len(z))
        for p in range(len(z)):
            mu = fo.expectation(model, z[p], rs[p]).astype(np.longdouble)
            with np.errstate(divide='ignore', invalid='ignore'):
                term = np.where(pos, n * np.log(np.where(pos, mu, 1.0)) - mu - lg, -mu)
                term = np.where(pos & (mu <= 0), -np.inf, term)
            out[p] = float(term.sum())
        return out
    return ll_of


def points_of(x, kind, index, z0, scale0, unit):
    """varmap_write_point: z0 / scale0 with the variables written in, a rate multiplier times its unit in one multiply"""
    z = np.tile(np.asarray(z0, dtype=float), (len(x), 1))
    rs = np.tile(np.asarray(scale0, dtype=float), (len(x), 1))
    for v, (k, i) in enumerate(zip(kind, index)):
        if k == 0:
            z[:, i] = x[:, v]
        else:
            rs[:, i] = x[:, v] * unit[i]
    return z, rs


def variable_sets(d, S):
    rate = (np.ones(S, dtype=np.int32), np.arange(S, dtype=np.int32))
    shape = (np.zeros(d, dtype=np.int32), np.arange(d, dtype=np.int32))
    return {'rates': rate, 'shapes': shape, 'all': tuple(np.concatenate(p) for p in zip(rate, shape))}


def box_of(model, kind, index):
    g = model['anchor_z']
    lo = np.array([0.0 if k else float(g[i][0]) for k, i in zip(kind, index)])
    hi = np.array([np.inf if k else float(g[i][-1]) for k, i in zip(kind, index)])
    return lo, hi


def start_of(model, kind, index, W, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for k, i in zip(kind, index):
        g = model['anchor_z'][i] if k == 0 else None
        cols.append(rng.uniform(0.9, 1.1, W) if k else 0.5 * (g[0] + g[-1]) + (g[-1] - g[0]) * rng.uniform(-0.1, 0.1, W))
    return np.stack(cols, axis=1)


_SAMPLER_CTX = {}


@pytest.fixture(scope='module')
def sampler_ctx():
    """one context and one oracle per model, shared by the replays"""
    def get(name):
        if name not in _SAMPLER_CTX:
            model, counts = class_case(name)
            _SAMPLER_CTX[name] = (model, counts, toy_cases.upload(model, counts), exact_ll(model, counts[0]))
        return _SAMPLER_CTX[name]
    yield get
    for _, _, ctx, _ in _SAMPLER_CTX.values():
        ctx.close()
    _SAMPLER_CTX.clear()


@pytest.mark.parametrize('W', [8, 64])
@pytest.mark.parametrize('which', ['rates', 'shapes', 'all'])
@pytest.mark.parametrize('name', ['s4_e1', 's4_e2', 'e3x8'])
def test_sampler_replays(sampler_ctx, name, which, W):
    model, counts, ctx, oracle = sampler_ctx(name)
    d, S = ctx.d, ctx.S
    assert bsc.source_class(model['own']) == {'s4_e1': (4, 1), 's4_e2': (4, 2), 'e3x8': (8, 3)}[name]
    kind, index = variable_sets(d, S)[which]
    F = len(kind)
    z0 = np.array([0.5 * (g[0] + g[-1]) for g in model['anchor_z']])
    scale0, unit = np.ones(S), np.full(S, 1.25)
    lo, hi = box_of(model, kind, index)
    steps = 40 if W == 8 else 6
    x0 = start_of(model, kind, index, W, 100 + F)
    x0[:, kind == 1] /= 1.25                                 # (rate scales around 1 at a unit of 1.25)
    seed = 42 + F
    before = ctx.get_param('n_sampler_half_steps')
    chain, ll, n_acc, counters = ctx.sample_stretch(W, kind, index, z0, scale0, unit, None, x0[None], lo, hi, steps, a=2.0, seed=seed)
    assert chain.shape == (steps, 1, W, F) and ll.shape == (steps, 1, W) and len(counters) == 5
    assert counters[0] == 2 * steps and counters[1] == W + steps * W and counters[4] == 0
    assert counters[3] == 3 * (2 * steps + 1)               # planner, evaluation, finish: one sub-batch per half-step and the start
    assert ctx.get_param('n_sampler_half_steps') == before + 2 * steps
    assert np.all((chain >= lo) & (chain <= hi))
    # every recorded log_prob is bi_eval_factored at the recorded position, bit for bit
    z, rs = points_of(chain.reshape(-1, F), kind, index, z0, scale0, unit)
    want, st = ctx.eval(z, rs)
    assert not st.any() and np.array_equal(bits(ll.reshape(-1)), bits(want))
    ll_of = lambda pts: oracle(*points_of(np.asarray(pts, dtype=float), kind, index, z0, scale0, unit))
    n_dec, n_band, n_accepted = so.replay(chain[:, 0], ll[:, 0], x0, ll_of, lo, hi, seed=seed, a=2.0)
    print('%s %s W=%d: %d decisions, %d in the band, %d accepted, max |ll| %.0f' % (name, which, W, n_dec, n_band, n_accepted, np.abs(ll).max()))
    assert np.abs(ll).max() < 1e4
    assert n_dec == steps * W and n_accepted == n_acc.sum() == counters[2] and n_accepted > 0
    assert n_band <= 1e-3 * n_dec


def nuisance_lf(priors=False):
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.3) if priors and s == 1 else None)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.) if priors else None)
    lf.prepare()
    return lf, names


def nuisance_start(lf, W, seed):
    _, names, guesses, _ = lf.make_objective(minus=False)
    rng = np.random.default_rng(seed)
    return np.array([rng.uniform(0.9, 1.1, W) if n.endswith('_rate_multiplier') else rng.uniform(-0.3, 0.3, W) for n in names]).T


def test_reproducible_ensembles_over_toys_and_fresh_lgsum():
    from blueice_amd.sampler import sample_posterior
    lf, names = nuisance_lf()
    truth = {names[0]: np.array([0.5]), 's0_rate_multiplier': np.array([1.2])}
    lf.simulate_toys_points(truth, 3, seed=12)
    p0 = nuisance_start(lf, 8, 1)
    kw = dict(n_walkers=8, n_steps=30, p0=p0)
    a = sample_posterior(lf, seed=6, datasets=[0, 1, 2], **kw)
    b = sample_posterior(lf, seed=6, datasets=[0, 1, 2], **kw)
    c = sample_posterior(lf, seed=7, datasets=[0, 1, 2], **kw)
    assert a.engine == 'native' and a.chain.shape == (30, 3, 8, 12) and a.counters[4] == 0
    assert np.array_equal(bits(a.chain), bits(b.chain)) and np.array_equal(bits(a.log_prob), bits(b.log_prob))
    assert not np.array_equal(a.chain, c.chain)
    for e in range(3):
        solo = sample_posterior(lf, seed=6, datasets=[e], first_ensemble=e, **kw)
        assert np.array_equal(bits(solo.chain[:, 0]), bits(a.chain[:, e])) and np.array_equal(bits(solo.log_prob[:, 0]), bits(a.log_prob[:, e]))
    assert not np.array_equal(a.chain[:, 0], a.chain[:, 1])
    # new toys between two calls: the planner subtracts the new datasets' sum lgamma(n + 1), as bi_eval_factored does
    lf.simulate_toys_points(truth, 3, seed=13)
    after = sample_posterior(lf, seed=6, datasets=[0, 1, 2], **kw)
    assert not np.array_equal(after.log_prob, a.log_prob)
    # (a stale sum would shift every log_prob of an ensemble by a constant of order 1 and leave the chain alone)
    pts = {n: after.chain[-1, 1, :, v] for v, n in enumerate(after.names)}
    want = lf.eval_points(pts, dataset=np.full(8, 1))
    assert np.allclose(after.log_prob[-1, 1], want, rtol=1e-12, atol=0)
    host = sample_posterior(lf, seed=6, datasets=[0, 1, 2], engine='host', **kw)
    assert host.engine == 'host' and host.chain.shape == a.chain.shape


def test_constraint_terms():
    """log_prob = ll + p with p summed in the header's order: p = const; per variable with a finite sigma t = (x - mean) / sigma,
    p = p - 0.5 (t t); the sum compared exactly"""
    from blueice_amd.sampler import sample_posterior
    model, counts = class_case('s4_e2')
    ctx = toy_cases.upload(model, counts)
    try:
        d, S = ctx.d, ctx.S
        kind, index = variable_sets(d, S)['all']
        F = len(kind)
        z0 = np.array([0.5 * (g[0] + g[-1]) for g in model['anchor_z']])
        one = np.ones(S)
        lo, hi = box_of(model, kind, index)
        x0 = start_of(model, kind, index, 16, 3)
        mean = np.where(kind == 1, 1.0, z0[np.minimum(index, d - 1)])
        sigma = np.full(F, np.inf)
        sigma[[0, 2, S, S + 3]] = [0.2, 0.1, 0.5, 0.3]
        const = np.array([-3.25])
        chain, lp, n_acc, counters = ctx.sample_stretch(16, kind, index, z0, one, one, None, x0[None], lo, hi, 20, seed=9,
                                                        priors=(mean, sigma, const))
        assert counters[4] == 0 and n_acc.sum() > 0
        x = chain.reshape(-1, F)
        ll, st = ctx.eval(*points_of(x, kind, index, z0, one, one))
        p = np.full(len(x), const[0])
        for v in np.flatnonzero(np.isfinite(sigma)):
            t = (x[:, v] - mean[v]) / sigma[v]
            p = p - 0.5 * (t * t)
        assert not st.any() and np.array_equal(bits(lp.reshape(-1)), bits(ll + p))
        free, _, _, _ = ctx.sample_stretch(16, kind, index, z0, one, one, None, x0[None], lo, hi, 20, seed=9)
        assert not np.array_equal(free, chain)
    finally:
        ctx.close()
    lf, names = nuisance_lf(priors=True)
    np.random.seed(5)
    lf.set_data(lf.base_model.simulate())
    res = sample_posterior(lf, n_walkers=24, n_steps=10, seed=2, p0=nuisance_start(lf, 24, 4))
    assert res.engine == 'native' and res.chain.shape == (10, 24, 12) and np.all(np.isfinite(res.log_prob))
    pts = {n: res.chain[-1, :, v] for v, n in enumerate(res.names)}
    assert np.allclose(res.log_prob[-1], lf.eval_points(pts), rtol=1e-12, atol=0)


def gamma_sourcewise(counts=(50.0, 20.0)):
    """test_sampler_gpu.gamma_likelihood's construction as a source-wise model"""
    from blueice_amd import SourceWiseBinnedLogLikelihood
    from blueice_amd.test_helpers import FixedSampleSource
    conf = dict(analysis_space=[['x', np.array([0.0, 1.0, 2.0])]], default_source_class=FixedSampleSource, livetime_days=1.0,
                force_recalculation=True, never_save_to_cache=True, sources=[])
    for s in range(2):
        data = np.zeros(10, dtype=[('x', float), ('source', int)])
        data['x'] = s + 0.5
        conf['sources'].append(dict(name='s%d' % s, events_per_day=1.0, data=data))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False))
    for s in range(2):
        lf.add_rate_parameter('s%d' % s)
    lf.prepare()
    lf.set_binned_data(np.array(counts))
    return lf


@pytest.mark.parametrize('engine', ['native', 'host'])
def test_known_posterior(engine):
    from blueice_amd.sampler import sample_posterior
    lf = gamma_sourcewise()
    res = sample_posterior(lf, n_walkers=32, n_steps=1200, seed=5, guess=GUESS, engine=engine)
    assert res.engine == engine and res.chain.shape == (1200, 32, 2)
    check_gamma(res.flat(discard=200), (50, 20))


def test_bestfit_emcee_as_a_function():
    from blueice_amd import inference
    lf = gamma_sourcewise()
    kw = dict(quiet=True, n_walkers=32, n_steps=300, n_burn_in=100, seed=3, guess=GUESS)
    best, ll, err = inference.bestfit_emcee(lf, return_errors=True, **kw)
    best2, ll2 = inference.bestfit_emcee(lf, **kw)
    assert best == best2 and ll == ll2 == lf(**best) and list(best) == ['s0_rate_multiplier', 's1_rate_multiplier'] and set(err) == set(best)
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.bestfit_emcee()
    assert 'blueice_amd.inference.bestfit_emcee(lf' in str(e.value)
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.sample_posterior()
    assert 'blueice_amd.sampler.sample_posterior(lf' in str(e.value)


def test_refusals():
    from blueice_amd.exceptions import NotPreparedException
    rng = np.random.default_rng(1)
    model = fo.random_model(rng, (3,), [(0,), ()], 63)
    g = model['anchor_z'][0]
    mid = 0.5 * (g[0] + g[-1])
    counts = rng.poisson(fo.expectation(model, np.array([mid]), np.ones(2))).astype(float)
    ctx = toy_cases.upload(model)
    try:
        kind, index = np.array([1, 0], dtype=np.int32), np.array([0, 0], dtype=np.int32)
        lo, hi, one = np.array([0.0, g[0]]), np.array([np.inf, g[-1]]), np.ones(2)
        x0 = np.stack([rng.uniform(0.9, 1.1, 8), rng.uniform(mid - 0.1, mid + 0.1, 8)], axis=1)[None]
        args = lambda x, k=kind, i=index: (k, i, np.array([mid]), one, one, None, x, lo, hi)
        with pytest.raises(NotPreparedException, match='no counts'):
            ctx.sample_stretch(8, *args(x0), 5)
        ctx.set_counts(counts)
        with pytest.raises(ValueError, match='bi_sample_stretch_sourcewise: the stretch move needs an even number of walkers'):
            ctx.sample_stretch(7, *args(x0[:, :7]), 5)
        with pytest.raises(ValueError, match='must be > 1'):
            ctx.sample_stretch(8, *args(x0), 5, a=1.0)
        with pytest.raises(ValueError, match='start walker 3 of ensemble 0 lies outside'):
            ctx.sample_stretch(8, *args(np.where(np.arange(8)[None, :, None] == 3, -2.0, x0)), 5)
        # a start walker of zero likelihood: both rates at zero where the data are not empty
        both = (np.array([1, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32))
        xr = rng.uniform(0.9, 1.1, (1, 8, 2))
        xr[0, 3] = 0.0
        assert counts.sum() > 0
        with pytest.raises(ValueError, match='the log likelihood of start walker 3 of ensemble 0 is not finite'):
            ctx.sample_stretch(8, both[0], both[1], np.array([mid]), one, one, None, xr, np.zeros(2), np.full(2, np.inf), 5)
        # var_index >= d of THIS model, although the context also holds a grid model of two axes
        S, B = 2, 63
        ps = rng.gamma(2.0, 1.0, (2, 2, S, B))
        ps /= ps.sum(axis=-1, keepdims=True)
        ctx._dev.upload_model([np.array([0.0, 1.0]), np.array([0.0, 1.0])], ps, np.full((2, 2, S), 100.0))
        with pytest.raises(ValueError, match='bi_sample_stretch_sourcewise: variable 1 is neither a shape parameter'):
            ctx.sample_stretch(8, *args(x0, kind, np.array([0, 1], dtype=np.int32)), 5)
        chain, ll, n_acc, counters = ctx.sample_stretch(8, *args(x0), 5)          # the context still works
        assert np.all(np.isfinite(ll)) and counters[0] == 10 and counters[4] == 0
    finally:
        ctx.close()
