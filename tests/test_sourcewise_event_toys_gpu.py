"""Event-level toys of source-wise models drawn on the device (bi_sourcewise_simulate_event_toys; k_sourcewise_pmf,
k_sourcewise_sim_counts / _room / _first / _events) and the Python layers on top of them.

Every event of every replayed toy is compared with toy_oracle.simulate_events on the factored specification in NumPy
(sourcewise_event_toy_cases): source, bin, and position within 2 ulp and inside its bin; a draw whose comparison lies inside the
oracle's band is undecided and at most toy_oracle.CAP of the draws may be (on these cases none is: test_sourcewise_event_toys_host).
Everything else -- layouts, independence of the sub-batches and of the grouping into calls, the store against the store scored from
the downloaded events, the fits through the class -- is compared bit for bit."""
import numpy as np
import pytest

import sourcewise_event_toy_cases as cases
import sourcewise_events_oracle as eo
import sourcewise_toy_cases as toy_cases
import toy_oracle as to

pytestmark = pytest.mark.gpu

OUTLIER = 1e-12
TILE = cases.TILE


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def lookup(method, edges, coords=None):
    """-> (grid, coords) of `score_events`: the edges, or the bin centres with the coordinates clipped to the outer ones"""
    if method == 'piecewise':
        return edges, coords
    grid = [0.5 * (e[:-1] + e[1:]) for e in edges]
    return grid, None if coords is None else [np.clip(c, g[0], g[-1]) for c, g in zip(coords, grid)]


def split(ctx, coords, source):
    """the downloaded events set by set -> [(coords [k, N_t], source [N_t])]"""
    n = ctx.event_set_counts()
    first = np.concatenate([[0], np.cumsum(n)])
    return [(coords[:, first[t]:first[t + 1]], source[first[t]:first[t + 1]]) for t in range(len(n))]


def snapshot(ctx):
    """everything a call leaves behind, as bits: the events and the stored values of every set"""
    coords, source = ctx.download_events()
    n = ctx.event_set_counts()
    return dict(n=n.tolist(), coords=bits(coords).copy(), source=source.copy(), store=[bits(ctx.download_event_set(t)).copy() for t in range(len(n))])


def same(a, b):
    return a['n'] == b['n'] and np.array_equal(a['coords'], b['coords']) and np.array_equal(a['source'], b['source']) and \
        all(np.array_equal(x, y) for x, y in zip(a['store'], b['store']))


# ---- 1. replay ------------------------------------------------------------------------------------------------------------------

REPLAYS = [(name, method) for name in cases.SHAPES for method in ('piecewise', 'linear')] + [('class_' + c, 'piecewise') for c in cases.CLASSES]


@pytest.mark.parametrize('name,method', REPLAYS)
def test_every_event_of_every_toy_is_the_oracles(name, method):
    case = cases.make_case(name)
    dens = cases.densities_at(case['model'], case['z'][0])
    ctx = toy_cases.upload(case['model'])
    try:
        total = [0, 0]
        for off in cases.OFFSETS:
            ctx.set_param('toy_offset', off)
            counts = ctx.simulate_event_toys(method, case['edges'], case['z'], case['rs'], [cases.T_REPLAY], cases.SEED, OUTLIER)
            assert counts.shape == (cases.T_REPLAY, len(case['model']['own']))
            assert ctx.event_set_counts().tolist() == counts.sum(axis=1).tolist()
            assert ctx.simulated_event_count() == counts.sum()
            sets = split(ctx, *ctx.download_events())
            for t in range(cases.T_REPLAY):
                rep = cases.oracle_toy(case, 0, cases.SEED, off + t, dens)
                draws, undecided, _ = to.compare_events(counts[t], sets[t][0], sets[t][1], rep, what='%s %s toy %d' % (name, method, off + t))
                assert (counts[t] == rep.n).all()
                total[0] += draws
                total[1] += undecided
        print('%s %s: %d draws replayed, %d undecided' % (name, method, total[0], total[1]))
    finally:
        ctx.close()


# ---- 2. layout ------------------------------------------------------------------------------------------------------------------

def test_layout_of_empty_toys_and_of_sets_on_both_sides_of_a_tile():
    case = cases.make_case('k1', 2)
    model, z = case['model'], case['z']
    rs = np.array([cases.scale_for(model, z[0], cases.LAYOUT_RATES), np.zeros(4)])      # truth 1: rate_scale = 0, no events at all
    want = cases.layout_counts(case)
    ctx = toy_cases.upload(model)
    try:
        counts = ctx.simulate_event_toys('piecewise', case['edges'], z, rs, [cases.LAYOUT_TOYS, 2], cases.SEED, OUTLIER)
        assert np.array_equal(counts[:cases.LAYOUT_TOYS], want) and not counts[cases.LAYOUT_TOYS:].any()
        n = ctx.event_set_counts()
        assert n.tolist() == counts.sum(axis=1).tolist()
        assert n[:cases.LAYOUT_TOYS].min() < TILE < n[:cases.LAYOUT_TOYS].max() and n[-2:].tolist() == [0, 0]
        rows = sum(np.asarray(m).size for m in model['mus'])
        cols = int(np.maximum(TILE, (n + TILE - 1) // TILE * TILE).sum())             # whole tiles, at least one
        assert ctx.get_param('sourcewise_events_bytes') == rows * cols * 8 and ctx.get_param('sourcewise_event_sets') == len(n)
        coords, source = ctx.download_events()
        assert coords.shape == (1, n.sum()) and (source == 0).all()
        # an empty toy: one padded tile, masked by index -> ll = - sum_s r_s at any point, sources ascending from 0.0
        zp, rp = toy_cases.box_points(model, np.random.default_rng(3), 2)
        T = len(n)
        ll, st = ctx.eval(zp, rp, np.array([T - 1, T - 2]))
        assert not st.any()
        for p in range(2):
            lam = 0.0
            for r in cases.rates_at(model, zp[p], rp[p]):
                lam = lam + r
            print('empty toy: ll = %.17g, - sum r = %.17g' % (ll[p], -lam))
            assert ll[p] == -lam
        # ... and a set one event past a tile evaluates like the same events scored from the host
        t_long = int(np.argmax(n))
        sets = split(ctx, coords, source)
        other = toy_cases.upload(model)
        try:
            other.score_events('piecewise', case['edges'], [[sets[t_long][0][0]]], OUTLIER)
            a, b = ctx.eval_grad(zp, rp, np.full(2, t_long)), other.eval_grad(zp, rp, np.zeros(2, dtype=np.int64))
            for x, y in zip(a, b):
                assert np.array_equal(bits(x), bits(y))
        finally:
            other.close()
    finally:
        ctx.close()


# ---- 3. independence ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,method', [('k2', 'linear'), ('k1_B1025', 'piecewise')])
def test_toys_do_not_depend_on_sub_batches_or_on_the_grouping_into_calls(name, method):
    case = cases.make_case(name, 3)
    n_toys = [2, 0, 3]
    ctx = toy_cases.upload(case['model'])
    try:
        def draw(z, rs, n, offset=0, chunk=0):
            ctx.set_param('toy_offset', offset)
            ctx.set_param('sim_truth_chunk', chunk)
            counts = ctx.simulate_event_toys(method, case['edges'], z, rs, n, cases.SEED, OUTLIER)
            ctx.set_param('sim_truth_chunk', 0)
            return counts, snapshot(ctx)
        counts, whole = draw(case['z'], case['rs'], n_toys)
        assert whole['n'] == counts.sum(axis=1).tolist() and len(whole['n']) == 5
        for chunk in (1, 2):                                # a seam behind every truth; behind truth 1 (which has no toys)
            c2, snap = draw(case['z'], case['rs'], n_toys, chunk=chunk)
            assert np.array_equal(c2, counts) and same(snap, whole), chunk
        # one call of 5 toys = two calls split by toy_offset; a single-toy call at offset D = toy D of the ensemble
        first = np.concatenate([[0], np.cumsum(whole['n'])])
        k = len(case['edges'])
        whole_coords = whole['coords'].reshape(k, -1)
        parts = [draw(case['z'][:1], case['rs'][:1], [2]), draw(case['z'][2:], case['rs'][2:], [3], offset=2)]
        singles = [draw(case['z'][h:h + 1], case['rs'][h:h + 1], [1], offset=D) for D, h in enumerate([0, 0, 2, 2, 2])]
        for pieces, starts in ((parts, [0, 2]), (singles, range(5))):
            for (c, snap), t0 in zip(pieces, starts):
                t1 = t0 + len(snap['n'])
                assert np.array_equal(c, counts[t0:t1]) and snap['n'] == whole['n'][t0:t1]
                assert np.array_equal(snap['coords'].reshape(k, -1), whole_coords[:, first[t0]:first[t1]])
                assert np.array_equal(snap['source'], whole['source'][first[t0]:first[t1]])
                assert all(np.array_equal(x, y) for x, y in zip(snap['store'], whole['store'][t0:t1]))
        assert ctx.get_param('toy_offset') == 4
        ctx.set_param('toy_offset', 0)
    finally:
        ctx.close()


# ---- 4. the store -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,method', [('k1', 'piecewise'), ('k1', 'linear'), ('k2', 'piecewise'), ('k2', 'linear'), ('k3', 'linear')])
def test_the_store_is_the_store_scored_from_the_downloaded_events(name, method):
    case = cases.make_case(name, 2)
    model = case['model']
    ctx, other = toy_cases.upload(model), toy_cases.upload(model)
    try:
        ctx.simulate_event_toys(method, case['edges'], case['z'], case['rs'], [2, 1], cases.SEED, OUTLIER)
        sets = split(ctx, *ctx.download_events())
        grid, _ = lookup(method, case['edges'])
        other.score_events(method, grid, [lookup(method, case['edges'], list(c))[1] for c, _ in sets], OUTLIER)
        assert other.event_set_counts().tolist() == ctx.event_set_counts().tolist()
        zp, rp = toy_cases.box_points(model, np.random.default_rng(4), 3)
        for t in range(3):
            assert np.array_equal(bits(ctx.download_event_set(t)), bits(other.download_event_set(t))), (name, method, t)
            ds = np.full(3, t)
            assert np.array_equal(bits(ctx.eval(zp, rp, ds)[0]), bits(other.eval(zp, rp, ds)[0]))
            for x, y in zip(ctx.eval_grad(zp, rp, ds), other.eval_grad(zp, rp, ds)):
                assert np.array_equal(bits(x), bits(y))
        assert np.isfinite(ctx.eval(zp, rp, np.zeros(3, dtype=np.int64))[0]).all()
    finally:
        ctx.close()
        other.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_name_their_reason_and_leave_the_previous_store():
    from blueice_amd.exceptions import NotPreparedException
    case = cases.make_case('k2', 2)
    model, edges, z, rs = case['model'], case['edges'], case['z'], case['rs']
    ctx = toy_cases.upload(model)
    try:
        ctx.simulate_event_toys('piecewise', edges, z, rs, [1, 2], cases.SEED, OUTLIER)
        zp, rp = toy_cases.box_points(model, np.random.default_rng(5), 3)
        ds = np.arange(3)
        before = [bits(x).copy() for x in ctx.eval_grad(zp, rp, ds)]
        events = snapshot(ctx)
        outside = z.copy()
        outside[1, 2] = model['anchor_z'][2][-1] + 0.5
        big = rs.copy()
        big[0, 3] = 2.0 ** 30 / cases.mus_at(model, z[0])[3] * 1.001
        refusals = [
            ('outside the anchor box', dict(z=outside)),
            ('2\\^30 expected events', dict(rate_scale=big)),
            ('negative', dict(n_toys=[2, -1])),
            ('T >= 1', dict(n_toys=[0, 0])),
            ('bins', dict(edges=[edges[0], edges[1][:-1]])),
            ('method', dict(method='cubic')),
            ('ascending', dict(edges=[edges[0][::-1], edges[1]])),
        ]
        for reason, change in refusals:
            kw = dict(method='piecewise', edges=edges, z=z, rate_scale=rs, n_toys=[1, 2], seed=cases.SEED, outlier_likelihood=OUTLIER)
            kw.update(change)
            if kw['method'] == 'cubic':
                with pytest.raises(KeyError):
                    ctx.simulate_event_toys(**kw)
                rc = ctx._dev._lib.bi_sourcewise_simulate_event_toys(ctx._dev._h, 2, 2, None, None, 2, None, None, None, 0, 0.0, None)
                assert rc == -1 and 'method' in ctx._dev._lib.bi_last_error(ctx._dev._h).decode()
            else:
                with pytest.raises(ValueError, match=reason):
                    ctx.simulate_event_toys(**kw)
            assert ctx.T == 3 and ctx.get_param('sourcewise_event_sets') == 3
            for x, y in zip(ctx.eval_grad(zp, rp, ds), before):
                assert np.array_equal(bits(x), y), reason
            assert same(snapshot(ctx), events), reason
        # the store beyond compact_budget: nothing is built, the previous one stays
        budget = ctx.get_param('compact_budget')
        ctx.set_param('compact_budget', 1024)
        with pytest.raises(ValueError, match='compact_budget'):
            ctx.simulate_event_toys('piecewise', edges, z, rs, [1, 2], cases.SEED, OUTLIER)
        ctx.set_param('compact_budget', budget)
        assert same(snapshot(ctx), events)
        # a one-bin carrier model has no histograms to draw from
        carrier = toy_cases.upload(eo.carrier(model))
        try:
            with pytest.raises(ValueError, match='bins'):
                carrier.simulate_event_toys('piecewise', edges, z, rs, [1, 2], cases.SEED, OUTLIER)
        finally:
            carrier.close()
        # the events belong to the simulated store: another store releases them
        coords = [[c for c in events['coords'].view(np.float64).reshape(2, -1)[:, :events['n'][0]]]]
        ctx.score_events('piecewise', edges, coords, OUTLIER)
        assert ctx.simulated_event_count() == -1
        with pytest.raises(NotPreparedException, match='simulated'):
            ctx.download_events()
        ctx.simulate_event_toys('linear', edges, z, rs, [1, 0], cases.SEED, OUTLIER)
        assert ctx.simulated_event_count() == ctx.event_set_counts().sum() > 0
        ctx.drop_events()
        assert ctx.simulated_event_count() == -1
        with pytest.raises(NotPreparedException):
            ctx.download_events()
    finally:
        ctx.close()


# ---- 6. through the class ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def small_lf():
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5), n_params=3, n_sources=3, own_per_source=1, events_per_day=30.,
                                             source_class=NuisanceHistogramSource)
    conf['pdf_interpolation_method'] = 'linear'
    lf = SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False))
    for s in range(3):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-1., 0., 1.))
    lf.prepare()
    yield lf, names
    lf.ctx.close()


def test_toys_through_the_class_fit_like_their_events_set_as_datasets(small_lf):
    from blueice_amd import inference, sourcewise_event_toys, sourcewise_simulated_events
    lf, names = small_lf
    assert lf.scoring_route == 'device'
    counts = sourcewise_event_toys(lf, 8, seed=31, np0=0.4, s1_rate_multiplier=1.3)
    assert counts.shape == (8, 3) and lf.n_events_per_dataset.tolist() == counts.sum(axis=1).tolist() and lf.ctx.T == 8
    assert lf.toy_truth.tolist() == [0] * 8 and lf.is_data_set
    best, ll = inference.bestfit_toys(lf)
    stored = [bits(lf.ctx.download_event_set(t)).copy() for t in range(8)]
    everything = sourcewise_simulated_events(lf)
    assert set(everything.dtype.names) == {'x', 'y', 'source', 'toy'} and len(everything) == counts.sum()
    events = [sourcewise_simulated_events(lf, t) for t in range(8)]
    for t, d in enumerate(events):
        assert set(d.dtype.names) == {'x', 'y', 'source'} and np.bincount(d['source'], minlength=3).tolist() == counts[t].tolist()
        assert np.array_equal(d['x'], everything['x'][everything['toy'] == t])
    lf.set_datasets(events)
    for t in range(8):
        assert np.array_equal(bits(lf.ctx.download_event_set(t)), stored[t])
    best2, ll2 = inference.bestfit_toys(lf)
    assert np.array_equal(bits(ll), bits(ll2)) and all(np.array_equal(bits(best[k]), bits(best2[k])) for k in best)
    assert np.isfinite(ll).all()


def test_toy_inference_does_not_depend_on_the_chunk_and_gives_the_data_back(small_lf):
    from blueice_amd import inference
    lf, names = small_lf
    np.random.seed(8)
    d = lf.base_model.simulate()
    lf.set_data(d)
    ll0 = lf(np1=0.3)
    truth = {'np2': -0.5, 's0_rate_multiplier': 1.2}
    a = inference.toy_mc_fits(lf, 12, chunk=5, seed=17, truth=truth)
    b = inference.toy_mc_fits(lf, 12, chunk=12, seed=17, truth=truth)
    assert np.array_equal(bits(a[1]), bits(b[1])) and all(np.array_equal(bits(a[0][k]), bits(b[0][k])) for k in a[0])
    assert len(a[1]) == 12 and np.isfinite(a[1]).all() and lf.ctx.get_param('toy_offset') == 0
    lf.set_data(d)
    hyp = np.array([0.6, 1.0, 1.7])
    stats = [inference.toy_test_statistics(lf, 's2_rate_multiplier', hyp, 4, seed=23, chunk=chunk, kind='central',
                                           truth={'np0': np.array([-0.5, 0.0, 0.5])}) for chunk in (5, 12)]
    for key in ('t', 'll_free', 'll_cond', 'target_hat'):
        assert np.array_equal(bits(getattr(stats[0], key)), bits(getattr(stats[1], key))), key
    assert stats[0].t.shape == (3, 4) and np.isfinite(stats[0].t).all() and (stats[0].t > -1e-6).all() and stats[0].n_failed == 0
    # its own data are back, by set_data
    assert lf.n_events_per_dataset.tolist() == [len(d)] and lf.ctx.T == 1 and lf(np1=0.3) == ll0
    table = inference.neyman_thresholds(lf, 's2_rate_multiplier', hyp, 4, seed=23, chunk=5, kind='central', truth={'np0': np.array([-0.5, 0.0, 0.5])})
    assert np.array_equal(bits(table.t), bits(stats[0].t[np.argsort(hyp, kind='stable')]))
    for name in ('simulate_toy', 'simulate_toys', 'simulate_toys_points', 'simulated_events', 'toy_mc_fits', 'toy_test_statistics',
                 'neyman_thresholds'):
        with pytest.raises(NotImplementedError, match='unbinned source-wise model'):
            getattr(lf, name)()
