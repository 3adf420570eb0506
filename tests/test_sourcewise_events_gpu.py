"""Unbinned source-wise likelihoods on the device (the event store of bi_sourcewise_events_begin / bi_sourcewise_score_events;
k_sourcewise_events): bi_eval_factored and bi_fit_batched_factored over events, and SourceWiseUnbinnedLogLikelihood.

Every comparison of a finite number is derivative_oracle.check_entries with C_POISSON = 256 against
`derivatives(expand(model), unbinned=True)`, the same likelihood on the full tensor-product grid; status words, -inf, nan and
"bitwise" comparisons are exact.  The reference's recorded values are held to 1e-10, the fits to the 1e-6 in ll of
tests/test_sourcewise_nonempty_gpu.py (FIT_BAR).  Every shape is the smallest at which the walk can go wrong: an empty set (one
tile of padding, masked by index), one event (511 padded columns that must not meet the outlier clamp), a few, exactly one tile
and one tile plus an event, two tiles plus one, a set longer than the blocks of an item, and sets of different lengths in one
launch."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import factored_oracle as fo
import model_zoo
import sourcewise_events_oracle as eo
import sourcewise_toy_cases as toy_cases
import sourcewise_walk_cases as wc
from derivative_oracle import C_POISSON, check_entries, derivatives
from test_sourcewise_sampler_gpu import bits, class_case

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
FIT_BAR = 1e-6            # tests/test_sourcewise_nonempty_gpu.py
OUTLIER = 1e-12
CLASSES = list(wc.FAMILIES['load_forms']) + ['s4_e2']
LENGTHS = [0, 1, 5, 512, 513, 1025]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'api_source_wise.npz')


def event_model(rng, n_anchor, own, N, zero_quarter=(1,)):
    """pdf values at N events: factored_oracle.random_model's rows scaled to order one.  A source of `zero_quarter` is exactly 0
    at a quarter of the events (at least one) while the others are comfortably positive: no event sits on the clamp's knife edge"""
    model = fo.random_model(rng, n_anchor, own, max(N, 1), zero_quarter=zero_quarter)
    model['ps'] = [np.nan_to_num(p, nan=0.0) for p in model['ps']]      # (N = 1: the zeroed source's only value, 0 / 0)
    model['ps'] = [np.ascontiguousarray(p[..., :N] * max(N, 1)) for p in model['ps']]
    return model


def uploaded(model, n_events=None, outlier=OUTLIER):
    """a context with the geometry and rates of `model` (one-bin rows) and its pdf values as the event store"""
    ctx = toy_cases.upload(eo.carrier(model))
    eo.upload_events(ctx, model, [fo.n_bins(model)] if n_events is None else n_events, outlier)
    return ctx


def expanded_oracle(model, outlier=OUTLIER):
    full = fo.expand(model)
    return lambda z, rs: derivatives(full, z, rs, unbinned=True, outlier=outlier, hessian=False)


def check_points(ctx, z, rs, oracles, what, dataset=None):
    """value and gradient of every point against oracles[dataset[p]](z, rs) -> the worst ratio; the values-only call has the bits
    of the call with the gradient"""
    ll, gz, gs, st = ctx.eval_grad(z, rs, dataset)
    ll0, st0 = ctx.eval(z, rs, dataset)
    assert not st.any() and not st0.any()
    assert np.array_equal(bits(ll0), bits(ll))
    worst = 0.0
    for p in range(len(z)):
        want = oracles[0 if dataset is None else int(dataset[p])](z[p], rs[p])
        print('%s ll[%d] = %.17g (oracle %.17g)' % (what, p, ll[p], want['ll']))
        worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (what, p)))
        worst = max(worst, check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='%s grad[%d]' % (what, p)))
    print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (what, worst, C_POISSON))
    return worst


# ---- 1. the reference's recorded values at the C ABI -------------------------------------------------------------------------

def zoo_calls(cls=None):
    ns = model_zoo.namespace_of('blueice_amd')
    if cls is not None:
        ns = SimpleNamespace(**dict(vars(ns), UnbinnedLogLikelihood=cls))
    return model_zoo.api_source_wise(ns)


def test_golden_at_the_c_abi():
    f = np.load(GOLDEN)
    model = eo.golden_model(f)
    lf, calls = zoo_calls()
    lf.ctx.close()
    ctx = uploaded(model)
    try:
        assert ctx.get_param('sourcewise_events_ready') == 1 and ctx.get_param('sourcewise_event_sets') == 1
        assert ctx.event_set_counts().tolist() == [63]
        zr = [eo.golden_point(kw) for kw in calls]
        z, rs = np.array([a for a, _ in zr]), np.array([b for _, b in zr])
        ll, st = ctx.eval(z, rs)
        for j in range(7):
            want = f['call_ll'][j]
            print('call %d: %.17g (reference %.17g)' % (j, ll[j], want))
            assert st[j] == 0 and abs(ll[j] - want) <= 1e-10 * max(1.0, abs(want)), (j, ll[j], want)
        assert np.all(ll[7:] == -np.inf) and st[7:].tolist() == [ST_OUT_OF_BOUNDS] * 2
    finally:
        ctx.close()


# ---- 2. every class at every set length --------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CLASSES)
def test_every_class_at_every_set_length(name):
    own = class_case(name)[0]['own']
    worst = 0.0
    for N in LENGTHS:
        rng = np.random.default_rng(sum(name.encode()) + 31 * N)
        model = event_model(rng, (2, 2, 2, 2), own, N)
        z, rs = toy_cases.box_points(model, rng, 2)
        ctx = uploaded(model)
        try:
            rows = sum(np.asarray(m).size for m in model['mus'])
            assert ctx.get_param('sourcewise_events_bytes') == 8 * rows * max(512, -(-N // 512) * 512)
            if N == 0:
                ll, gz, gs, st = ctx.eval_grad(z, rs)
                assert not st.any() and np.array_equal(bits(ctx.eval(z, rs)[0]), bits(ll))
                for p in range(2):
                    total = float(eo.rate_terms(model, z[p], rs[p])[0].v)
                    print('%s N=0 ll[%d] = %.17g, -sum r = %.17g' % (name, p, ll[p], -total))
                    assert abs(ll[p] + total) <= 1e-12 * total
                    want = eo.events_derivatives(model, z[p], rs[p])
                    check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='%s N=0 grad[%d]' % (name, p))
            else:
                worst = max(worst, check_points(ctx, z, rs, [expanded_oracle(model)], '%s N=%d' % (name, N)))
            assert ctx.get_param('last_morph_nbx') == max(1, -(-N // 512))
        finally:
            ctx.close()
    print('%s: worst over the lengths %.3g of C = %d' % (name, worst, C_POISSON))


# ---- 3. the clamp and nan ----------------------------------------------------------------------------------------------------

def test_clamp_and_nan():
    rng = np.random.default_rng(33)
    own = ((0,), (1, 2), ())
    N = 63
    model = event_model(rng, (3, 2, 4), own, N, zero_quarter=())
    z, rs = toy_cases.box_points(model, rng, 3)
    base = uploaded(model)
    dead = {k: [np.array(p) for p in v] if k == 'ps' else v for k, v in model.items()}
    for p in dead['ps']:
        p[..., 5] = 0.0                                     # event 5: every row is 0
    holed = {k: [np.array(p) for p in v] if k == 'ps' else v for k, v in model.items()}
    holed['ps'][1][1, 2, 7] = np.nan                        # one corner of source 1 at event 7
    try:
        ll_base = base.eval(z, rs)[0]
        # an event whose every row is 0 contributes log(outlier) and no slope ...
        ctx = uploaded(dead)
        check_points(ctx, z, rs, [expanded_oracle(dead)], 'clamped event')
        ll, gz, gs, _ = ctx.eval_grad(z, rs)
        without = {k: [np.delete(p, 5, axis=-1) for p in v] if k == 'ps' else v for k, v in model.items()}
        for p in range(3):
            want = eo.events_derivatives(without, z[p], rs[p])
            check_entries(ll[p] - np.log(OUTLIER), want['ll'], want['ll_cond'] + abs(np.log(OUTLIER)), what='clamp ll[%d]' % p)
            check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='clamp grad[%d]' % p)
        ctx.close()
        # ... and with outlier = 0: -inf, and a nan gradient
        ctx = uploaded(dead, outlier=0.0)
        ll, gz, gs, st = ctx.eval_grad(z, rs)
        assert not st.any() and np.all(ll == -np.inf) and np.isnan(gz).all() and np.isnan(gs).all()
        assert np.all(ctx.eval(z, rs)[0] == -np.inf)
        ctx.close()
        # a nan at one corner: the source leaves that event where the point's cell has the corner, and nowhere else
        ctx = uploaded(holed)
        oracle = expanded_oracle(holed)
        check_points(ctx, z, rs, [oracle], 'nan corner')
        ll, _, _, _ = ctx.eval_grad(z, rs)
        # (source 1 owns axes 1 and 2; its rows [1, 2] are a corner of the point's cell wherever z_2 lies at or above anchor 1 of axis 2)
        touched = z[:, 2] >= holed['anchor_z'][2][1]
        assert touched[2]
        for p in range(3):
            assert np.isfinite(ll[p]) and (ll[p] != ll_base[p]) == bool(touched[p]), (p, touched[p])
        ctx.close()
        # +-inf is refused at the upload, and the store is gone
        bad = {k: [np.array(p) for p in v] if k == 'ps' else v for k, v in model.items()}
        bad['ps'][0][1, 3] = np.inf
        ctx = toy_cases.upload(eo.carrier(bad))
        with pytest.raises(ValueError, match='finite or nan'):
            eo.upload_events(ctx, bad, [N])
        assert ctx.get_param('sourcewise_events_ready') == 0
        ctx.close()
    finally:
        base.close()


# ---- 4. several sets in one launch -------------------------------------------------------------------------------------------

def test_several_sets_in_one_launch():
    """N_t = (0, 3, 513, 1200): one, one, two and three tiles.  A point has the bits it has alone whatever is evaluated beside it"""
    n = [0, 3, 513, 1200]
    own = class_case('mixed')[0]['own']
    rng = np.random.default_rng(44)
    model = event_model(rng, (2, 2, 2, 2), own, sum(n))
    off = np.concatenate([[0], np.cumsum(n)])
    per_set = [{k: [p[..., off[t]:off[t + 1]] for p in v] if k == 'ps' else v for k, v in model.items()} for t in range(4)]
    ctx = uploaded(model, n)
    try:
        assert ctx.get_param('sourcewise_event_sets') == 4 and ctx.event_set_counts().tolist() == n
        rows = sum(np.asarray(m).size for m in model['mus'])
        assert ctx.get_param('sourcewise_events_bytes') == 8 * rows * (512 + 512 + 1024 + 1536)
        P = 40
        z, rs = toy_cases.box_points(model, rng, P)
        ds = rng.integers(0, 4, P)
        ds[:8] = [0, 1, 2, 3, 3, 2, 1, 0]
        ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
        assert not st.any() and ctx.get_param('last_morph_nbx') == 3
        ll0, _ = ctx.eval(z, rs, ds)
        assert np.array_equal(bits(ll0), bits(ll))
        again = ctx.eval_grad(z, rs, ds)
        for a, b in zip(again, (ll, gz, gs)):
            assert np.array_equal(bits(a), bits(b))
        for p in range(P):
            a = ctx.eval_grad(z[p], rs[p:p + 1], ds[p:p + 1])
            assert bits(a[0])[0] == bits(ll)[p] and np.array_equal(bits(a[1][0]), bits(gz[p])) and np.array_equal(bits(a[2][0]), bits(gs[p]))
            assert bits(ctx.eval(z[p], rs[p:p + 1], ds[p:p + 1])[0])[0] == bits(ll)[p]
        oracles = [expanded_oracle(m) if t else (lambda zz, rr, m=m: eo.events_derivatives(m, zz, rr)) for t, m in enumerate(per_set)]
        check_points(ctx, z[:8], rs[:8], oracles, 'mixed sets', dataset=ds[:8])
        # a set of its own context: the same bits (nothing of the other sets enters)
        solo = uploaded(per_set[2])
        pick = np.flatnonzero(ds == 2)
        assert np.array_equal(bits(solo.eval(z[pick], rs[pick])[0]), bits(ll[pick]))
        solo.close()
        ds_bad = ds.copy()
        ds_bad[3], ds_bad[5] = 4, -1
        ll_b, gz_b, gs_b, st_b = ctx.eval_grad(z, rs, ds_bad)
        assert st_b[3] == ST_BAD_DATASET and st_b[5] == ST_BAD_DATASET and st_b.sum() == 2 * ST_BAD_DATASET
        assert ll_b[3] == -np.inf and np.isnan(gz_b[3]).all()
        keep = np.delete(np.arange(P), [3, 5])
        assert np.array_equal(bits(ll_b[keep]), bits(ll[keep]))
    finally:
        ctx.close()


# ---- 5. a set longer than an item's blocks -----------------------------------------------------------------------------------

def test_a_set_longer_than_the_blocks_of_an_item():
    """1026 tiles of events on the 1024 blocks of an item: blocks 0 and 1 walk a second tile, k_finish adds 1024 partials"""
    N = 1026 * 512 - 100
    rng = np.random.default_rng(1026)
    model = event_model(rng, (2, 2), [(0,), (1,)], N, zero_quarter=())
    z, rs = toy_cases.box_points(model, rng, 2)
    ctx = uploaded(model)
    try:
        check_points(ctx, z[:1], rs[:1], [expanded_oracle(model)], '1026 tiles')
        assert ctx.get_param('last_morph_nbx') == 1024
        both = ctx.eval(z, rs)[0]
        assert bits(both)[0] == bits(ctx.eval(z[:1], rs[:1])[0])[0]
    finally:
        ctx.close()


# ---- 6. device scoring -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('method,k', [('piecewise', 1), ('piecewise', 2), ('linear', 1), ('linear', 2)])
def test_device_scoring(method, k):
    """T = 3 sets, one empty: the stored values are bit for bit the NumPy lookup ('piecewise') or scipy's RegularGridInterpolator
    ('linear'), and the likelihood is bit for bit that of the same values uploaded row by row"""
    from scipy.interpolate import RegularGridInterpolator
    rng = np.random.default_rng(600 + 10 * k + len(method))
    edges = [np.sort(rng.uniform(-3.0, 3.0, n)) for n in ((14,), (9, 7))[k - 1]]
    shape = tuple(len(e) - 1 for e in edges)
    B = int(np.prod(shape))
    own = ((0,), (1, 2), ())
    model = fo.random_model(rng, (3, 2, 4), own, B, zero_quarter=(1,))
    model['ps'] = [p * B for p in model['ps']]               # densities of order one
    n = [700, 0, 37]
    coords = []
    for nt in n:
        cs = [rng.uniform(e[0] - 0.2, e[-1] + 0.2, nt) for e in edges]
        for c, e in zip(cs, edges):
            if nt:
                c[:3] = [e[0], e[-1], e[len(e) // 2]]        # on the outer edges and on an inner one
        coords.append(cs)
    centres = [0.5 * (e[:-1] + e[1:]) for e in edges]
    if method == 'linear':
        grid = centres
        coords = [[np.clip(c, g[0], g[-1]) for c, g in zip(cs, grid)] for cs in coords]
    else:
        grid = edges
    ctx = toy_cases.upload(model)
    try:
        with pytest.raises(ValueError, match='bins'):
            ctx.score_events(method, [g[:-1] for g in grid], coords, OUTLIER)
        assert ctx.get_param('sourcewise_events_ready') == 0
        ctx.score_events(method, grid, coords, OUTLIER)
        assert ctx.get_param('sourcewise_events_ready') == 1 and ctx.event_set_counts().tolist() == n
        flat = [np.asarray(p).reshape(-1, B) for p in model['ps']]
        rows = np.concatenate(flat)
        stored = []
        for t, cs in enumerate(coords):
            got = ctx.download_event_set(t)
            assert got.shape == (len(rows), n[t])
            if method == 'piecewise':
                idx = tuple(np.clip(np.searchsorted(e, c) - 1, 0, len(e) - 2) for e, c in zip(edges, cs))
                want = np.array([r.reshape(shape)[idx] for r in rows]).reshape(len(rows), n[t])
            else:
                want = np.array([RegularGridInterpolator(centres, r.reshape(shape))(np.transpose(cs)) for r in rows]).reshape(len(rows), n[t])
            assert np.array_equal(bits(got), bits(want)), (method, k, t)
            stored.append(got)
        z, rs = toy_cases.box_points(model, rng, 6)
        ds = np.array([0, 1, 2, 2, 1, 0])
        scored = ctx.eval_grad(z, rs, ds)
        assert not scored[3].any() and np.isfinite(scored[0]).all()
        # the same values through _set_row, on a context whose model rows are never read
        values = np.concatenate(stored, axis=1)
        first = np.concatenate([[0], np.cumsum([len(f) for f in flat])])
        host = toy_cases.upload(eo.carrier(model))
        host.set_event_rows(n, lambda s, local: values[first[s] + local], OUTLIER)
        for a, b in zip(host.eval_grad(z, rs, ds), scored):
            assert np.array_equal(bits(a), bits(b))
        assert np.array_equal(bits(host.eval(z, rs, ds)[0]), bits(scored[0]))
        host.close()
    finally:
        ctx.close()


# ---- 7. native fits ----------------------------------------------------------------------------------------------------------

def event_likelihoods(model, sets, priors):
    """The unbinned source-wise likelihood of `model` -- whose rows are pmfs over the positions 0 .. B - 1, an event being a
    position -- and the plain UnbinnedLogLikelihood of the same sources on the full grid (bi_set_unbinned, bi_fit_batched),
    built through the ordinary config -> Model -> prepare() route from one Source class"""
    from blueice_amd import GaussianPrior, SourceWiseUnbinnedLogLikelihood, UnbinnedLogLikelihood
    from blueice_amd.source import Source
    d, S, B = len(model['anchor_z']), len(model['own']), fo.n_bins(model)
    names = ['shape%d' % i for i in range(d)]

    class TensorSource(Source):
        def __init__(self, config, *args, **kwargs):
            m, s = config['tensor_model'], config['source_index']
            idx = tuple(int(np.flatnonzero(np.asarray(m['anchor_z'][i]) == float(config[names[i]]))[0]) for i in m['own'][s])
            self._row = np.asarray(m['ps'][s])[idx]
            super().__init__(dict(config, events_per_day=float(np.asarray(m['mus'][s])[idx]), livetime_days=1), *args, **kwargs)

        def pdf(self, *coords):
            return self._row[np.asarray(coords[0]).astype(int)]

    out = []
    for cls in (SourceWiseUnbinnedLogLikelihood, UnbinnedLogLikelihood):
        conf = dict(analysis_space=[('x', np.arange(B + 1, dtype=float))], default_source_class=TensorSource, tensor_model=model,
                    sources=[dict(name='s%d' % s, source_index=s,
                                  extra_dont_hash_settings=[n for i, n in enumerate(names) if i not in model['own'][s]]) for s in range(S)],
                    **{n: float(g[len(g) // 2]) for n, g in zip(names, model['anchor_z'])})
        lf = cls(conf, likelihood_config=dict(device=0, device_histograms=False))
        for s in range(2):
            lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.2) if priors else None)
        for i, (n, g) in enumerate(zip(names, model['anchor_z'])):
            lf.add_shape_parameter(n, tuple(float(v) for v in g),
                                   log_prior=GaussianPrior(float(g[len(g) // 2]), 0.5) if priors and i == 0 else None)
        lf.prepare()
        lf.set_datasets(sets)
        out.append(lf)
    return out


@pytest.mark.parametrize('priors', [False, True])
def test_native_fits_against_the_unbinned_grid_model(priors):
    """64 problems (one event set each) floating two shape parameters and two rate multipliers, with and without Gaussian
    constraints: bi_fit_batched_factored over the event store against bi_fit_batched[_gauss] on the expanded unbinned grid model"""
    B = 1001
    rng = np.random.default_rng(500 + B)
    model = fo.random_model(rng, (3, 2, 4), ((0,), (1, 2), ()), B, zero_quarter=(1,))
    rng = np.random.default_rng(64)
    from test_factored_gpu import box_points
    z, rs = box_points(model, rng, 64, on_anchor=False)
    z[:, 2] = 0.5 * (model['anchor_z'][2][1] + model['anchor_z'][2][2])
    rs[:, 2] = 1.0
    sets = []
    for t in range(64):
        counts = rng.poisson(0.25 * fo.expectation(model, z[t], rs[t]))
        d = np.zeros(int(counts.sum()), dtype=[('x', float), ('source', int)])
        d['x'] = np.repeat(np.arange(B), counts) + 0.5
        sets.append(d)
    sw, plain = event_likelihoods(model, sets, priors)
    assert type(sw.ctx).__name__ == 'SourceWiseContext' and sw.last_scoring_route == 'host' and plain.ctx.d == 3
    assert sw.n_events_per_dataset.tolist() == [len(d) for d in sets] == plain.n_events_per_dataset.tolist()
    fixed = dict(shape2=float(z[0, 2]))
    results = []
    for lf in (sw, plain):
        best, ll, info = lf.bestfit_batched(datasets=np.arange(64), return_info=True, **fixed)
        assert list(best) == ['s0_rate_multiplier', 's1_rate_multiplier', 'shape0', 'shape1']
        assert info['evaluations'] > 0                      # the native loop ran
        results.append((best, ll, info))
        print('%s: %d of 64 converged, %d failed, %d evaluations' % (type(lf).__name__, int(info['converged'].sum()), int(info['failed'].sum()),
                                                                     info['evaluations']))
    (b_sw, ll_sw, i_sw), (b_pl, ll_pl, i_pl) = results
    assert not i_sw['failed'].any() and not i_pl['failed'].any()
    worst = float(np.abs(ll_sw - ll_pl).max())
    print('priors=%s: worst |ll difference| %.3g over 64 problems' % (priors, worst))
    assert worst <= FIT_BAR
    sw.ctx.close()
    plain.ctx.close()


# ---- 8. state ----------------------------------------------------------------------------------------------------------------

def test_other_entry_points_refuse_while_the_store_exists():
    from blueice_amd.exceptions import NotPreparedException
    model, counts = class_case('mixed')
    B = fo.n_bins(model)
    rng = np.random.default_rng(8)
    z, rs = toy_cases.box_points(model, rng, 3)
    ds = np.array([0, 1, 2])
    ctx = toy_cases.upload(model, counts)
    try:
        before = ctx.eval_grad(z, rs, ds)
        # a context that never creates a store runs the code it ran before; with one, it is an unbinned likelihood
        edges = [np.arange(B + 1, dtype=float)]
        coords = [[rng.integers(0, B, 40) + 0.5], [rng.integers(0, B, 7) + 0.5]]
        ctx.score_events('piecewise', edges, coords, OUTLIER)
        assert ctx.get_param('sourcewise_events_ready') == 1 and ctx.get_param('sourcewise_events_bytes') == 8 * 1024 * sum(m.size for m in ctx.mus)
        ll, st = ctx.eval(z, rs, ds)
        assert st.tolist() == [0, 0, ST_BAD_DATASET] and np.isfinite(ll[:2]).all()
        refused = {
            'bi_factored_set_counts': lambda: ctx.set_counts(counts),
            'bi_sourcewise_generate_toys': lambda: ctx.generate_toys_points(z[:1], rs[:1], 2, seed=1),
            'bi_eval_sourcewise_hess': lambda: ctx.eval_hess(z, rs),
            'bi_eval_sourcewise_fisher': lambda: ctx.eval_fisher(z, rs),
            'bi_eval_sourcewise_gof': lambda: ctx.eval_gof(z, rs),
            'bi_sourcewise_expected_counts': lambda: ctx.expected_counts(z, rs),
            'bi_sourcewise_set_coarse_binning': lambda: ctx.set_coarse_binning([B], [np.array([0, B // 2, B])]),
            'bi_sourcewise_download_counts': lambda: (setattr(ctx, '_counts', None), ctx.download_counts(0)),
            'bi_sourcewise_set_real_counts': lambda: ctx.set_real_counts(counts[0]),
            'bi_sourcewise_set_asimov_counts': lambda: ctx.set_asimov_counts(z[:1], rs[:1]),
            'bi_sourcewise_build_nonempty': lambda: ctx.build_nonempty(),
            'bi_eval_sourcewise_planned': lambda: ctx.eval_planned(z, rs),
            'bi_eval_sourcewise_scan': lambda: ctx.eval_scan(z, rs),
            'bi_sample_stretch_sourcewise': lambda: ctx.sample_stretch(2, [1], [0], z[0], rs[0], np.ones(ctx.S), None, np.ones((1, 2, 1)),
                                                                       [0.0], [4.0], 1),
            'bi_grid_reduce_sourcewise': lambda: ctx.grid_reduce([1], [0], z[0], rs[0], np.ones(ctx.S), None, 1, [np.array([0.5, 1.0])]),
        }
        for who, call in refused.items():
            with pytest.raises(NotPreparedException, match='event store') as info:
                call()
            assert who in str(info.value), (who, str(info.value))
        # a row-wise store that is still being filled refuses to be evaluated, a row twice is an error, _end names what is missing
        from blueice_amd._capi import ptr
        dev = ctx._dev
        n_ev = np.array([3], dtype=np.int64)
        v = np.ones(3)
        dev._check(dev._lib.bi_sourcewise_events_begin(dev._h, 1, ptr(n_ev), OUTLIER))
        assert ctx.get_param('sourcewise_events_ready') == 0
        with pytest.raises(NotPreparedException, match='bi_sourcewise_events_end'):
            ctx.eval(z, rs)
        dev._check(dev._lib.bi_sourcewise_events_set_row(dev._h, 1, 0, ptr(v)))
        with pytest.raises(ValueError, match='set before'):
            dev._check(dev._lib.bi_sourcewise_events_set_row(dev._h, 1, 0, ptr(v)))
        with pytest.raises(NotPreparedException, match='anchor 0 of source 0 was never set'):
            dev._check(dev._lib.bi_sourcewise_events_end(dev._h))
        # beyond the budget: refused with the bytes, nothing is built
        ctx.drop_events()
        budget = ctx.get_param('compact_budget')
        ctx.set_param('compact_budget', 1000)
        with pytest.raises(ValueError, match='compact_budget'):
            ctx.score_events('piecewise', edges, coords, OUTLIER)
        assert ctx.get_param('sourcewise_events_ready') == 0 and ctx.get_param('sourcewise_events_bytes') == 0
        ctx.set_param('compact_budget', budget)
        # dropped: the counts stayed resident beside the store, and the binned evaluation has the bits of before; with new counts too
        assert ctx.T == 3
        for a, b in zip(ctx.eval_grad(z, rs, ds), before):
            assert np.array_equal(bits(a), bits(b))
        ctx.set_counts(counts)
        for a, b in zip(ctx.eval_grad(z, rs, ds), before):
            assert np.array_equal(bits(a), bits(b))
        # a new model releases the store
        ctx.score_events('piecewise', edges, coords, OUTLIER)
        ctx.begin_model(model['anchor_z'], len(model['own']), B, model['own'])
        assert ctx.get_param('sourcewise_events_ready') == 0 and ctx.get_param('sourcewise_event_sets') == 0
    finally:
        ctx.close()


# ---- 9. through the class ----------------------------------------------------------------------------------------------------

def test_the_class_reproduces_the_reference_and_the_full_grid_route():
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    f = np.load(GOLDEN)
    sw, calls = zoo_calls(SourceWiseUnbinnedLogLikelihood)
    full, _ = zoo_calls()
    try:
        assert type(sw.ctx).__name__ == 'SourceWiseContext' and sw.ctx.get_param('sourcewise_events_ready') == 1
        for j, kw in enumerate(calls):
            got, want = sw(**kw), f['call_ll'][j]
            print('call %d: %.17g (reference %.17g)' % (j, got, want))
            if j < 7:
                assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (j, got, want)
            else:
                assert got == -np.inf
        model = eo.golden_model(f)
        rng = np.random.default_rng(19)
        P = 6
        pts = dict(mu=rng.uniform(-0.95, 0.95, P), sigma=rng.uniform(0.85, 1.45, P))
        pts.update({n + '_rate_multiplier': rng.uniform(0.6, 1.5, P) for n in 'abc'})
        ll_sw, ll_full = sw.eval_points(pts), full.eval_points(pts)
        (llg_sw, g_sw), (llg_full, g_full) = sw.values_and_gradients(pts), full.values_and_gradients(pts)
        np.testing.assert_array_equal(llg_sw, ll_sw)
        names = ['mu', 'sigma'] + [n + '_rate_multiplier' for n in 'abc']
        for p in range(P):
            assert abs(ll_sw[p] - ll_full[p]) <= 1e-10 * max(1.0, abs(ll_full[p])), (p, ll_sw[p], ll_full[p])
            zp, rp = eo.golden_point({k: v[p] for k, v in pts.items()})
            want = eo.events_derivatives(model, zp, rp)
            check_entries(ll_sw[p], want['ll'], want['ll_cond'], what='eval_points[%d]' % p)
            check_entries(np.array([g_sw[n][p] for n in names]), want['grad'], want['grad_cond'], what='values_and_gradients[%d]' % p)
            check_entries(np.array([g_full[n][p] for n in names]), want['grad'], want['grad_cond'], what='full grid gradient[%d]' % p)
        fits = []
        for lf in (sw, full):
            best, ll = lf.bestfit_device()
            scan = lf.likelihood_ratio_scan(('b_rate_multiplier', np.array([0.5, 1.0, 1.5, 2.0])))
            limit = lf.one_parameter_interval('c_rate_multiplier', 6.0, confidence_level=0.9, kind='upper')
            fits.append((ll, np.asarray(scan, dtype=float), limit))
            print('%s: ll %.12g, scan %s, limit %.9g' % (type(lf).__name__, ll, scan, limit))
        assert abs(fits[0][0] - fits[1][0]) <= FIT_BAR
        # (Nelder-Mead stops when the simplex spans 1e-4 in f: never above the maximum, and not far below it)
        ll_scipy = sw.bestfit_scipy()[1]
        print('bestfit_scipy: ll %.12g' % ll_scipy)
        assert fits[0][0] - 1e-3 <= ll_scipy <= fits[0][0] + FIT_BAR
        print('likelihood_ratio_scan: worst |difference| %.3g' % np.max(np.abs(fits[0][1] - fits[1][1])))
        assert np.all(np.abs(fits[0][1] - fits[1][1]) <= FIT_BAR)
        # second derivatives: differences of the analytic gradient here, the analytic Hessian on the full grid.  A central difference
        # over h = 1e-5 (rates) or 1e-4 of a cell of a gradient good to 1e-13 of its terms (some 1e2) is good to about 1e-6 in
        # entries of 10 to 1e3: 1e-5 of sqrt(|H_ii H_jj|) bounds it with room
        at = dict(mu=np.array([0.3]), sigma=np.array([1.2]), a_rate_multiplier=np.array([1.1]), b_rate_multiplier=np.array([0.9]),
                  c_rate_multiplier=np.array([1.3]))
        _, _, names_sw, H_sw = sw.values_gradients_hessians(at)
        _, _, names_full, H_full = full.values_gradients_hessians(at)
        assert names_sw == names_full and sw.hessian_method == 'gradient-differences' and full.hessian_method == 'analytic'
        scale = np.sqrt(np.abs(np.outer(np.diag(H_full[0]), np.diag(H_full[0]))))
        print('Hessian by gradient differences: worst |difference| / sqrt(|H_ii H_jj|) = %.3g' % np.max(np.abs(H_sw[0] - H_full[0]) / scale))
        assert np.all(np.abs(H_sw[0] - H_full[0]) <= 1e-5 * scale)
        minuit, ll_minuit = sw.bestfit_minuit()
        assert abs(ll_minuit - fits[0][0]) <= FIT_BAR and all(n + '_error' in minuit for n in names_sw)
        # the interval, in ll: the two limits are two hypotheses of the signal; either likelihood's conditional profile has the same
        # value at both, and the two profiles agree at either
        limits = np.array([fits[0][2], fits[1][2]])
        assert np.isfinite(limits).all() and 0.0 < limits.min()
        prof_sw = np.asarray(sw.bestfit_batched(points={'c_rate_multiplier': limits})[1], dtype=float)
        prof_full = np.asarray(full.bestfit_batched(points={'c_rate_multiplier': limits})[1], dtype=float)
        print('one_parameter_interval: limits %.12g and %.12g; profiles there %s (source-wise) and %s (full grid)'
              % (limits[0], limits[1], prof_sw, prof_full))
        assert abs(prof_sw[0] - prof_sw[1]) <= FIT_BAR and abs(prof_full[0] - prof_full[1]) <= FIT_BAR
        assert np.all(np.abs(prof_sw - prof_full) <= FIT_BAR)
    finally:
        sw.ctx.close()
        full.ctx.close()


def twelve_nuisances(**likelihood_config):
    """d = 12 nuisances of 5 anchors (5^12 grid anchors: no grid model), 6 histogram sources with one or two own parameters"""
    from blueice_amd import GaussianPrior, SourceWiseUnbinnedLogLikelihood
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(12, 10), n_params=12, n_sources=6, own_per_source=2, events_per_day=40.,
                                             source_class=NuisanceHistogramSource)
    for s in (1, 4):                                        # one own parameter
        spec = conf['sources'][s]
        spec['own_settings'] = spec['own_settings'][:1]
        spec['extra_dont_hash_settings'] = [n for n in names if n not in spec['own_settings']]
    lf = SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False, **likelihood_config))
    for s in range(6):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    return lf, names


def test_twelve_nuisances_have_no_grid():
    from blueice_amd import LogLikelihoodSum, inference
    lf, names = twelve_nuisances()
    host, _ = twelve_nuisances(device_scoring=False)
    try:
        assert lf.scoring_route == 'device' and host.scoring_route == 'host'
        assert [len(lf._own_sources(s)) for s in range(6)] == [25, 5, 25, 25, 5, 25]
        np.random.seed(12)
        d = lf.base_model.simulate()[:300]
        assert len(d) == 300
        for x in (lf, host):
            x.set_data(d)
        assert lf.last_scoring_route == 'device' and host.last_scoring_route == 'host'
        assert np.array_equal(bits(lf.ctx.download_event_set(0)), bits(host.ctx.download_event_set(0)))
        coords = lf.base_model.to_analysis_dimensions(d)
        anchor_z = [np.array(sorted(lf.shape_parameters[n][0])) for n in names]
        own, ps, mus = [], [], []
        for s, name in enumerate(lf.source_name_list):
            o = tuple(names.index(k) for k in lf.source_shape_parameters[name])
            shape = tuple(5 for _ in o)
            srcs = lf._own_sources(s)
            own.append(o)
            ps.append(np.array([x.pdf(*coords) for x in srcs]).reshape(shape + (300,)))
            mus.append(np.array([x.expected_events for x in srcs]).reshape(shape))
        model = dict(anchor_z=anchor_z, own=own, ps=ps, mus=mus)
        rng = np.random.default_rng(9)
        P = 4
        pts = {n: rng.uniform(-1.9, 1.9, P) for n in names}
        pts.update({'s%d_rate_multiplier' % s: rng.uniform(0.6, 1.5, P) for s in range(6)})
        ll = lf.eval_points(pts)
        ll_g, grads = lf.values_and_gradients(pts)
        np.testing.assert_array_equal(ll_g, ll)
        assert np.array_equal(bits(host.eval_points(pts)), bits(ll))
        assert np.array_equal(bits(host.values_and_gradients(pts)[1][names[3]]), bits(grads[names[3]]))
        for p in range(P):
            zp = np.array([pts[n][p] for n in names])
            rp = np.array([pts['s%d_rate_multiplier' % s][p] for s in range(6)])
            want = eo.events_derivatives(model, zp, rp)
            prior = float(sum(lf.shape_parameters[n][1](zp[i]) for i, n in enumerate(names)))
            check_entries(ll[p] - prior, want['ll'], want['ll_cond'] + abs(prior), what='eval_points[%d]' % p)
            assert lf(**{k: float(v[p]) for k, v in pts.items()}) == ll[p]
            got = np.array([grads[n][p] - lf.shape_parameters[n][1].slope(zp[i]) for i, n in enumerate(names)]
                           + [grads['s%d_rate_multiplier' % s][p] for s in range(6)])
            check_entries(got, want['grad'], want['grad_cond'] + np.concatenate([np.abs(zp), np.zeros(6)]), what='values_and_gradients[%d]' % p)
        assert lf(np0=2.5) == -np.inf
        # the fit layers: Gaussian constraints on the native loop, a scan, and fits of several sets at once
        best, ll_best = lf.bestfit_device()
        assert np.isfinite(ll_best) and ll_best >= ll.max() and set(best) == set(names) | {'s%d_rate_multiplier' % s for s in range(6)}
        scan = np.asarray(lf.likelihood_ratio_scan(('s5_rate_multiplier', np.array([0.5, 1.0, 2.0]))), dtype=float)
        assert scan.shape == (3,) and np.all(scan >= -FIT_BAR)
        total = LogLikelihoodSum([lf, host])
        at = {k: float(v[0]) for k, v in pts.items()}
        assert abs(total(**at) - 2 * ll[0]) <= 1e-9 * abs(ll[0])
        np.random.seed(13)
        sets = [lf.base_model.simulate()[:n] for n in (250, 0, 300)]
        lf.set_datasets(sets)
        assert lf.n_events_per_dataset.tolist() == [250, 0, 300] and lf.ctx.T == 3
        fitted, lls = inference.bestfit_toys(lf)
        assert np.asarray(lls).shape == (3,) and np.isfinite(lls).all()
        lf.set_data(sets[2])
        assert abs(lf.bestfit_device()[1] - lls[2]) <= FIT_BAR
        for name in ('simulate_toys', 'sample_posterior', 'grid_scan', 'goodness_of_fit', 'fisher_information'):
            with pytest.raises(NotImplementedError, match='unbinned source-wise'):
                getattr(lf, name)()
        with pytest.raises(NotImplementedError, match='SourceWiseUnbinnedLogLikelihood'):
            lf(compute_pdf=True)
    finally:
        lf.ctx.close()
        host.ctx.close()
