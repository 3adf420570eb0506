"""Unbinned toy-MC ensembles on the device: T event-level toys drawn in one call (bi_simulate_event_toys), T event sets side
by side in one context (bi_score_event_sets), evaluated (k_morph_sets, or the single-set kernels over one set's columns) and
fitted (bi_fit_batched over a dataset column) -- every stage against a yardstick the tree already has: the draw-for-draw
replay of tests/toy_oracle.py, device scoring of one set alone, the per-entry bound of tests/derivative_oracle.py, and the
single-set fit."""
from collections import OrderedDict

import numpy as np
import pytest

import derivative_oracle as do
import model_zoo
import toy_oracle as orc

pytestmark = pytest.mark.gpu

SPACE = [['x', np.linspace(-4, 4, 9)], ['y', np.array([0., 0.4, 1., 2.2, 3.5, 5., 6.])]]          # 8 x 6 bins
SHAPES = {'a': OrderedDict(), 'b': OrderedDict(shift=(-1., 0., 1.)), 'c': OrderedDict(shift=(-1., 0., 1.), stretch=(0., 1.))}
VARIANTS = [(v, m) for v in 'abc' for m in ('piecewise', 'linear')]
SMALL = dict(s0_rate_multiplier=0.02, s1_rate_multiplier=0.01, s2_rate_multiplier=0.004)           # about two events per toy
T6 = 6


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


def make_lf(ns, variant, method, n_data=20, **lc):
    rng = np.random.default_rng(700 + ord(variant))
    return model_zoo.morph_lf(ns, rng, 3, SPACE, SHAPES[variant], 3000, n_data, unbinned=True, lc=lc or None,
                              extra_config=dict(pdf_interpolation_method=method))


_LF = {}


def shared_lf(ns, variant, method):
    """one prepared likelihood per variant for the whole module (its data are replaced by every test)"""
    if (variant, method) not in _LF:
        _LF[variant, method] = make_lf(ns, variant, method)
    return _LF[variant, method]


def truth_of(variant, **rates):
    t = dict(rates)
    if variant in 'bc':
        t['shift'] = 0.35
    if variant == 'c':
        t['stretch'] = 0.6
    return t


def truth_inputs(lf, truth):
    """-> (densities [S, B] and rates [S] at the truth point as the generator sees them, the bin edges)"""
    tp, _, _ = lf._histogram_templates()
    _, zs, scale = lf._host_terms(None, truth)
    dens = tp.interpolate('ps', zs)
    rates = tp.interpolate('mus', zs) * scale
    return dens, rates, [np.asarray(e, dtype=float) for _, e in SPACE]


def oracle_counts(rates, seed, toys):
    from blueice_amd import toy_seed
    out = np.zeros((len(toys), len(rates)))
    for i, D in enumerate(toys):
        for s, M in enumerate(rates):
            if M > 0:
                n, und = orc.event_count(float(M), toy_seed(seed, D) ^ orc.SIM_COUNT_KEY, [s])
                out[i, s] = n[0]
    return out


def pick_seed(rates, toys):
    """the first seed whose toys include an empty one, one with an odd and one with an even (non-zero) count -- on the CPU"""
    for seed in range(1, 400):
        tot = oracle_counts(rates, seed, toys).sum(axis=1)
        if (tot == 0).any() and (tot % 2 == 1).any() and ((tot > 0) & (tot % 2 == 0)).any():
            return seed
    raise AssertionError("no seed below 400 gives an empty, an odd and an even toy")


def check_ensemble(lf, truth, seed, offset, T, counts, what):
    from blueice_amd import toy_seed
    dens, rates, edges = truth_inputs(lf, truth)
    off = lf.ctx.event_set_offsets()
    n_dev = lf.n_events_per_dataset
    assert np.all(off % 2 == 0) and len(off) == T + 1 and off[0] == 0
    for t in range(T):
        rep = orc.simulate_events(dens, edges, rates, toy_seed(seed, offset + t))
        ev = lf.simulated_events(t)
        coords = np.stack([ev[n] for n, _ in SPACE])
        orc.compare_events(counts[t], coords, ev['source'].astype(np.int32), rep, '%s toy %d' % (what, offset + t))
        if not rep.und_n.any():
            assert n_dev[t] == int(rep.n.sum()) and off[t + 1] == off[t] + (n_dev[t] + 1) // 2 * 2


@pytest.mark.parametrize('variant,method', VARIANTS)
def test_draws_are_the_single_toy_generator_with_toy_seed(ns, variant, method):
    lf = shared_lf(ns, variant, method)
    truth = truth_of(variant, **SMALL)
    _, rates, _ = truth_inputs(lf, truth)
    toys = list(range(0, T6)) + list(range(5, 5 + T6))
    seed = pick_seed(rates, toys[:T6])
    want = oracle_counts(rates, seed, toys)
    tot = want[:T6].sum(axis=1)
    assert (tot == 0).any() and (tot % 2 == 1).any() and ((tot > 0) & (tot % 2 == 0)).any()       # the precondition, on the oracle
    try:
        for offset in (0, 5):
            lf.ctx.set_param('toy_offset', offset)
            counts = lf.simulate_toys(T6, seed=seed, **truth)
            assert counts.shape == (T6, 3) and lf.ctx.T == T6
            check_ensemble(lf, truth, seed, offset, T6, counts, '%s %s' % (variant, method))
        # T = 6 in one call = two calls of T = 3 at toy_offset 0 and 3
        lf.ctx.set_param('toy_offset', 0)
        c6 = lf.simulate_toys(T6, seed=seed, **truth)
        e6 = [lf.simulated_events(t) for t in range(T6)]
        for offset in (0, 3):
            lf.ctx.set_param('toy_offset', offset)
            c3 = lf.simulate_toys(3, seed=seed, **truth)
            assert np.array_equal(c3, c6[offset:offset + 3])
            for t in range(3):
                assert np.array_equal(lf.simulated_events(t), e6[offset + t])
    finally:
        lf.ctx.set_param('toy_offset', 0)


@pytest.mark.parametrize('variant,method', [('b', 'piecewise'), ('c', 'linear')])
def test_draws_of_segments_longer_than_a_tile(ns, variant, method):
    """T = 3 at about 700 expected events: a set spans more than one 512-event tile and more than one block"""
    lf = shared_lf(ns, variant, method)
    truth = truth_of(variant, s0_rate_multiplier=5.0, s1_rate_multiplier=2.5, s2_rate_multiplier=2.5)
    _, rates, _ = truth_inputs(lf, truth)
    assert 600 < rates.sum() < 900
    counts = lf.simulate_toys(3, seed=77, **truth)
    assert counts.sum(axis=1).min() > 512
    check_ensemble(lf, truth, 77, 0, 3, counts, 'long %s %s' % (variant, method))


def oracle_sets(lf, truth, seed, T):
    """the oracle's events of toys 0 .. T - 1 as record arrays"""
    from blueice_amd import toy_seed
    dens, rates, edges = truth_inputs(lf, truth)
    out = []
    for t in range(T):
        rep = orc.simulate_events(dens, edges, rates, toy_seed(seed, t))
        d = np.zeros(len(rep.source), dtype=[(n, float) for n, _ in SPACE] + [('source', int)])
        for (n, _), c in zip(SPACE, rep.coords):
            d[n] = c
        d['source'] = rep.source
        out.append(d)
    return out


@pytest.mark.parametrize('variant,method', VARIANTS)
def test_uploaded_stack_equals_every_set_scored_alone(ns, variant, method):
    lf = shared_lf(ns, variant, method)
    truth = truth_of(variant, **SMALL)
    _, rates, _ = truth_inputs(lf, truth)
    seed = pick_seed(rates, range(T6))
    sets = oracle_sets(lf, truth, seed, T6)
    more = model_zoo.sample(np.random.default_rng(5), 600, SPACE)                                 # one set longer than a tile
    longer = np.zeros(len(sets[1]) + len(more), dtype=sets[1].dtype)
    for name in sets[1].dtype.names:
        longer[name] = np.concatenate([sets[1][name], more[name]])
    sets[1] = longer
    lf.set_datasets(sets)
    assert lf.ctx.T == T6 and np.array_equal(lf.n_events_per_dataset, [len(d) for d in sets])
    got = [lf.ctx.download_event_set(t) for t in range(T6)]
    for t, d in enumerate(sets):
        lf.set_data(d)
        assert lf.ctx.T == 1 and lf.ctx.get_param('events_sorted') == 0
        alone = lf.ctx.download_event_set(0)
        assert alone.shape == got[t].shape
        np.testing.assert_allclose(got[t], alone, rtol=1e-14, atol=0)


def anchor_model(lf, t, edit=None):
    """the oracle's model dict of event set t: anchor grid, the set's own [A.., S, N_t] columns, the anchors' rates"""
    ctx = lf.ctx
    grid = [np.asarray(g, dtype=float) for g in ctx.anchor_z]
    shape = tuple(len(g) for g in grid)
    ps = ctx.download_event_set(t)
    ps = ps.reshape(shape + ps.shape[1:])
    mus = np.empty(shape + (ctx.S,))
    for idx in np.ndindex(*shape):
        mus[idx] = ctx.interpolate('mus', np.array([g[i] for g, i in zip(grid, idx)]))
    return dict(anchor_z=grid, ps=ps, mus=mus, n_model=None)


def points_for(lf, rng, datasets):
    """a point per dataset entry: on anchors and inside cells alternately; rate scales around the truth's"""
    ctx = lf.ctx
    P = len(datasets)
    z = np.empty((P, ctx.d))
    for p in range(P):
        for i, g in enumerate(ctx.anchor_z):
            z[p, i] = g[rng.integers(len(g))] if p % 3 == 0 else rng.uniform(g[0], g[-1])
    rs = rng.uniform(0.005, 0.05, (P, ctx.S))
    return z, rs


def check_against_oracle(lf, z, rs, ds, what, outlier=1e-12):
    ctx = lf.ctx
    z_arg = z if ctx.d else None
    ll_g, gz, gs, st_g = ctx.eval_grad(z_arg, rs, ds)
    ll_e, st_e = ctx.eval(z_arg, rs, ds)
    assert not st_g.any() and not st_e.any()
    g = np.concatenate([gz, gs], axis=1)
    models = {}
    for p in range(len(rs)):
        t = 0 if ds is None else int(ds[p])
        if t not in models:
            models[t] = anchor_model(lf, t)
        o = do.derivatives(models[t], z[p], rs[p], unbinned=True, outlier=outlier, hessian=False)
        do.check_entries(ll_e[p], o['ll'], o['ll_cond'], do.C_POISSON, '%s bi_eval p%d set %d' % (what, p, t))
        do.check_entries(ll_g[p], o['ll'], o['ll_cond'], do.C_POISSON, '%s bi_eval_grad ll p%d set %d' % (what, p, t))
        do.check_entries(g[p], o['grad'], o['grad_cond'], do.C_POISSON, '%s grad p%d set %d' % (what, p, t))
    return ll_e


def small_ensemble(lf, variant, extra=0):
    truth = truth_of(variant, **SMALL)
    _, rates, _ = truth_inputs(lf, truth)
    seed = pick_seed(rates, range(T6))
    counts = lf.simulate_toys(T6, seed=seed, **truth)
    return truth, seed, counts


@pytest.mark.parametrize('variant,method', VARIANTS)
def test_values_and_gradients_of_mixed_datasets(ns, variant, method):
    lf = shared_lf(ns, variant, method)
    truth, seed, counts = small_ensemble(lf, variant)
    tot = counts.sum(axis=1)
    empty = int(np.flatnonzero(tot == 0)[0])
    rng = np.random.default_rng(31)
    ds = np.array([3, 0, empty, 5, 1, 3, 2, empty, 4, 0, 5, 1, 2, 3, 4], dtype=np.int64)             # P = 2 T + 3, unsorted, repeats
    assert len(ds) == 2 * T6 + 3
    z, rs = points_for(lf, rng, ds)
    before = lf.ctx.get_param('n_set_launches')
    check_against_oracle(lf, z, rs, ds, 'mixed %s %s' % (variant, method))
    assert lf.ctx.get_param('n_set_launches') >= before + 2                                        # bi_eval and bi_eval_grad: k_morph_sets
    # all points name one dataset t > 0: the single-set kernels over that set's columns
    t1 = int(np.flatnonzero(tot > 0)[-1])
    assert t1 > 0
    before = lf.ctx.get_param('n_set_launches')
    check_against_oracle(lf, z[:5], rs[:5], np.full(5, t1, dtype=np.int64), 'one set %s %s' % (variant, method))
    assert lf.ctx.get_param('n_set_launches') == before
    # no dataset column, and the plain call: set 0
    ll0 = check_against_oracle(lf, z[:4], rs[:4], None, 'set 0 %s %s' % (variant, method))
    kw = dict(truth)
    m0 = anchor_model(lf, 0)
    _, zs, scale = lf._host_terms(None, kw)
    o = do.derivatives(m0, zs, scale, unbinned=True, hessian=False)
    do.check_entries(lf(**kw), o['ll'], o['ll_cond'], do.C_POISSON, 'plain call')
    toys_ll = lf.eval_toys(**kw)
    assert toys_ll.shape == (T6,) and np.isfinite(toys_ll).all()
    do.check_entries(toys_ll[0], o['ll'], o['ll_cond'], do.C_POISSON, 'eval_toys[0]')
    assert np.isfinite(ll0).all()


def test_long_segments_mixed(ns):
    """sets of more than one tile: several blocks per item, items of different lengths in one launch"""
    lf = shared_lf(ns, 'b', 'linear')
    truth = truth_of('b', s0_rate_multiplier=5.0, s1_rate_multiplier=2.5, s2_rate_multiplier=2.5)
    lf.simulate_toys(3, seed=78, **truth)
    sets = [lf.simulated_events(t) for t in range(3)]
    sets[1] = sets[1][:37]
    sets.append(sets[0][:0])
    lf.set_datasets(sets)
    rng = np.random.default_rng(32)
    ds = np.array([2, 1, 3, 0, 2, 0], dtype=np.int64)
    z, _ = points_for(lf, rng, ds)
    rs = rng.uniform(3.0, 6.0, (len(ds), 3))
    check_against_oracle(lf, z, rs, ds, 'long mixed')


@pytest.mark.parametrize('kind', ['nan', 'outlier'])
def test_nan_pdf_entry_and_clamped_event_in_another_set_than_0(ns, kind):
    """host-scored stacks (the tensor is streamed up), edited in set 2: a nan pdf entry / an event no source expects"""
    lf = make_lf(ns, 'b', 'piecewise', device_scoring=False)
    rng = np.random.default_rng(33)
    sets = [model_zoo.sample(rng, n, SPACE) for n in (7, 0, 11, 4)]
    real = type(lf.base_model).score_events

    def edited(model, d):
        out = np.array(real(model, d), dtype=float)
        if len(d) == 11:
            if kind == 'nan':
                out[1, 4] = np.nan
            else:
                out[:, 6] = 0.0
        return out
    import unittest.mock as mock
    with mock.patch.object(type(lf.base_model), 'score_events', edited):
        lf.set_datasets(sets)
    assert lf.ctx.T == 4 and np.array_equal(lf.n_events_per_dataset, [7, 0, 11, 4])
    col = lf.ctx.download_event_set(2)
    assert np.isnan(col[:, 1, 4]).all() if kind == 'nan' else (col[:, :, 6] == 0).all()
    ds = np.array([2, 0, 1, 2, 3], dtype=np.int64)
    z, _ = points_for(lf, rng, ds)
    rs = rng.uniform(0.02, 0.2, (len(ds), 3))
    check_against_oracle(lf, z, rs, ds, kind)
    check_against_oracle(lf, z[:2], rs[:2], np.full(2, 2, dtype=np.int64), kind + ' one set')


def test_single_set_contexts_give_the_same_bits(ns):
    """T = 1 through the new calls is today's layout and today's kernels: the same bits as set_data"""
    lf = shared_lf(ns, 'c', 'linear')
    rng = np.random.default_rng(34)
    d = model_zoo.sample(rng, 333, SPACE)
    z, rs = points_for(lf, rng, np.zeros(5))
    lf.set_data(d)
    want = lf.ctx.eval_grad(z, rs, None)
    want_ds = lf.ctx.eval_grad(z, rs, np.zeros(5, dtype=np.int64))
    want_e = lf.ctx.eval(z, rs)
    lf.set_datasets([d])
    assert lf.ctx.T == 1
    for a, b in zip(want + want_ds + want_e, lf.ctx.eval_grad(z, rs, None) + lf.ctx.eval_grad(z, rs, np.zeros(5, dtype=np.int64)) + lf.ctx.eval(z, rs)):
        assert np.array_equal(a, b, equal_nan=True)
    # ... and a set alone in a stack evaluates to the single-set context's bits through the pointer-offset route
    lf.set_datasets([d[:10], d])
    got = lf.ctx.eval_grad(z, rs, np.ones(5, dtype=np.int64))
    for a, b in zip(want, got):
        assert np.array_equal(a, b, equal_nan=True)
    lf.simulate_toy(seed=3)                                   # back to one set
    assert lf.ctx.T == 1 and len(lf.ctx.event_set_offsets()) == 2


def fit_each_alone(ns, variant, method, sets, prior=None, **fixed):
    from blueice_amd.profile import bestfit_batched
    lf1 = make_lf(ns, variant, method)
    if prior is not None:
        lf1.rate_parameters['s1'] = prior
    out = []
    for d in sets:
        lf1.set_data(d)
        best, ll = bestfit_batched(lf1, **fixed)
        out.append(float(ll[0]))
    return np.array(out)


@pytest.mark.parametrize('variant,method', VARIANTS)
def test_fits_of_the_ensemble_equal_fits_of_every_toy_alone(ns, variant, method):
    from blueice_amd.inference import bestfit_toys, hesse
    lf = shared_lf(ns, variant, method)
    truth, seed, counts = small_ensemble(lf, variant)
    sets = [lf.simulated_events(t) for t in range(T6)]
    calls = []
    orig = lf.ctx.fit_batched
    lf.ctx.fit_batched = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        before = lf.ctx.get_param('n_set_launches')
        best, ll = bestfit_toys(lf)
    finally:
        del lf.ctx.fit_batched
    assert calls and lf.ctx.get_param('n_set_launches') > before                  # the native loop, over k_morph_sets
    alone = fit_each_alone(ns, variant, method, sets)
    print('maxima: ensemble %r\n        alone    %r' % (list(ll), list(alone)))
    np.testing.assert_allclose(ll, alone, rtol=0, atol=1e-6)
    names, cov = hesse(lf, best, datasets=np.arange(T6))
    F = len(names)
    assert cov.shape == (T6, F, F)
    assert lf.hessian_method == 'gradient-differences'
    # The covariance of these toys.  A toy of N events constrains at most N directions of the rates (-H over the rates is
    # sum_e g_e g_e^T / lambda_e^2, of rank <= N), and the non-empty toys here have as few as one event: with every parameter
    # floating no code could return a finite (-H)^-1 for them.  So the six toys are fitted once more with one rate floating and
    # the other parameters held at the truth, where -H > 0 for every toy that has an event; test_hesse_of_an_ensemble asserts
    # the same for full-rank [F, F] covariances of toys with enough events.
    fixed = {k: v for k, v in truth.items() if k != 's0_rate_multiplier'}
    best1, ll1 = bestfit_toys(lf, **fixed)
    assert list(best1) == ['s0_rate_multiplier'] and np.isfinite(ll1).all()
    names1, cov1 = hesse(lf, best1, datasets=np.arange(T6), **fixed)
    assert names1 == ['s0_rate_multiplier'] and cov1.shape == (T6, 1, 1)
    filled = np.flatnonzero(counts.sum(axis=1) > 0)
    assert len(filled) >= 2
    for t in filled:
        assert np.isfinite(cov1[t]).all() and cov1[t, 0, 0] > 0 and np.array_equal(cov1[t], cov1[t].T), (t, cov1[t])


@pytest.mark.parametrize('variant,method', [('a', 'piecewise'), ('b', 'linear')])
def test_hesse_of_an_ensemble(ns, variant, method):
    """toys of about 140 events, every parameter floating: finite, symmetric, positive definite [T, F, F]"""
    from blueice_amd.inference import bestfit_toys, hesse
    lf = shared_lf(ns, variant, method)
    truth = truth_of(variant, s0_rate_multiplier=1.0, s1_rate_multiplier=0.5, s2_rate_multiplier=0.5)
    lf.simulate_toys(4, seed=9, **truth)
    best, ll = bestfit_toys(lf)
    ll_pts, grads, names, H = lf.values_gradients_hessians(best, dataset=np.arange(4))
    assert H.shape == (4, len(names), len(names)) and np.isfinite(H).all() and np.array_equal(H, np.swapaxes(H, 1, 2))
    cov_names, cov = hesse(lf, best, datasets=np.arange(4))
    assert cov_names == [n for n in names if n in best] and cov.shape == H.shape
    assert (lf.n_events_per_dataset > 50).all()
    for t in range(4):
        assert np.isfinite(cov[t]).all(), (t, cov[t])
        np.testing.assert_allclose(cov[t], cov[t].T, rtol=1e-12, atol=0)
        assert np.all(np.linalg.eigvalsh(0.5 * (cov[t] + cov[t].T)) > 0)


def test_toy_mc_fits_do_not_depend_on_the_chunk(ns):
    from blueice_amd.inference import toy_mc_fits
    lf = shared_lf(ns, 'b', 'piecewise')
    truth = truth_of('b', s0_rate_multiplier=0.2, s1_rate_multiplier=0.1, s2_rate_multiplier=0.1)
    events = {}
    out = {}
    for chunk in (3, 7):
        seen = []
        real = lf.simulate_toys

        def spy(n, **kw):
            c = real(n, **kw)
            off = lf.ctx.get_param('toy_offset')
            for t in range(n):
                seen.append((off + t, lf.simulated_events(t)))
            return c
        lf.simulate_toys = spy
        try:
            out[chunk] = toy_mc_fits(lf, 7, chunk=chunk, seed=21, truth=truth)
        finally:
            del lf.simulate_toys
        events[chunk] = seen
    assert [t for t, _ in events[3]] == list(range(7)) == [t for t, _ in events[7]]
    for (_, a), (_, b) in zip(events[3], events[7]):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(out[3][1], out[7][1], rtol=0, atol=1e-6)
    assert lf.ctx.get_param('toy_offset') == 0


def test_gaussian_prior_fits(ns):
    from blueice_amd import GaussianPrior
    from blueice_amd.inference import bestfit_toys
    prior = GaussianPrior(0.3, 0.1)
    lf = make_lf(ns, 'b', 'linear')
    lf.rate_parameters['s1'] = prior
    truth = truth_of('b', s0_rate_multiplier=0.2, s1_rate_multiplier=0.3, s2_rate_multiplier=0.1)
    lf.simulate_toys(T6, seed=5, **truth)
    sets = [lf.simulated_events(t) for t in range(T6)]
    calls = []
    orig = lf.ctx.fit_batched
    lf.ctx.fit_batched = lambda *a, **k: (calls.append(k.get('priors')), orig(*a, **k))[1]
    try:
        before = lf.ctx.get_param('n_set_launches')
        best, ll = bestfit_toys(lf)
    finally:
        del lf.ctx.fit_batched
    # the native loop with the constraint terms (bi_fit_batched_gauss), over k_morph_sets
    assert calls and all(p is not None for p in calls) and lf.ctx.get_param('n_set_launches') > before
    alone = fit_each_alone(ns, 'b', 'linear', sets, prior=prior)
    print('maxima with a Gaussian constraint: ensemble %r\n        alone    %r' % (list(ll), list(alone)))
    np.testing.assert_allclose(ll, alone, rtol=0, atol=1e-6)


def test_entry_points_out_of_scope_say_so(ns):
    lf = shared_lf(ns, 'b', 'piecewise')
    truth = truth_of('b', s0_rate_multiplier=0.2, s1_rate_multiplier=0.1, s2_rate_multiplier=0.1)
    lf.simulate_toys(3, seed=2, **truth)
    ctx = lf.ctx
    assert (lf.n_events_per_dataset > 0).all()
    z, rs = np.array([[0.2], [0.4]]), np.full((2, 3), 0.02)
    ds = np.array([0, 1], dtype=np.int64)
    msg = 'several event sets'
    with pytest.raises(ValueError, match=msg):
        ctx.plan(z, rs, ds)
    with pytest.raises(ValueError, match=msg):
        ctx.plan_share(z, rs, ds)
    with pytest.raises(ValueError, match=msg):
        ctx.eval_hess(z, rs, ds)
    with pytest.raises(ValueError, match=msg):
        ctx.eval_datasets(z[0], rs[0])
    with pytest.raises(ValueError, match=msg):
        ctx.eval_datasets_points(z, rs)
    zbuf = ctx.device_alloc(64)
    try:
        with pytest.raises(ValueError, match=msg):
            ctx.plan_resident(2, zbuf)
    finally:
        zbuf.free()
    W = 4
    kind, index, lo, hi = np.array([1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([0.0]), np.array([10.0])

    def sample(E, dataset, priors=None):
        return ctx.sample_stretch(W, kind, index, np.tile(z[:1], (E, 1)), np.tile(rs[:1], (E, 1)), np.ones((E, 3)), dataset,
                                  np.full((E, W, 1), 1.0), lo, hi, 2, priors=priors)
    gauss = (np.array([1.0]), np.array([0.5]), None)
    for priors in (None, gauss):                               # bi_sample_stretch and bi_sample_stretch_gauss
        with pytest.raises(ValueError, match=msg):
            sample(2, np.arange(2, dtype=np.int64), priors)    # more than one ensemble
        with pytest.raises(ValueError, match=msg):
            sample(1, np.array([1], dtype=np.int64), priors)   # one ensemble on another set than 0
    # bi_eval_full of a set other than 0: the single-point kernel over that set's columns, and that set's pdf values
    ll1, mus1, ps1, st1 = ctx.eval_full(z[0], rs[0], dataset=1)
    one, _ = ctx.eval(z[:1], rs[:1], np.array([1], dtype=np.int64))
    col = ctx.download_event_set(1)                            # [3 anchors, S, N_1]; z = 0.2 lies between anchors 0 and 1
    assert st1 == 0 and ll1 == one[0] and ps1.shape == col.shape[1:]
    np.testing.assert_allclose(ps1, 0.8 * col[1] + 0.2 * col[2], rtol=1e-13, atol=0)
    ll, st = ctx.eval(z, rs, ds)                               # the context still works
    assert np.isfinite(ll).all() and not st.any()
    ll_h = ctx.eval_hess(z, rs)[0]                             # no dataset column: set 0
    assert np.isfinite(ll_h).all()
