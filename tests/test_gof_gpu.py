"""Goodness of fit on the device: bi_eval_gof and bi_expected_counts against the numpy oracle (tests/gof_oracle.py) at every
shape and in every form of the data, the likelihood classes' expected_counts / gof_statistics, goodness_of_fit end to end,
and the refusals of the C ABI.

The bar for finite values is the project's fp64 bar, 1e-10 max(1, |want|) (the value kernels' own); +-inf, nan and the status
words are exact."""
from collections import OrderedDict

import numpy as np
import pytest

import gof_oracle
import model_zoo
from golden_util import load_case, same
from oracle import blueice_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-10

# the smallest shapes that reach every path: B = 63 (one masked tile of 512 bins), B = 600 (two tiles, the second with a
# masked tail), 2 and 3 sources, no shape parameter / one with 3 anchors / two with 3 x 3 anchors
SHAPES = OrderedDict([
    ('d0_S2_B63', dict(S=2, space=[['x', np.linspace(-4, 4, 64)]], anchors=OrderedDict())),
    ('d1_S3_B600', dict(S=3, space=[['x', np.linspace(-4, 4, 31)], ['y', np.linspace(0, 5, 21)]],
                        anchors=OrderedDict(shift=(-1., 0., 1.)), livetime=2.0)),
    ('d2_S2_B63', dict(S=2, space=[['x', np.linspace(-4, 4, 10)], ['y', np.linspace(0, 5, 8)]],
                       anchors=OrderedDict(shift=(-1., 0., 1.), stretch=(-1., 0., 1.)))),
])


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


@pytest.fixture(scope='module')
def zoo(ns):
    """name -> (likelihood, its anchor tensors): built once, never changed by a test (tests that give a likelihood other
    data put `own_data` back)"""
    out = OrderedDict()
    for i, (name, s) in enumerate(SHAPES.items()):
        lf = model_zoo.morph_lf(ns, np.random.default_rng(100 + i), s['S'], s['space'], s['anchors'], 20000, 150, livetime=s.get('livetime'))
        out[name] = (lf, gof_oracle.tensors_of(lf), lf.ctx.download_counts(0).reshape(lf.bin_shape))
    return out


def case_of(model, seed):
    """The tensors of a shape with a floor under every template and one bin in which every template is 0, three datasets -- most bins filled (none in that
    bin), all zeros, few events and one of them in that bin -- and the points: on an anchor, inside a cell, on the edge of
    the box, outside it, with a negative rate; every point against every dataset."""
    rng = np.random.default_rng(seed)
    d, S = len(model['anchor_z']), model['mus'].shape[-1]
    B = model['ps'].shape[-1]
    ps = np.array(model['ps'], dtype=float) + 0.25 / B       # (no other bin without expectation: sampled templates have many)
    dead = B // 3
    ps[..., dead] = 0.0
    model = dict(model, ps=ps)
    centre = gof_oracle.statistics(model, np.zeros(B), [0.0] * d, np.ones(S))['mu']
    filled = rng.poisson(centre + 4.0).astype(float)
    filled[dead] = 0.0
    few = rng.poisson(0.3 * centre).astype(float)
    few[dead] = 1.0
    counts = np.stack([filled, np.zeros(B), few])
    zs = np.array([[0.0] * d, [0.37, -0.62][:d], [1.0, -1.0][:d], [1.5, 0.0][:d], [-0.4, 0.8][:d]], dtype=float).reshape(5, d)
    rs = rng.uniform(0.6, 1.5, size=(5, S))
    rs[4, 0] = -0.5
    P, T = len(zs), len(counts)
    return model, counts, np.repeat(zs, T, axis=0), np.repeat(rs, T, axis=0), np.tile(np.arange(T), P), dead


def context_of(model, counts, sparse, allow_negative=None):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', sparse)
    ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])
    if allow_negative is not None:
        ctx.set_allow_negative([1 if a else 0 for a in allow_negative])
    ctx.upload_counts(counts)
    return ctx


def check_against_oracle(got, model, counts, zs, rs, ds, allow_negative=None, what=''):
    hd, pe, st = got
    worst = 0.0
    for p in range(len(ds)):
        want = gof_oracle.point(model, counts[ds[p]], zs[p], rs[p], allow_negative)
        assert st[p] == want[2], '%s point %d: status %d, want %d' % (what, p, st[p], want[2])
        for name, g, w in (('half-deviance', hd[p], want[0]), ('pearson', pe[p], want[1])):
            if np.isfinite(w):
                worst = max(worst, abs(g - w) / max(1.0, abs(w)))
                assert abs(g - w) <= TOL * max(1.0, abs(w)), '%s point %d %s: %r, want %r' % (what, p, name, g, w)
            else:
                assert (np.isnan(g) if np.isnan(w) else g == w), '%s point %d %s: %r, want %r' % (what, p, name, g, w)
    print('%s: largest deviation %.3g of max(1, |want|)' % (what, worst))


@pytest.mark.parametrize('name', list(SHAPES))
def test_bi_eval_gof_against_the_oracle_in_both_forms(zoo, name):
    """Every shape, dense (sparse = 0) and non-empty-bin form (sparse = 2) of one context's data, every point against every
    dataset in one call: the oracle's values, its +inf (outside the box, a negative rate, an event in the bin where every
    template is 0) and its status words; and the two forms agree."""
    model, counts, zs, rs, ds, dead = case_of(zoo[name][1], seed=7)
    d = zs.shape[1]
    results = {}
    for form, sparse in (('dense', 0), ('non-empty bins', 2)):
        ctx = context_of(model, counts, sparse)
        try:
            results[form] = ctx.eval_gof(zs if d else None, rs, ds)
            check_against_oracle(results[form], model, counts, zs, rs, ds, what='%s, %s' % (name, form))
            if sparse:                     # the form under test really is the compacted one: dataset 0 fills more than one tile at B = 600
                assert np.count_nonzero(counts[0]) > 512 or counts.shape[1] < 512
        finally:
            ctx.close()
    a, b = results['dense'], results['non-empty bins']
    assert np.array_equal(a[2], b[2])
    live = (a[2] == 0)
    assert np.array_equal(live, np.repeat([True, True, True, d == 0, False], 3))     # (no box without shape parameters)
    assert np.all(np.isinf(a[0][ds == 2])) and np.all(a[0][~live] == np.inf) and np.all(a[1][~live] == np.inf)
    assert np.all(np.isfinite(a[0][live & (ds != 2)])) and np.all(np.isfinite(a[1][live & (ds != 2)]))
    for x, y in zip(a[:2], b[:2]):
        fin = np.isfinite(x)
        assert np.array_equal(fin, np.isfinite(y)) and np.array_equal(x[~fin], y[~fin])
        assert np.all(np.abs(x[fin] - y[fin]) <= TOL * np.maximum(1.0, np.abs(x[fin])))


@pytest.mark.parametrize('name', ['d1_S3_B600', 'd2_S2_B63'])
def test_bi_eval_gof_dense_through_a_source_that_may_go_negative(zoo, name):
    """sparse = 2 with an allow-negative source: the dense form is forced.  A negative rate of that source is physical while
    the summed rate is not negative; where a bin's expectation goes negative both statistics are nan, as ll is."""
    model, counts, zs, rs, ds, dead = case_of(zoo[name][1], seed=8)
    S = rs.shape[1]
    allow = [False] * (S - 1) + [True]
    rs[3:6, S - 1] = -0.05                  # the point inside a cell: slightly negative
    rs[6:9, S - 1] = -0.5 * (model['mus'][..., :S - 1].sum(axis=-1).min() / model['mus'][..., S - 1].max())    # the point on the edge: strongly
    ctx = context_of(model, counts, 2, allow)
    try:
        got = ctx.eval_gof(zs, rs, ds)
        ll, st = ctx.eval(zs, rs, ds)
        check_against_oracle(got, model, counts, zs, rs, ds, allow, what='%s, allow-negative' % name)
        assert np.array_equal(st, got[2])
        assert np.array_equal(np.isnan(ll), np.isnan(got[0])) and np.array_equal(ll == -np.inf, got[0] == np.inf)
        assert np.array_equal(np.isnan(got[0]), np.isnan(got[1])) and np.array_equal(got[0] == np.inf, got[1] == np.inf)
    finally:
        ctx.close()


def test_bi_eval_gof_on_device_generated_toys(zoo):
    """Toys of simulate_toys exist as non-empty-bin lists only: every toy at a point of its own against the oracle on the
    toy's downloaded counts."""
    lf, model, own_data = zoo['d1_S3_B600']
    T = 8
    try:
        lf.simulate_toys(T, seed=3, shift=0.2, s0_rate_multiplier=1.1)
        rng = np.random.default_rng(4)
        zs, rs = rng.uniform(-1, 1, size=(T, 1)), rng.uniform(0.7, 1.4, size=(T, 3))
        ds = np.arange(T)
        counts = np.stack([lf.ctx.download_counts(t) for t in range(T)])
        assert counts.sum() > 0 and lf.ctx.get_param('sparse') != 0
        check_against_oracle(lf.ctx.eval_gof(zs, rs, ds), model, counts, zs, rs, ds, what='device toys')
    finally:
        lf.set_binned_data(own_data)


@pytest.mark.parametrize('name', list(SHAPES))
def test_expected_counts_against_the_oracle(zoo, name):
    lf, model, own_data = zoo[name]
    S, shape = len(lf.source_name_list), tuple(lf.bin_shape)
    params = dict(zip(lf.shape_parameters, (0.37, -0.62)))
    params.update(s0_rate_multiplier=1.3, s1_rate_multiplier=0.6)
    livetime = 5.0 if SHAPES[name].get('livetime') else None
    z = [params[k] for k in lf.shape_parameters]
    rs = np.array([1.3, 0.6] + [1.0] * (S - 2)) * (livetime / SHAPES[name]['livetime'] if livetime else 1.0)
    want = gof_oracle.statistics(model, own_data, z, rs)
    total = lf.expected_counts(livetime_days=livetime, **params)
    parts = lf.expected_counts(per_source=True, livetime_days=livetime, **params)
    assert total.shape == shape and parts.shape == (S,) + shape
    print('%s: total within %.3g, per source within %.3g (relative)' % (
        name, np.max(np.abs(total.ravel() - want['mu']) / np.where(want['mu'] > 0, want['mu'], 1.0)),
        np.max(np.abs(parts.reshape(S, -1) - want['mu_sources']) / np.where(want['mu_sources'] > 0, want['mu_sources'], 1.0))))
    np.testing.assert_allclose(total.ravel(), want['mu'], rtol=TOL, atol=0)
    np.testing.assert_allclose(parts.reshape(S, -1), want['mu_sources'], rtol=TOL, atol=0)
    np.testing.assert_allclose(parts.sum(axis=0), total, rtol=1e-13, atol=0)
    # the likelihood of the returned expectation is the likelihood (no priors here)
    ll = lf(livetime_days=livetime, **params)
    assert same(np.sum(orc.poisson_logpmf(own_data.ravel(), total.ravel())), ll, TOL) and abs(ll) > 1
    # several points in one call, one of them outside the box (no box without shape parameters: a negative rate then)
    pts = {k: np.array([v, v, v]) for k, v in params.items()}
    if lf.shape_parameters:
        pts[list(lf.shape_parameters)[0]] = np.array([0.37, 1.5, -1.0])
    else:
        pts['s0_rate_multiplier'] = np.array([1.3, -1.0, 0.2])
    many = lf.expected_counts_points(pts, livetime_days=livetime)
    assert many.shape == (3,) + shape and np.isnan(many[1]).all() and np.isfinite(many[2]).all()
    np.testing.assert_allclose(many[0], total, rtol=1e-14, atol=0)
    # the statistics from nothing but the device: its expectation and its counts
    stats_ = lf.gof_statistics(points=pts, livetime_days=livetime)
    n = lf.ctx.download_counts(0)
    for p in (0, 2):
        half, pearson = gof_oracle.per_bin(n, many[p].ravel())
        assert same(stats_['deviance'][p], 2 * half.sum(), TOL) and same(stats_['pearson'][p], pearson.sum(), TOL)
    assert stats_['deviance'][1] == np.inf and stats_['pearson'][1] == np.inf and stats_['status'][1] != 0
    assert stats_['n_bins'] == int(np.prod(shape)) and np.all(stats_['n_events'] == n.sum())


@pytest.fixture(scope='module')
def fit_lf(ns):
    """Two sources, one shape parameter with 3 anchors, 25 x 25 bins"""
    space = [['x', np.linspace(-4, 4, 26)], ['y', np.linspace(0, 5, 26)]]
    lf = model_zoo.morph_lf(ns, np.random.default_rng(77), 2, space, OrderedDict(shift=(-1., 0., 1.)), 30000, 130)
    # data that the model can describe: drawn from its own expectation (sampled templates have bins without any)
    lf.set_binned_data(np.random.default_rng(78).poisson(lf.expected_counts(shift=0.2, s0_rate_multiplier=1.1)).astype(float))
    return lf


@pytest.mark.parametrize('statistic', ['deviance', 'pearson'])
def test_goodness_of_fit_end_to_end(fit_lf, statistic):
    from blueice_amd.inference import toy_p_value
    lf = fit_lf
    model = gof_oracle.tensors_of(lf)
    data = lf.ctx.download_counts(0)
    n_toys, seed = 64, 11
    best, _ = lf.bestfit_device()
    before = lf(**best)
    a = lf.goodness_of_fit(n_toys=n_toys, statistic=statistic, chunk=16, seed=seed)
    assert lf(**best) == before and lf.ctx.get_param('toy_offset') == 0          # the data are back
    np.testing.assert_array_equal(lf.ctx.download_counts(0), data)
    b = lf.goodness_of_fit(n_toys=n_toys, statistic=statistic, chunk=64, seed=seed)
    assert lf(**best) == before and lf.ctx.get_param('toy_offset') == 0
    # the ensemble does not depend on the chunk
    np.testing.assert_allclose(a.toys, b.toys, rtol=1e-9, atol=1e-9)
    assert list(a.toy_best) == list(b.toy_best) == list(a.best) == ['s0_rate_multiplier', 's1_rate_multiplier', 'shift']
    for k in a.toy_best:
        np.testing.assert_allclose(a.toy_best[k], b.toy_best[k], rtol=1e-9, atol=1e-9)
    assert a.p_value == b.p_value and np.array_equal(a.failed, b.failed)
    assert a.p_value == toy_p_value(a.observed, a.toys, a.failed) and a.n_failed == np.count_nonzero(a.failed)
    assert a.ndof == 625 - 3 and 0 < a.p_value <= 1 and a.toys.shape == (n_toys,) and np.all(np.isfinite(a.toys))
    # the observed statistic, and every toy of the last chunk at its own fit, against the oracle on the downloaded counts
    key = {'deviance': 'half_deviance', 'pearson': 'pearson'}[statistic]
    factor = 2.0 if statistic == 'deviance' else 1.0
    want = factor * gof_oracle.statistics(model, data, [a.best['shift']], [a.best['s0_rate_multiplier'], a.best['s1_rate_multiplier']])[key]
    assert abs(a.observed - want) <= TOL * max(1.0, want)
    try:
        lf.ctx.set_param('toy_offset', 48)
        lf.simulate_toys(16, seed=seed, **a.best)
        for j in range(16):
            t = 48 + j
            want = factor * gof_oracle.statistics(model, lf.ctx.download_counts(j), [a.toy_best['shift'][t]],
                                                  [a.toy_best['s0_rate_multiplier'][t], a.toy_best['s1_rate_multiplier'][t]])[key]
            assert abs(a.toys[t] - want) <= TOL * max(1.0, want), (t, a.toys[t], want)
    finally:
        lf.ctx.set_param('toy_offset', 0)
        lf.set_binned_data(data.reshape(lf.bin_shape))


def test_the_c_abi_refuses_beeston_barlow_and_unbinned_contexts():
    """A plain error return (BI_ERR_INVALID -> ValueError) with a message, from both entry points."""
    from blueice_amd.device import DeviceContext
    c = load_case('ref_bb_multi_bin')
    ctx = DeviceContext(0)
    try:
        ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'], n_model=c['model']['n_model'], bb_source=c['bb_source'])
        ctx.upload_counts(c['counts'])
        with pytest.raises(ValueError, match='Beeston-Barlow'):
            ctx.eval_gof(None, np.ones((1, c['S'])))
        with pytest.raises(ValueError, match='Beeston-Barlow'):
            ctx.expected_counts(None, np.ones((1, c['S'])))
        ll, st = ctx.eval(None, np.ones((1, c['S'])))          # the context is as usable as before
        assert np.isfinite(ll[0]) and st[0] == 0
    finally:
        ctx.close()
    c = load_case('unb_d0_three_sources')
    ctx = DeviceContext(0)
    try:
        n_ev = c['bins'][0]
        ctx.begin_model(c['model']['anchor_z'], c['S'], n_ev)
        ctx.set_anchor(0, np.asarray(c['model']['ps']).reshape(c['S'], n_ev), np.asarray(c['model']['mus']).reshape(c['S']))
        ctx.end_model()
        ctx.set_unbinned(c['outlier'])
        with pytest.raises(ValueError, match='unbinned'):
            ctx.eval_gof(None, np.ones((1, c['S'])))
        with pytest.raises(ValueError, match='unbinned'):
            ctx.expected_counts(None, np.ones((1, c['S'])))
    finally:
        ctx.close()
