"""Coarse views on the device: bi_expected_coarse and bi_coarse_counts against the numpy oracle (tests/gof_oracle.py in long
double, reduced with np.add.at over `CoarseBinning.bin_map()`) at the smallest shapes that reach every path of the kernels and
for every kind of coarsening, the likelihood classes' expected_coarse / coarse_counts / gof_statistics(binning=),
goodness_of_fit(binning=) end to end, and the refusals of the C ABI.

The bar for finite values is the project's fp64 bar, 1e-10 max(1, |want|) (TOL of tests/test_gof_gpu.py); nan, +-inf, status
words and sums of integer counts are exact.  Templates are >= 0 (the floor of `case_of`), so no cell is a cancelling sum."""
from collections import OrderedDict

import numpy as np
import pytest

import gof_oracle
import model_zoo
from blueice_amd.coarse import CoarseBinning
from golden_util import load_case
from test_gof_gpu import TOL, case_of, context_of

pytestmark = pytest.mark.gpu

# k = 1: B = 63 (one leading row, one x-tile with a masked tail), B = 600 (L beyond one x-tile of 256 lanes); k = 2: 30 x 20 with
# three sources, 3 x 300 (a long last axis and few rows), 9 x 7 with two shape parameters (64 lanes, four sub-rows); k = 3:
# 5 x 4 x 7 (odd L: rows that are not 16-byte aligned).  Two more reach what these are too small for, a coarse row whose fine
# rows are dealt into several shares (at least 8 fine rows per sub-row of lanes): 33 x 9 (four sub-rows of 64 lanes, two shares)
# and 9 x 130 (one sub-row of 256 lanes, two shares)
# Cells that gather 256 partials or more are finished by a block instead of a thread: everything summed and the box at B = 600
# (one share), at 3 x 300 and, with two shares, at 9 x 130
SHAPES = OrderedDict([
    ('k1_B63_d0', dict(S=2, space=[['x', np.linspace(-4, 4, 64)]], anchors=OrderedDict())),
    ('k1_B600_d1', dict(S=2, space=[['x', np.linspace(-4, 4, 601)]], anchors=OrderedDict(shift=(-1., 0., 1.)))),
    ('k2_30x20_d1_S3', dict(S=3, space=[['x', np.linspace(-4, 4, 31)], ['y', np.linspace(0, 5, 21)]],
                            anchors=OrderedDict(shift=(-1., 0., 1.)), livetime=2.0)),
    ('k2_3x300_d1', dict(S=2, space=[['x', np.linspace(-4, 4, 4)], ['y', np.linspace(0, 5, 301)]], anchors=OrderedDict(shift=(-1., 0., 1.)))),
    ('k2_9x7_d2', dict(S=2, space=[['x', np.linspace(-4, 4, 10)], ['y', np.linspace(0, 5, 8)]],
                       anchors=OrderedDict(shift=(-1., 0., 1.), stretch=(-1., 0., 1.)))),
    ('k3_5x4x7_d1', dict(S=2, space=[['x', np.linspace(-4, 4, 6)], ['y', np.linspace(0, 5, 5)], ['w', np.linspace(-1, 1, 8)]],
                         anchors=OrderedDict(shift=(-1., 0., 1.)))),
    ('k2_33x9_d0', dict(S=2, space=[['x', np.linspace(-4, 4, 34)], ['y', np.linspace(0, 5, 10)]], anchors=OrderedDict())),
    ('k2_9x130_d1', dict(S=2, space=[['x', np.linspace(-4, 4, 10)], ['y', np.linspace(0, 5, 131)]], anchors=OrderedDict(shift=(-1., 0., 1.)))),
])


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


@pytest.fixture(scope='module')
def zoo(ns):
    """name -> (likelihood, its anchor tensors, its own data): built once, never changed by a test (tests that give a
    likelihood other data put `own_data` back)"""
    out = OrderedDict()
    for i, (name, s) in enumerate(SHAPES.items()):
        lf = model_zoo.morph_lf(ns, np.random.default_rng(300 + i), s['S'], s['space'], s['anchors'], 20000, 150, livetime=s.get('livetime'))
        out[name] = (lf, gof_oracle.tensors_of(lf), lf.ctx.download_counts(0).reshape(lf.bin_shape))
    return out


def irregular(edges):
    """edge values of irregular groups of an axis: its first fine bin alone, then up to the middle, up to the last but one ..."""
    n = len(edges) - 1
    return np.asarray(edges)[sorted({0, 1, max(n // 2, 1), max(n - 2, 1), n})]


def binnings_of(lf, space):
    """name -> CoarseBinning: identity, every single axis kept, everything summed, rebin 2 / 3 / 7 (a short last group on some
    axis in each shape), irregular groups, ranges that drop the first and last fine bins of a kept and of a summed axis, and
    one binning with all of these"""
    names = [n for n, _ in space]
    edges = {n: np.asarray(e, dtype=float) for n, e in space}
    inner = {n: (e[1], e[-2]) for n, e in edges.items()}
    out = OrderedDict(identity=CoarseBinning(lf), all_summed=CoarseBinning(lf, keep=[]))
    for n in names:
        out['keep_' + n] = CoarseBinning(lf, keep=[n])
    for m in (2, 3, 7):
        out['rebin%d' % m] = CoarseBinning(lf, rebin={n: m for n in names})
    out['irregular'] = CoarseBinning(lf, rebin={n: irregular(edges[n]) for n in names})
    first, last = names[0], names[-1]
    out['ranges_keep_first'] = CoarseBinning(lf, keep=[first], ranges={first: inner[first], last: inner[last]})
    out['ranges_keep_last'] = CoarseBinning(lf, keep=[last], ranges={first: inner[first], last: inner[last]})
    out['box'] = CoarseBinning(lf, keep=[], ranges=inner)
    rebin = {last: irregular(edges[last][1:-1])}
    if first != last:
        rebin[first] = 2
    out['combined'] = CoarseBinning(lf, keep=sorted({first, last}, key=names.index), rebin=rebin, ranges=inner)
    return out


def reduce_wide(binning, fine):
    """fine [..., B] -> [..., C] in long double with np.add.at over bin_map(): the specification"""
    m = binning.bin_map()
    inside = m >= 0
    fine = np.asarray(fine, dtype=np.longdouble)
    out = np.zeros(fine.shape[:-1] + (binning.n_cells,), dtype=np.longdouble)
    flat, dst = fine.reshape(-1, fine.shape[-1]), out.reshape(-1, binning.n_cells)
    for i in range(len(flat)):
        np.add.at(dst[i], m[inside], flat[i, inside])
    return out


def within_bar(got, want, what):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert np.all(dev <= TOL), '%s: off by %.3g of max(1, |want|)' % (what, float(dev.max()))
    return float(dev.max()) if dev.size else 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def set_binning(ctx, lf, b):
    assert ctx.set_coarse_binning(lf.bin_shape, b.groups) == b.n_cells == ctx.get_param('coarse_cells')


@pytest.mark.parametrize('name', list(SHAPES))
def test_bi_expected_coarse_against_the_oracle(zoo, name):
    """Every binning of the shape at the points of `case_of` -- on an anchor, inside a cell, on the edge of the box, outside it,
    with a negative rate --, total and per source: the oracle's coarse expectation, Σ_s per_source = total, nan in every cell
    and the oracle's status for dead points; a repeated call is bitwise equal, a point's row does not depend on the batch, and
    the identity binning agrees with bi_expected_counts."""
    lf = zoo[name][0]
    model, counts, zs, rs, ds, dead = case_of(zoo[name][1], seed=17)
    T = len(counts)
    zs, rs = zs[::T], rs[::T]
    P, d, S = len(zs), zs.shape[1], rs.shape[1]
    status = np.array([gof_oracle.point(model, counts[1], zs[p], rs[p])[2] for p in range(P)], dtype=np.int32)
    live = status == 0
    assert list(live) == [True, True, True, d == 0, False]
    mu_sources = {p: gof_oracle.statistics(model, counts[1], zs[p], rs[p], dtype=np.longdouble)['mu_sources'] for p in np.flatnonzero(live)}
    ctx = context_of(model, counts, 0)
    worst = 0.0
    try:
        fine = ctx.expected_counts(zs if d else None, rs)
        for label, b in binnings_of(lf, SHAPES[name]['space']).items():
            what = '%s, %s' % (name, label)
            set_binning(ctx, lf, b)
            total, st = ctx.expected_coarse(b.n_cells, zs if d else None, rs)
            parts, st2 = ctx.expected_coarse(b.n_cells, zs if d else None, rs, per_source=True)
            assert total.shape == (P, b.n_cells) and parts.shape == (P, S, b.n_cells)
            assert np.array_equal(st, status) and np.array_equal(st2, status), what
            assert np.isnan(total[~live]).all() and np.isnan(parts[~live]).all(), what
            for p in np.flatnonzero(live):
                want = reduce_wide(b, mu_sources[p])                                 # [S, C]
                want_total = want.sum(axis=0)
                worst = max(worst, within_bar(parts[p], want, what + ', per source, point %d' % p),
                            within_bar(total[p], want_total, what + ', total, point %d' % p),
                            within_bar(parts[p].sum(axis=0), total[p], what + ', sum of the sources, point %d' % p))
                if label == 'all_summed':
                    within_bar(total[p, 0], mu_sources[p].sum(), what + ', against the sum over all bins')
                if label == 'identity':                  # one fine bin per cell, the same fma chain: the same bits
                    assert np.array_equal(bits(total[p]), bits(fine[p])), what + ', against bi_expected_counts'
            # the same call again, and the second point alone: the same bits
            again, _ = ctx.expected_coarse(b.n_cells, zs if d else None, rs)
            assert np.array_equal(bits(again), bits(total)), what
            again, _ = ctx.expected_coarse(b.n_cells, zs if d else None, rs, per_source=True)
            assert np.array_equal(bits(again), bits(parts)), what
            alone, _ = ctx.expected_coarse(b.n_cells, zs[1:2] if d else None, rs[1:2])
            assert np.array_equal(bits(alone[0]), bits(total[1])), what
        assert ctx.set_coarse_binning() == 0 and ctx.get_param('coarse_cells') == 0
    finally:
        ctx.close()
    print('%s: largest deviation %.3g of max(1, |want|)' % (name, worst))


@pytest.mark.parametrize('name', list(SHAPES))
def test_bi_coarse_counts_of_uploaded_data(zoo, name):
    """Uploaded data in dense form (sparse = 0) and with sparse = 2: exactly np.bincount over bin_map of the downloaded counts,
    for every binning, all datasets or a list of them; a dataset with non-integer counts to the bar."""
    lf = zoo[name][0]
    model, counts, _, _, _, _ = case_of(zoo[name][1], seed=18)
    binnings = binnings_of(lf, SHAPES[name]['space'])
    for sparse in (0, 2):
        ctx = context_of(model, counts, sparse)
        try:
            assert ctx.get_param('dense_counts') == 1
            down = np.stack([ctx.download_counts(t) for t in range(len(counts))])
            assert np.array_equal(down, counts)
            for label, b in binnings.items():
                set_binning(ctx, lf, b)
                m = b.bin_map()
                want = np.stack([np.bincount(m[m >= 0], weights=row[m >= 0], minlength=b.n_cells) for row in down])
                got = ctx.coarse_counts(b.n_cells)
                assert got.shape == want.shape and np.array_equal(got, want), '%s, %s, sparse = %d' % (name, label, sparse)
                assert np.array_equal(ctx.coarse_counts(b.n_cells, [2, 0, 2]), want[[2, 0, 2]])
                assert np.array_equal(bits(ctx.coarse_counts(b.n_cells)), bits(got))
            with pytest.raises(ValueError, match='outside'):
                ctx.coarse_counts(b.n_cells, [0, 3])
        finally:
            ctx.close()
    real = counts[0] * 0.37 + 0.125 * (np.arange(counts.shape[1]) % 5)
    ctx = context_of(model, real[None, :], 0)
    try:
        for label, b in binnings.items():
            set_binning(ctx, lf, b)
            got = ctx.coarse_counts(b.n_cells)
            within_bar(got[0], reduce_wide(b, real), '%s, %s, real-valued counts' % (name, label))
            assert np.array_equal(bits(ctx.coarse_counts(b.n_cells)), bits(got))
    finally:
        ctx.close()


@pytest.mark.parametrize('name', ['k1_B600_d1', 'k2_30x20_d1_S3', 'k3_5x4x7_d1'])
def test_coarse_counts_of_device_generated_toys(zoo, name):
    """Toys of simulate_toys exist as non-empty-bin lists only: the list kernel, exactly np.bincount of every toy's downloaded
    counts; the likelihood's method gives the same in the binning's shape."""
    lf, _, own_data = zoo[name]
    T = 6
    try:
        lf.simulate_toys(T, seed=5, s0_rate_multiplier=1.2, **({'shift': 0.3} if lf.shape_parameters else {}))
        assert lf.ctx.get_param('dense_counts') == 0 and lf.ctx.T == T
        down = np.stack([lf.ctx.download_counts(t) for t in range(T)])
        assert down.sum() > 0
        for label, b in binnings_of(lf, SHAPES[name]['space']).items():
            m = b.bin_map()
            want = np.stack([np.bincount(m[m >= 0], weights=row[m >= 0], minlength=b.n_cells) for row in down])
            got = lf.coarse_counts(b)
            assert got.shape == (T,) + b.shape and np.array_equal(got.reshape(T, -1), want), '%s, %s' % (name, label)
            assert np.array_equal(lf.coarse_counts(b, datasets=[4, 1]).reshape(2, -1), want[[4, 1]])
        assert lf.ctx.get_param('dense_counts') == 0
    finally:
        lf.set_binned_data(own_data)


@pytest.mark.parametrize('name', ['k2_30x20_d1_S3', 'k2_9x7_d2', 'k3_5x4x7_d1'])
def test_likelihood_methods_and_gof_statistics_with_a_binning(zoo, name):
    """expected_coarse / expected_coarse_points with the host terms of the likelihood (rate multipliers, live time), and
    gof_statistics(binning=) -- every point against every dataset -- against the numpy statistic of the oracle's coarse arrays;
    with the identity binning it equals the statistic over the fine bins."""
    lf, model, own_data = zoo[name]
    S, B = len(lf.source_name_list), int(np.prod(lf.bin_shape))
    base_livetime = SHAPES[name].get('livetime')
    livetime = 5.0 if base_livetime else None
    factor = livetime / base_livetime if livetime else 1.0
    shape_names = list(lf.shape_parameters)
    zs = np.array([[0.0, 0.0], [0.37, -0.62], [1.0, -1.0], [1.5, 0.0], [-0.4, 0.8]])[:, :len(shape_names)]
    mult = np.random.default_rng(21).uniform(0.6, 1.5, size=(5, S))
    mult[4, 0] = -0.5
    P = len(zs)
    status = np.array([gof_oracle.point(model, own_data, zs[p], mult[p] * factor)[2] for p in range(P)])
    live = status == 0
    mu_sources = {p: gof_oracle.statistics(model, own_data, zs[p], mult[p] * factor, dtype=np.longdouble)['mu_sources'] for p in np.flatnonzero(live)}
    centre = np.asarray(mu_sources[0].sum(axis=0), dtype=float)
    nothing_expected = np.flatnonzero(np.all(np.asarray(model['ps']).reshape(-1, B) == 0, axis=0))
    lone = np.zeros(B)
    lone[nothing_expected[:1]] = 1.0                 # one event in a fine bin where no template expects anything (if there is one)
    data = np.stack([own_data.ravel(), lone, np.random.default_rng(22).poisson(centre).astype(float)])
    T = len(data)
    points = {k: zs[:, i] for i, k in enumerate(shape_names)}
    points.update({'s%d_rate_multiplier' % s: mult[:, s] for s in range(S)})
    every = {k: np.repeat(v, T) for k, v in points.items()}
    ds = np.tile(np.arange(T), P)
    other = CoarseBinning(zoo['k3_5x4x7_d1' if name != 'k3_5x4x7_d1' else 'k2_9x7_d2'][0], keep=['x'])
    for call in (lambda: lf.expected_coarse(other), lambda: lf.coarse_counts(other), lambda: lf.gof_statistics(binning=other)):
        with pytest.raises(ValueError, match='another analysis space'):
            call()                                   # a binning belongs to the analysis space it was made for
    with pytest.raises(TypeError):
        lf.expected_coarse(np.arange(3))
    try:
        lf.set_binned_data(data.reshape((T,) + tuple(lf.bin_shape)))
        fine = lf.gof_statistics(points=every, datasets=ds, livetime_days=livetime)
        for label, b in binnings_of(lf, SHAPES[name]['space']).items():
            what = '%s, %s' % (name, label)
            many = lf.expected_coarse_points(b, points, livetime_days=livetime)
            parts = lf.expected_coarse_points(b, points, per_source=True, livetime_days=livetime)
            assert many.shape == (P,) + b.shape and parts.shape == (P, S) + b.shape
            assert np.isnan(many[~live]).all() and np.isnan(parts[~live]).all()
            one = lf.expected_coarse(b, livetime_days=livetime, **{k: v[1] for k, v in points.items()})
            assert one.shape == b.shape and np.array_equal(bits(one), bits(many[1]))
            one = lf.expected_coarse(b, per_source=True, livetime_days=livetime, **{k: v[1] for k, v in points.items()})
            assert one.shape == (S,) + b.shape and np.array_equal(bits(one), bits(parts[1]))
            assert np.isnan(lf.expected_coarse(b, livetime_days=livetime, **{k: v[4] for k, v in points.items()})).all()
            n_coarse = reduce_wide(b, data)
            assert np.array_equal(lf.coarse_counts(b).reshape(T, -1), np.asarray(n_coarse, dtype=float))
            got = lf.gof_statistics(points=every, datasets=ds, livetime_days=livetime, binning=b)
            assert got['n_bins'] == b.n_cells and np.array_equal(got['status'], np.repeat(status, T))
            assert np.array_equal(got['n_events'], np.tile(np.asarray(n_coarse.sum(axis=1), dtype=float), P))
            for p in range(P):
                for t in range(T):
                    i = p * T + t
                    if not live[p]:
                        assert got['deviance'][i] == np.inf and got['pearson'][i] == np.inf
                        continue
                    mu = reduce_wide(b, mu_sources[p])
                    within_bar(parts[p].reshape(S, -1), mu, what + ', per source')
                    within_bar(many[p].ravel(), mu.sum(axis=0), what + ', total')
                    half, pearson = gof_oracle.per_bin(n_coarse[t], mu.sum(axis=0))
                    for key, want in (('deviance', 2 * half.sum()), ('pearson', pearson.sum())):
                        if np.isfinite(want):
                            within_bar(got[key][i], want, '%s, %s of point %d against dataset %d' % (what, key, p, t))
                        else:
                            assert got[key][i] == want, (what, key, p, t)
                    if label == 'identity' and np.isfinite(fine['deviance'][i]):
                        within_bar(got['deviance'][i], fine['deviance'][i], what + ', deviance over the fine bins')
                        within_bar(got['pearson'][i], fine['pearson'][i], what + ', Pearson over the fine bins')
        # an event in a fine bin without expectation: +inf over the fine bins, finite over cells that expect something
        if len(nothing_expected):
            assert np.all(fine['deviance'][np.repeat(live, T) & (ds == 1)] == np.inf)
        coarse = lf.gof_statistics(points=every, datasets=ds, livetime_days=livetime, binning=CoarseBinning(lf, keep=[]))
        assert np.all(np.isfinite(coarse['deviance'][np.repeat(live, T)])) and np.all(np.isfinite(coarse['pearson'][np.repeat(live, T)]))
    finally:
        lf.set_binned_data(own_data)


def test_goodness_of_fit_with_a_binning_end_to_end(zoo):
    """goodness_of_fit(binning=, n_toys=24) on the 30 x 20 model: finite toys, 0 < p <= 1, ndof = C - n_floating, the toys THE SAME
    ARRAY for chunk=7 and chunk=24 (toy j is toy j of the seed's ensemble whatever the chunk, and neither the coarse statistic of
    a point nor its fit depends on the batch it is in), the observed statistic against the numpy statistic of the oracle's
    coarse arrays, and the likelihood's own data back afterwards."""
    lf, model, own_data = zoo['k2_30x20_d1_S3']
    b = CoarseBinning(lf, rebin=dict(x=5, y=4))
    try:
        truth = dict(shift=0.2, s0_rate_multiplier=1.1)
        data = np.random.default_rng(31).poisson(lf.expected_counts(**truth)).astype(float)
        lf.set_binned_data(data)
        best, _ = lf.bestfit_device()
        before = lf(**best)
        res = {}
        for chunk in (7, 24):
            res[chunk] = lf.goodness_of_fit(n_toys=24, chunk=chunk, seed=13, binning=b)
            assert lf(**best) == before and lf.ctx.get_param('toy_offset') == 0                 # the data are back
            np.testing.assert_array_equal(lf.ctx.download_counts(0), data.ravel())
        a, c = res[7], res[24]
        print('toys, chunk 7 against chunk 24: largest difference %.3g' % np.max(np.abs(a.toys - c.toys)))
        np.testing.assert_array_equal(a.toys, c.toys)                                  # the same array
        assert a.toys.shape == (24,) and np.all(np.isfinite(a.toys)) and 0 < a.p_value <= 1 and a.p_value == c.p_value
        assert a.ndof == b.n_cells - len(a.best) == 30 - 4
        z, mult = [a.best['shift']], [a.best['s%d_rate_multiplier' % s] for s in range(3)]
        mu = reduce_wide(b, gof_oracle.statistics(model, data, z, mult, dtype=np.longdouble)['mu'])
        half, _ = gof_oracle.per_bin(reduce_wide(b, data.ravel()), mu)
        within_bar(a.observed, 2 * half.sum(), 'observed deviance over the cells')
        fine = lf.goodness_of_fit(n_toys=4, seed=13)
        assert fine.ndof == 600 - 4 and list(fine.best) == list(a.best)         # binning=None: as before
    finally:
        lf.set_binned_data(own_data)


def test_the_c_abi_refusals(zoo):
    """Every BI_ERR_INVALID of bi_set_coarse_binning, the calls without a binning, a binning that a new model releases, and
    Beeston-Barlow and unbinned contexts."""
    from blueice_amd.device import DeviceContext
    from blueice_amd.exceptions import NotPreparedException
    model, counts, zs, rs, _, _ = case_of(zoo['k2_9x7_d2'][1], seed=19)
    ctx = context_of(model, counts, 0)
    try:
        for what in (lambda: ctx.expected_coarse(1, zs, rs), lambda: ctx.coarse_counts(1)):
            with pytest.raises(NotPreparedException, match='no coarse binning'):
                what()
        good = [[0, 4, 9], [1, 2, 7]]
        assert ctx.set_coarse_binning([9, 7], good) == 4
        for n_fine, groups, match in (([9, 8], good, 'fine bins'), ([63], [[0, 63, 64]], 'leave'), ([9, 7], [[0, 4, 4, 9], [0, 7]], 'ascending'),
                                      ([9, 7], [[0, 9], [3, 2]], 'ascending'), ([9, 7], [[-1, 9], [0, 7]], 'leave'),
                                      ([9, 7], [[0, 10], [0, 7]], 'leave'), ([9, 7], [[0, 9], [7]], 'groups'), ([3, 3, 8], [[0, 3]] * 3, 'fine bins')):
            with pytest.raises(ValueError, match=match):
                ctx.set_coarse_binning(n_fine, groups)
            assert ctx.get_param('coarse_cells') == 4                           # a refused binning leaves the one that was set
        mu, st = ctx.expected_coarse(4, zs[:1], rs[:1])
        assert st[0] == 0 and np.all(np.isfinite(mu))
        ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])          # a new model releases it
        assert ctx.get_param('coarse_cells') == 0
        ctx.upload_counts(counts)
        for what in (lambda: ctx.expected_coarse(4, zs, rs), lambda: ctx.coarse_counts(4)):
            with pytest.raises(NotPreparedException, match='no coarse binning'):
                what()
        assert ctx.set_coarse_binning([9, 7], good) == 4 and ctx.set_coarse_binning() == 0
        ll, st = ctx.eval(zs[:1], rs[:1])                                       # the context is as usable as before
        assert np.isfinite(ll[0]) and st[0] == 0
    finally:
        ctx.close()
    c = load_case('ref_bb_multi_bin')
    ctx = DeviceContext(0)
    try:
        ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'], n_model=c['model']['n_model'], bb_source=c['bb_source'])
        ctx.upload_counts(c['counts'])
        with pytest.raises(ValueError, match='Beeston-Barlow'):
            ctx.set_coarse_binning([ctx.B], [[0, ctx.B]])
        with pytest.raises(ValueError, match='Beeston-Barlow'):
            ctx.expected_coarse(1, None, np.ones((1, c['S'])))
        with pytest.raises(ValueError, match='Beeston-Barlow'):
            ctx.coarse_counts(1)
        assert ctx.set_coarse_binning() == 0                                    # clearing is always possible
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
            ctx.set_coarse_binning([n_ev], [[0, n_ev]])
        with pytest.raises(ValueError, match='unbinned'):
            ctx.expected_coarse(1, None, np.ones((1, c['S'])))
    finally:
        ctx.close()
