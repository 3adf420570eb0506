"""Coarse views of a source-wise model on the device: bi_sourcewise_expected_coarse and bi_sourcewise_coarse_counts against the
exact oracle (sourcewise_toy_cases.exact_expectation in long double, reduced with np.add.at over the cell map of the binning) at
the smallest fine shapes that reach every path of k_sourcewise_coarse and the finish kernels and for every kind of coarsening,
the nine (source slots, own axes) classes with and without per-source sums, the functions of blueice_amd.coarse and
gof_statistics(binning=) / goodness_of_fit(binning=) on a SourceWiseBinnedLogLikelihood end to end, and the refusals of the C ABI.

The bar for finite values is the project's fp64 bar, 1e-10 max(1, |want|) (TOL of tests/test_gof_gpu.py); nan, status words and
sums of integer counts are exact.  Templates are >= 0, so no cell is a cancelling sum."""
from collections import OrderedDict

import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_toy_cases as cases
from test_gof_gpu import TOL

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL = 1, 2

# (63,): one leading row, one x-tile with a masked tail; (600,): several x-tiles of 256 lanes, everything summed through the wide
# finish; (9, 7): 64 lanes, four sub-rows; (5, 4, 7): odd L, rows that are not 16-byte aligned; (33, 9): two shares at TX = 64;
# (9, 130): two shares at TX = 256, the wide finish with two shares; (3, 300): a long last axis and few rows
SHAPES = [(63,), (600,), (9, 7), (5, 4, 7), (33, 9), (9, 130), (3, 300)]
CLASS_SHAPE = (13, 79)          # B = 1027, the bins of the nine class models: 128 lanes, two sub-rows


def irregular(n):
    """irregular groups of n fine bins: the first alone, then up to the middle, up to the last but one ..."""
    return sorted({0, 1, max(n // 2, 1), max(n - 2, 1), n})


def binnings_of(shape, few=False):
    """name -> groups (per axis the ascending fine-bin boundaries): the set `binnings_of` of test_coarse_gpu.py builds, restated for
    a fine shape -- identity, every single axis kept, everything summed, rebin 2 / 3 / 7, irregular groups, ranges that drop
    the first and last fine bins of a kept and of a summed axis, the box, and one binning with all of these.  few: identity, one
    kept axis, everything summed and the combined binning."""
    k = len(shape)
    fine = [list(range(n + 1)) for n in shape]
    whole = [[0, n] for n in shape]
    inner = [[1, n - 1] for n in shape]
    inner_fine = [list(range(1, n)) for n in shape]
    out = OrderedDict(identity=fine, all_summed=whole)
    for j in range(k):
        out['keep_%d' % j] = [fine[i] if i == j else whole[i] for i in range(k)]
    for m in (2, 3, 7):
        out['rebin%d' % m] = [list(range(0, n, m)) + [n] for n in shape]
    out['irregular'] = [irregular(n) for n in shape]
    out['ranges_keep_first'] = [inner_fine[i] if i == 0 else inner[i] for i in range(k)]
    out['ranges_keep_last'] = [inner_fine[i] if i == k - 1 else inner[i] for i in range(k)]
    out['box'] = inner
    combined = [list(b) for b in inner]
    combined[k - 1] = [1 + e for e in irregular(shape[k - 1] - 2)]
    if k > 1:
        combined[0] = list(range(1, shape[0] - 1, 2)) + [shape[0] - 1]
    out['combined'] = combined
    if few:
        out = OrderedDict((n, out[n]) for n in ('identity', 'keep_0', 'all_summed', 'combined'))
    return OrderedDict((n, [np.asarray(g, dtype=np.int32) for g in groups]) for n, groups in out.items())


def cell_map(shape, groups):
    """int64 [B]: the coarse flat index of every fine bin (C order), -1 where it is left out -- `CoarseBinning.bin_map()` over
    (fine_shape, groups); -> (map, cells)"""
    cell = np.zeros(shape, dtype=np.int64)
    out = np.zeros(shape, dtype=bool)
    cells = 1
    for axis, (n, bounds) in enumerate(zip(shape, groups)):
        g = np.searchsorted(bounds, np.arange(n), side='right') - 1
        left_out = (np.arange(n) < bounds[0]) | (np.arange(n) >= bounds[-1])
        at = [1] * len(shape)
        at[axis] = n
        cell = cell * (len(bounds) - 1) + np.where(left_out, 0, g).reshape(at)
        out = out | left_out.reshape(at)
        cells *= len(bounds) - 1
    return np.where(out, -1, cell).ravel(), cells


def reduce_wide(m, cells, fine):
    """fine [..., B] -> [..., C] in long double with np.add.at over the cell map: the specification"""
    inside = m >= 0
    fine = np.asarray(fine, dtype=np.longdouble)
    out = np.zeros(fine.shape[:-1] + (cells,), dtype=np.longdouble)
    flat, dst = fine.reshape(-1, fine.shape[-1]), out.reshape(-1, cells)
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


def five_points(model, seed):
    """three truths of box_points (the last on the upper edge of the box), one point outside the box and one with a negative rate
    scale -> (z [5, d], rs [5, S], status [5])"""
    z, rs = cases.box_points(model, np.random.default_rng(seed), 3)
    z, rs = np.concatenate([z, z[:2]]), np.concatenate([rs, rs[:2]])
    z[3, 1] = model['anchor_z'][1][-1] + 0.5
    rs[4, 0] = -0.25
    return z, rs, np.array([0, 0, 0, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL], dtype=np.int32)


def check_expected_coarse(name, model, shape, few):
    S, B = len(model['own']), fo.n_bins(model)
    assert B == int(np.prod(shape))
    z, rs, status = five_points(model, B + S)
    live = np.flatnonzero(status == 0)
    exact = {p: cases.exact_expectation(model, z[p], rs[p])[1] for p in live}             # [S, B] long double
    ctx = cases.upload(model)                                                            # no counts: none are needed
    worst = 0.0
    try:
        fine = ctx.expected_counts(z, rs)
        fine_parts = ctx.expected_counts(z, rs, per_source=True)
        for label, groups in binnings_of(shape, few).items():
            what = '%s, %s' % (name, label)
            m, cells = cell_map(shape, groups)
            assert ctx.set_coarse_binning(shape, groups) == cells, what
            total, st = ctx.expected_coarse(cells, z, rs)
            parts, st2 = ctx.expected_coarse(cells, z, rs, per_source=True)
            assert total.shape == (5, cells) and parts.shape == (5, S, cells), what
            assert np.array_equal(st, status) and np.array_equal(st2, status), what
            assert np.isnan(total[3:]).all() and np.isnan(parts[3:]).all(), what
            for p in live:
                want = reduce_wide(m, cells, exact[p])                                   # [S, C]
                worst = max(worst, within_bar(parts[p], want, what + ', per source, point %d' % p),
                            within_bar(total[p], want.sum(axis=0), what + ', total, point %d' % p),
                            within_bar(parts[p].sum(axis=0), total[p], what + ', sum of the sources, point %d' % p))
                if label == 'identity':                  # one fine bin per cell, the same chain: the same bits
                    assert np.array_equal(bits(total[p]), bits(fine[p])), what + ', against bi_sourcewise_expected_counts'
                    assert np.array_equal(bits(parts[p]), bits(fine_parts[p])), what + ', per source, against bi_sourcewise_expected_counts'
            # the same call again, and the second point alone: the same bits
            again, _ = ctx.expected_coarse(cells, z, rs)
            assert np.array_equal(bits(again), bits(total)), what
            again, _ = ctx.expected_coarse(cells, z, rs, per_source=True)
            assert np.array_equal(bits(again), bits(parts)), what
            alone, _ = ctx.expected_coarse(cells, z[1:2], rs[1:2])
            assert np.array_equal(bits(alone[0]), bits(total[1])), what
            alone, _ = ctx.expected_coarse(cells, z[1:2], rs[1:2], per_source=True)
            assert np.array_equal(bits(alone[0]), bits(parts[1])), what
        assert ctx.set_coarse_binning() == 0
    finally:
        ctx.close()
    print('%s: largest deviation %.3g of max(1, |want|)' % (name, worst))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(n) for n in s))
def test_expected_coarse_against_the_exact_oracle(shape):
    """Every binning of the shape at three truths, a point outside the box and one with a negative rate scale, total and per
    source: the oracle's cells, sum_s per source = total, nan in every cell and the screen's status for the dead points; a
    repeated call is bitwise equal, a point's row does not depend on the batch, and the identity binning has the bits of
    bi_sourcewise_expected_counts."""
    B = int(np.prod(shape))
    model = fo.random_model(np.random.default_rng(5100 + B), cases.N_ANCHOR, cases.OWN, B, zero_quarter=(1,))
    check_expected_coarse('x'.join(str(n) for n in shape), model, shape, few=False)


@pytest.mark.parametrize('name', cases.CLASS_CASES)
def test_expected_coarse_of_every_kernel_class(name):
    """The nine (source slots, own axes) classes at 13 x 79 bins: every instantiation of k_sourcewise_coarse, with and without
    per-source sums, at 128 lanes"""
    model, _, _ = cases.make_case(name)
    check_expected_coarse(name, model, CLASS_SHAPE, few=True)


@pytest.mark.parametrize('shape', [(63,), (33, 9), (9, 130), (5, 4, 7)], ids=lambda s: 'x'.join(str(n) for n in s))
def test_coarse_counts_of_uploaded_data_and_of_device_toys(shape):
    """Uploaded integer counts against np.add.at over the cell map, and toys drawn on the device against their downloaded rows
    reduced on the host: exact, for every binning, all datasets or a list with a repeated index; an index of T raises."""
    B = int(np.prod(shape))
    rng = np.random.default_rng(5200 + B)
    model = fo.random_model(rng, cases.N_ANCHOR, cases.OWN, B, zero_quarter=(1,))
    z, rs = cases.box_points(model, rng, 3)
    counts = rng.poisson(np.stack([fo.expectation(model, z[h], rs[h]) for h in range(3)])).astype(float)
    binnings = binnings_of(shape)
    ctx = cases.upload(model, counts)
    try:
        for stage in ('uploaded', 'toys'):
            if stage == 'toys':
                ctx.generate_toys_points(z, rs, cases.N_TOYS, cases.SEED)
            T = ctx.T
            assert T == (3 if stage == 'uploaded' else sum(cases.N_TOYS))
            down = np.stack([ctx.download_counts(t) for t in range(T)])
            assert np.array_equal(down, np.floor(down)) and down.sum() > 0
            for label, groups in binnings.items():
                what = '%s, %s, %s' % (shape, label, stage)
                m, cells = cell_map(shape, groups)
                assert ctx.set_coarse_binning(shape, groups) == cells
                want = np.stack([np.bincount(m[m >= 0], weights=row[m >= 0], minlength=cells) for row in down])
                assert np.array_equal(want, reduce_wide(m, cells, down).astype(float)), what
                got = ctx.coarse_counts(cells)
                assert got.shape == want.shape and np.array_equal(got, want), what
                assert np.array_equal(ctx.coarse_counts(cells, [2, 0, 2]), want[[2, 0, 2]]), what
                assert np.array_equal(bits(ctx.coarse_counts(cells)), bits(got)), what
            with pytest.raises(ValueError, match='outside'):
                ctx.coarse_counts(cells, [0, T])
    finally:
        ctx.close()


# ---- through the likelihood class -----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nuisance_lf():
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(5)
    lf.set_data(lf.base_model.simulate())
    return lf, names


def points_of(names, P, seed):
    rng = np.random.default_rng(seed)
    pts = {n: rng.uniform(-1.9, 1.9, P) for n in names}
    pts.update({'s%d_rate_multiplier' % s: rng.uniform(0.6, 1.5, P) for s in range(4)})
    return pts


def test_coarse_functions_on_the_likelihood(nuisance_lf):
    """blueice_amd.coarse on a SourceWiseBinnedLogLikelihood: expected_coarse_points is the context's call reshaped and the oracle's
    cells, expected_coarse its one-row form, coarse_counts the data's cells; gof_statistics(binning=) is coarse_statistics of the
    oracle's cells, and with the identity binning the statistics over the fine bins."""
    from blueice_amd import coarse, inference
    from test_factored_gpu import model_of
    lf, names = nuisance_lf
    model = model_of(lf)
    space = lf.base_model.config['analysis_space']
    first, last = str(space[0][0]), str(space[-1][0])
    P = 4
    pts = points_of(names, P, 11)
    zs = np.stack([pts[n] for n in names], axis=1)
    rs = np.stack([pts['s%d_rate_multiplier' % s] for s in range(4)], axis=1)
    exact = [cases.exact_expectation(model, zs[p], rs[p])[1] for p in range(P)]
    data = lf.ctx.download_counts(0)
    binnings = OrderedDict(identity=coarse.CoarseBinning(lf), keep_first=coarse.CoarseBinning(lf, keep=[first]),
                           rebin=coarse.CoarseBinning(lf, rebin={first: 2, last: 3}), all_summed=coarse.CoarseBinning(lf, keep=[]),
                           box=coarse.CoarseBinning(lf, keep=[last], ranges={first: (space[0][1][1], space[0][1][-2])}))
    worst = 0.0
    for label, b in binnings.items():
        m = b.bin_map().astype(np.int64)
        assert np.array_equal(m, cell_map(b.fine_shape, b.groups)[0])
        mu = coarse.expected_coarse_points(lf, b, pts)
        parts = coarse.expected_coarse_points(lf, b, pts, per_source=True)
        assert mu.shape == (P,) + b.shape and parts.shape == (P, 4) + b.shape, label
        direct, st = lf.ctx.expected_coarse(b.n_cells, zs, rs)
        assert np.array_equal(bits(mu.reshape(P, -1)), bits(direct)) and not st.any(), label
        want = np.stack([reduce_wide(m, b.n_cells, e) for e in exact])               # [P, S, C]
        worst = max(worst, within_bar(parts.reshape(P, 4, -1), want, label + ', per source'),
                    within_bar(mu.reshape(P, -1), want.sum(axis=1), label + ', total'))
        one = coarse.expected_coarse(lf, b, **{k: float(v[2]) for k, v in pts.items()})
        assert one.shape == b.shape and np.array_equal(bits(one), bits(mu[2])), label
        n = coarse.coarse_counts(lf, b)
        want_n = np.bincount(m[m >= 0], weights=data[m >= 0], minlength=b.n_cells)
        assert n.shape == (1,) + b.shape and np.array_equal(n.reshape(-1), want_n), label
        stats_ = inference.gof_statistics(lf, pts, binning=b)
        dev, pearson = coarse.coarse_statistics(want_n, want.sum(axis=1).astype(float))
        assert stats_['n_bins'] == b.n_cells and not stats_['status'].any(), label
        assert np.array_equal(stats_['n_events'], np.full(P, want_n.sum())), label
        worst = max(worst, within_bar(stats_['deviance'], dev, label + ', deviance'), within_bar(stats_['pearson'], pearson, label + ', pearson'))
        if label == 'identity':
            plain = inference.gof_statistics(lf, pts)
            assert plain['n_bins'] == b.n_cells
            worst = max(worst, within_bar(stats_['deviance'], plain['deviance'], 'identity against the fine bins, deviance'),
                        within_bar(stats_['pearson'], plain['pearson'], 'identity against the fine bins, pearson'))
    print('likelihood level: largest deviation %.3g of max(1, |want|)' % worst)
    with pytest.raises(NotImplementedError, match='source-wise'):
        coarse.expected_coarse_jacobian_points(lf, binnings['rebin'], pts)
    with pytest.raises(NotImplementedError, match='binning'):
        inference.gof_statistics(lf, pts, binning=object())


def test_goodness_of_fit_with_a_binning_end_to_end(nuisance_lf):
    from blueice_amd import coarse, inference
    lf, names = nuisance_lf
    space = lf.base_model.config['analysis_space']
    b = coarse.CoarseBinning(lf, rebin={str(space[0][0]): 2, str(space[-1][0]): 3})
    own = lf.ctx.download_counts(0)
    res = inference.goodness_of_fit(lf, n_toys=8, chunk=3, seed=2, binning=b)
    assert len(res.toys) == 8 and np.isfinite(res.toys).all() and np.isfinite(res.observed)
    assert 0 < res.p_value <= 1
    assert b.n_cells == 6 and res.ndof == b.n_cells - (4 + len(names))
    assert lf.ctx.T == 1
    np.testing.assert_array_equal(lf.ctx.download_counts(0), own)          # the likelihood's own data, bit for bit
    stats_ = inference.gof_statistics(lf, binning=b, **res.best)
    assert stats_['deviance'][0] == res.observed and stats_['n_events'][0] == own.sum()
    same = inference.goodness_of_fit(lf, n_toys=8, chunk=8, seed=2, binning=b)
    np.testing.assert_allclose(res.toys, same.toys, rtol=1e-9, atol=1e-9)


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------

def test_abi_refusals_and_the_life_of_the_binning():
    from blueice_amd._capi import ERR_INVALID, ERR_STATE, ptr
    from blueice_amd.exceptions import NotPreparedException
    shape = (9, 7)
    rng = np.random.default_rng(77)
    model = fo.random_model(rng, cases.N_ANCHOR, cases.OWN, 63)
    z, rs = cases.box_points(model, rng, 2)
    ctx = cases.upload(model, rng.poisson(5.0, 63).astype(float))
    dev = ctx._dev
    try:
        # no binning yet
        out = np.empty((2, 63))
        assert dev._lib.bi_sourcewise_expected_coarse(dev._h, 2, ptr(z), ptr(rs), 0, ptr(out), None) == ERR_STATE
        assert dev._lib.bi_sourcewise_coarse_counts(dev._h, 1, None, ptr(out)) == ERR_STATE
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse(63, z, rs)
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.coarse_counts(63)
        # binnings that do not fit
        with pytest.raises(ValueError, match='fine bins'):
            ctx.set_coarse_binning((9, 8), [[0, 9], [0, 8]])
        with pytest.raises(ValueError, match='ascending'):
            ctx.set_coarse_binning(shape, [[0, 4, 4, 9], [0, 7]])
        n_fine, n_groups, bounds = np.array(shape, dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([0, 0, 7], dtype=np.int32)
        cells = np.zeros(1, dtype=np.int64)
        assert dev._lib.bi_sourcewise_set_coarse_binning(dev._h, 2, ptr(n_fine), ptr(n_groups), ptr(bounds),
                                                         cells.ctypes.data_as(dev._lib.bi_sourcewise_set_coarse_binning.argtypes[5])) == ERR_INVALID
        with pytest.raises(NotPreparedException):       # (a refused binning leaves none behind)
            ctx.coarse_counts(63)
        # a binning, cleared by k = 0
        groups = [[0, 4, 9], [0, 7]]
        assert ctx.set_coarse_binning(shape, groups) == 2
        mu, _ = ctx.expected_coarse(2, z, rs)
        n = ctx.coarse_counts(2)
        assert np.isfinite(mu).all() and n.sum() == ctx.download_counts(0).sum()
        # the grid model's binning on the same context is a state of its own: without a grid model it is refused, with one
        # (20 bins, one source, no shape axis) either binning is set, used and cleared without the other noticing
        with pytest.raises(NotPreparedException):
            dev.set_coarse_binning(shape, groups)
        assert dev.get_param('coarse_cells') == 0
        grid_ps = rng.uniform(0.5, 1.5, (1, 20))
        dev.upload_model([], grid_ps, np.array([30.0]))
        assert dev.set_coarse_binning((4, 5), [[0, 1, 4], [0, 5]]) == 2 == dev.get_param('coarse_cells')
        grid_mu, _ = dev.expected_coarse(2, None, np.ones((1, 1)))
        assert np.allclose(grid_mu[0], 30.0 * np.array([grid_ps[0, :5].sum(), grid_ps[0, 5:].sum()]), rtol=1e-12, atol=0)
        again, _ = ctx.expected_coarse(2, z, rs)
        assert np.array_equal(bits(again), bits(mu))
        assert np.array_equal(ctx.coarse_counts(2), n)
        assert ctx.set_coarse_binning() == 0
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse(2, z, rs)
        assert dev.get_param('coarse_cells') == 2
        assert np.array_equal(bits(dev.expected_coarse(2, None, np.ones((1, 1)))[0]), bits(grid_mu))
        assert ctx.set_coarse_binning(shape, groups) == 2
        assert dev.set_coarse_binning() == 0 and dev.get_param('coarse_cells') == 0
        again, _ = ctx.expected_coarse(2, z, rs)
        assert np.array_equal(bits(again), bits(mu))
        # ... and released by a new model
        assert ctx.set_coarse_binning(shape, groups) == 2
        ctx.begin_model(model['anchor_z'], len(model['own']), 63, model['own'])
        for s in range(len(model['own'])):
            rows = np.asarray(model['ps'][s]).reshape(-1, 63)
            for k in range(len(rows)):
                ctx.set_anchor(s, k, rows[k], float(np.asarray(model['mus'][s]).reshape(-1)[k]))
        ctx.end_model()
        assert dev._lib.bi_sourcewise_expected_coarse(dev._h, 2, ptr(z), ptr(rs), 0, ptr(out), None) == ERR_STATE
        assert ctx.set_coarse_binning(shape, groups) == 2
        fresh, _ = ctx.expected_coarse(2, z, rs)
        assert np.array_equal(bits(fresh), bits(mu))
    finally:
        ctx.close()
