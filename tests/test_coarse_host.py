"""Host side of the coarse views, no device: `CoarseBinning` -- groups, shape, edges and `bin_map()`, the executable
specification that the device tests reduce with -- for every kind of coarsening, its refusals, and the statistics over coarse
cells (`coarse_statistics`) against the oracle's per-bin forms (tests/gof_oracle.py) on the reduced arrays."""
import numpy as np
import pytest

import gof_oracle
import model_zoo
from blueice_amd import coarse, inference
from blueice_amd.coarse import CoarseBinning

# 6 x 7 x 5 fine bins, none of the axes uniform
X = np.array([-3.0, -2.0, -1.5, 0.0, 0.5, 2.0, 4.0])
Y = np.array([0.0, 0.1, 0.3, 0.6, 1.0, 1.5, 2.1, 2.8])
W = np.array([10.0, 20.0, 40.0, 50.0, 70.0, 100.0])
SHAPE = (6, 7, 5)


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


@pytest.fixture(scope='module')
def lf(ns):
    """an unprepared binned likelihood: the analysis space is all a binning needs (there is no device here)"""
    return ns.BinnedLogLikelihood(ns.conf_for_test(analysis_space=[['x', X], ['y', Y], ['w', W]]))


def by_hand(groups):
    """bin_map from the per-axis boundaries with plain loops"""
    out = np.full(SHAPE, -1, dtype=np.int64)
    n_groups = [len(g) - 1 for g in groups]
    for i in range(SHAPE[0]):
        for j in range(SHAPE[1]):
            for k in range(SHAPE[2]):
                cell = 0
                for idx, g, m in zip((i, j, k), groups, n_groups):
                    inside = [q for q in range(m) if g[q] <= idx < g[q + 1]]
                    if not inside:
                        cell = -1
                        break
                    cell = cell * m + inside[0]
                out[i, j, k] = cell
    return out.ravel()


def check(b, dims, shape, groups, edges):
    assert list(b.dims) == dims and b.shape == shape and b.n_cells == int(np.prod(shape, dtype=int))
    assert [list(g) for g in b.groups] == groups and all(g.dtype == np.int32 for g in b.groups)
    assert len(b.edges) == len(edges)
    for got, want in zip(b.edges, edges):
        np.testing.assert_array_equal(got, want)
    m = b.bin_map()
    assert m.dtype == np.int32 and m.shape == (int(np.prod(SHAPE)),)
    np.testing.assert_array_equal(m, by_hand(groups))
    used = np.unique(m[m >= 0])
    np.testing.assert_array_equal(used, np.arange(b.n_cells))          # every cell holds a fine bin
    return m


def test_identity_and_keeping_or_summing_every_axis(lf):
    m = check(CoarseBinning(lf), ['x', 'y', 'w'], SHAPE, [list(range(7)), list(range(8)), list(range(6))], [X, Y, W])
    np.testing.assert_array_equal(m, np.arange(6 * 7 * 5))
    check(CoarseBinning(lf, keep=['x']), ['x'], (6,), [list(range(7)), [0, 7], [0, 5]], [X])
    m = check(CoarseBinning(lf, keep=['y']), ['y'], (7,), [[0, 6], list(range(8)), [0, 5]], [Y])
    np.testing.assert_array_equal(m.reshape(SHAPE)[3, :, 2], np.arange(7))
    check(CoarseBinning(lf, keep='w'), ['w'], (5,), [[0, 6], [0, 7], list(range(6))], [W])
    check(CoarseBinning(lf, keep=['w', 'x']), ['x', 'w'], (6, 5), [list(range(7)), [0, 7], list(range(6))], [X, W])   # analysis order
    b = CoarseBinning(lf, keep=[])
    m = check(b, [], (), [[0, 6], [0, 7], [0, 5]], [])
    assert b.n_cells == 1 and np.all(m == 0)


def test_rebin_by_an_integer_with_a_short_last_group(lf):
    check(CoarseBinning(lf, rebin=dict(x=2, y=2)), ['x', 'y', 'w'], (3, 4, 5),
          [[0, 2, 4, 6], [0, 2, 4, 6, 7], list(range(6))], [X[[0, 2, 4, 6]], Y[[0, 2, 4, 6, 7]], W])
    check(CoarseBinning(lf, keep=['y', 'w'], rebin=dict(y=3, w=3)), ['y', 'w'], (3, 2),
          [[0, 6], [0, 3, 6, 7], [0, 3, 5]], [Y[[0, 3, 6, 7]], W[[0, 3, 5]]])
    check(CoarseBinning(lf, keep=['w'], rebin=dict(w=7)), ['w'], (1,), [[0, 6], [0, 7], [0, 5]], [W[[0, 5]]])


def test_irregular_edges(lf):
    b = CoarseBinning(lf, keep=['x', 'y'], rebin=dict(x=[-3.0, -1.5, 0.0, 4.0], y=[0.1, 1.0 + 1e-11, 2.8]))
    check(b, ['x', 'y'], (3, 2), [[0, 2, 3, 6], [1, 4, 7], [0, 5]], [X[[0, 2, 3, 6]], Y[[1, 4, 7]]])
    assert np.count_nonzero(b.bin_map() < 0) == 6 * 1 * 5         # the first fine y bin lies below the first edge


def test_ranges_on_kept_and_on_summed_axes(lf):
    # a kept axis loses its first and last fine bins, a summed one too; rebinning starts at the range's first bin
    b = CoarseBinning(lf, keep=['x'], ranges=dict(x=(-2.0, 2.0), w=(20.0, 70.0)))
    m = check(b, ['x'], (4,), [[1, 2, 3, 4, 5], [0, 7], [1, 4]], [X[1:6]])
    full = m.reshape(SHAPE)
    assert np.all(full[0] == -1) and np.all(full[5] == -1) and np.all(full[:, :, 0] == -1) and np.all(full[:, :, 4] == -1)
    assert np.all(full[1:5, :, 1:4] >= 0)
    check(CoarseBinning(lf, keep=['y'], rebin=dict(y=2), ranges=dict(y=(0.1, 2.1))), ['y'], (3,),
          [[0, 6], [1, 3, 5, 6], [0, 5]], [Y[[1, 3, 5, 6]]])
    # a signal box is one cell
    box = CoarseBinning(lf, keep=[], ranges=dict(x=(-1.5, 0.5), y=(0.3, 1.5), w=(40.0, 100.0)))
    m = check(box, [], (), [[2, 4], [2, 5], [2, 5]], [])
    assert np.count_nonzero(m == 0) == 2 * 3 * 3 and np.count_nonzero(m == -1) == 210 - 18
    # everything at once
    check(CoarseBinning(lf, keep=['x', 'w'], rebin=dict(x=3, w=[20.0, 50.0, 70.0]), ranges=dict(x=(-2.0, 4.0), y=(0.1, 2.1), w=(20.0, 100.0))),
          ['x', 'w'], (2, 2), [[1, 4, 6], [1, 6], [1, 3, 4]], [X[[1, 4, 6]], W[[1, 3, 4]]])


def test_refusals(lf, ns):
    with pytest.raises(ValueError, match='not an edge'):
        CoarseBinning(lf, rebin=dict(x=[-3.0, -1.4, 4.0]))                # off the fine grid
    with pytest.raises(ValueError, match='not an edge'):
        CoarseBinning(lf, rebin=dict(y=[0.0, 0.1 + 2e-10, 2.8]))          # 1e-9 of the bin's width (0.1) is 1e-10
    CoarseBinning(lf, rebin=dict(y=[0.0, 0.1 + 5e-11, 2.8]))
    with pytest.raises(ValueError, match='not an edge'):
        CoarseBinning(lf, ranges=dict(w=(15.0, 70.0)))
    for bad in (dict(keep=['z']), dict(rebin=dict(z=2)), dict(ranges=dict(z=(0, 1))), dict(keep=['x', 'x'])):
        with pytest.raises(ValueError):
            CoarseBinning(lf, **bad)                                      # an unknown name
    for empty in ((0.5, 0.5), (2.0, -2.0)):
        with pytest.raises(ValueError, match='holds no bin'):
            CoarseBinning(lf, ranges=dict(x=empty))                       # an empty range
    with pytest.raises(ValueError):
        CoarseBinning(lf, rebin=dict(x=0))
    with pytest.raises(ValueError):
        CoarseBinning(lf, rebin=dict(x=[0.0, -2.0]))
    with pytest.raises(ValueError):
        CoarseBinning(lf, keep=['x'], rebin=dict(y=2))                    # a summed axis is not rebinned
    with pytest.raises(ValueError):
        CoarseBinning(lf, rebin=dict(x=[-3.0, 0.0, 4.0]), ranges=dict(x=(-2.0, 4.0)))
    # likelihoods without bins of their own, or whose expectation depends on the data: before any device is touched
    unbinned = ns.UnbinnedLogLikelihood(ns.conf_for_test(events_per_day=1))
    anc = ns.LogAncillaryLikelihood(lambda values: 0.0, ['nuisance'], config=dict(nuisance=0.5))
    total = ns.LogLikelihoodSum([unbinned, anc])
    data, _ = ns.make_data([dict(n_events=32, x=0.5)])
    bb = ns.BinnedLogLikelihood(ns.conf_for_test(default_source_class=ns.FixedSampleSource, events_per_day=32 / 5,
                                                 analysis_space=[['x', [0, 1]]], data=data),
                                likelihood_config=dict(model_zoo.BB_LC))
    for other in (bb, unbinned, total):
        with pytest.raises(NotImplementedError):
            CoarseBinning(other)
        assert getattr(other, 'ctx', None) is None
    # ... and the methods refuse them whatever the binning
    b = CoarseBinning(lf, keep=['x'])
    for other in (bb, unbinned, total):
        for call in (lambda o: o.expected_coarse(b), lambda o: o.expected_coarse_points(b, {}), lambda o: o.coarse_counts(b),
                     lambda o: o.gof_statistics(binning=b), lambda o: o.goodness_of_fit(binning=b)):
            with pytest.raises(NotImplementedError):
                call(other)
        assert getattr(other, 'ctx', None) is None


def test_names_are_public_and_methods():
    from blueice_amd.likelihood import BinnedLogLikelihood
    for name in ('expected_coarse', 'expected_coarse_points', 'coarse_counts'):
        assert name in inference.__all__ and getattr(BinnedLogLikelihood, name) is getattr(inference, name) is getattr(coarse, name)


def test_coarse_statistics_against_the_oracle_on_reduced_arrays(lf):
    """mu and n reduced with np.add.at over bin_map(), the statistics of the cells against gof_oracle.per_bin: cells with
    n > 0 and mu = 0 (+inf in both), with n = mu = 0 (nothing), and the nan / +inf of values that are no expectation or no count."""
    rng = np.random.default_rng(12)
    b = CoarseBinning(lf, keep=['x', 'w'], rebin=dict(x=2, w=3), ranges=dict(y=(0.1, 2.1)))
    m = b.bin_map()
    inside = m >= 0
    mu_fine = rng.uniform(0.0, 3.0, size=(4, m.size))
    n_fine = rng.poisson(mu_fine[0]).astype(float)
    mu_fine[:, m == 1] = 0.0                       # a cell without expectation ...
    n_fine[m == 1] = 0.0                           # ... and without events
    mu, n = np.zeros((4, b.n_cells)), np.zeros(b.n_cells)
    for p in range(4):
        np.add.at(mu[p], m[inside], mu_fine[p, inside])
    np.add.at(n, m[inside], n_fine[inside])
    assert mu[0, 1] == 0.0 and n[1] == 0.0 and np.all(n[[0, 2, 3, 4, 5]] > 0)
    dev, pearson = coarse.coarse_statistics(n, mu)
    assert dev.shape == pearson.shape == (4,)
    for p in range(4):
        half, pe = gof_oracle.per_bin(n, mu[p])
        assert np.isfinite(half.sum()) and abs(dev[p] - 2 * half.sum()) <= 1e-13 * abs(2 * half.sum())
        assert abs(pearson[p] - pe.sum()) <= 1e-13 * pe.sum()
    assert half[1] == 0.0 and pe[1] == 0.0
    # an event in a FINE bin without expectation does not force +inf while its cell expects something
    n2 = n.copy()
    n2[1] = 1.0                                    # ... an event in the cell that expects nothing does
    dev, pearson = coarse.coarse_statistics(n2, mu)
    assert np.all(dev == np.inf) and np.all(pearson == np.inf)
    half, pe = gof_oracle.per_bin(n2, mu[0])
    assert half.sum() == np.inf and pe.sum() == np.inf
    # every point against every dataset by broadcasting
    dev, pearson = coarse.coarse_statistics(np.stack([n, n2])[None, :, :], mu[:, None, :])
    assert dev.shape == (4, 2) and np.all(np.isfinite(dev[:, 0])) and np.all(dev[:, 1] == np.inf)
    # what is no expectation or no count
    one = coarse.coarse_statistics([2.0, 0.0], [-1.0, 1.0])
    assert np.isnan(one[0]) and np.isnan(one[1])
    one = coarse.coarse_statistics([2.0, np.nan], [1.0, 1.0])
    assert np.isnan(one[0]) and np.isnan(one[1])
    one = coarse.coarse_statistics([2.5, 0.0], [1.0, 1.0])
    assert one == (np.inf, np.inf)
    assert coarse.coarse_statistics([0.0, 0.0], [0.0, 8.0]) == (16.0, 8.0)
