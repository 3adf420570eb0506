"""Coarse views of a source-wise model without a GPU: the Python layers (blueice_amd.coarse, gof_statistics(binning=) of
blueice_amd.inference) over a recording context that stands where SourceWiseContext would, the refusals that stay, and the header
/ binding of the three C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from test_sourcewise_toys_host import RecordingToyContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('bi_sourcewise_set_coarse_binning', 'bi_sourcewise_expected_coarse', 'bi_sourcewise_coarse_counts')


class RecordingCoarseContext(RecordingToyContext):
    """... with the three coarse calls: cell c of every point expects 1 + c (source s: (1 + c) (1 + s) / 10 of it), dataset t
    holds t + c events in it"""

    def set_coarse_binning(self, fine_shape=None, groups=None):
        if fine_shape is None:
            self.calls.append(('set_coarse_binning', None, None))
            self.cells = 0
            return 0
        groups = [np.asarray(g) for g in groups]
        self.calls.append(('set_coarse_binning', tuple(fine_shape), groups))
        self.cells = int(np.prod([len(g) - 1 for g in groups]))
        return self.cells

    def expected_coarse(self, n_cells, z, rate_scale=None, per_source=False):
        P = len(z)
        assert n_cells == self.cells
        self.calls.append(('expected_coarse', n_cells, np.array(z), np.array(rate_scale), bool(per_source)))
        mu = np.broadcast_to(1.0 + np.arange(n_cells), (P, n_cells)).copy()
        if per_source:
            mu = mu[:, None, :] * (1.0 + np.arange(self.S))[None, :, None] / 10.0
        return mu, np.zeros(P, dtype=np.int32)

    def coarse_counts(self, n_cells, datasets=None):
        assert n_cells == self.cells
        datasets = np.arange(self.T) if datasets is None else np.atleast_1d(datasets)
        self.calls.append(('coarse_counts', n_cells, np.array(datasets)))
        return np.asarray(datasets, dtype=float)[:, None] + np.arange(n_cells)[None, :]


def make_lf(monkeypatch, prepare=True):
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingCoarseContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    if prepare:
        lf.prepare()
    return lf, names, conf


@pytest.fixture
def recorded(monkeypatch):
    return make_lf(monkeypatch)


def test_binning_and_attach_reach_the_context(recorded):
    from blueice_amd.coarse import CoarseBinning
    lf, names, conf = recorded
    (first, e0), (last, e1) = [(str(n), np.asarray(e, dtype=float)) for n, e in conf['analysis_space']]
    b = CoarseBinning(lf, keep=[first], rebin={first: 2}, ranges={last: (e1[1], e1[4])})
    assert b.fine_shape == (6, 5) == tuple(lf.bin_shape) and b.shape == (3,) and b.n_cells == 3
    assert [list(g) for g in b.groups] == [[0, 2, 4, 6], [1, 4]]
    m = b.bin_map().reshape(6, 5)
    assert (m[:, 0] == -1).all() and (m[:, 4] == -1).all() and list(m[:, 2]) == [0, 0, 1, 1, 2, 2]
    n_before = len(lf.ctx.calls)
    assert b.attach(lf, 'test') is lf
    kind, shape, groups = lf.ctx.calls[-1]
    assert len(lf.ctx.calls) == n_before + 1 and kind == 'set_coarse_binning' and shape == (6, 5)
    assert [list(g) for g in groups] == [[0, 2, 4, 6], [1, 4]]
    # every other kind of binning is taken as for the grid model
    assert CoarseBinning(lf).shape == (6, 5) and CoarseBinning(lf, keep=[]).n_cells == 1
    assert CoarseBinning(lf, keep=[last], rebin={last: e1[[0, 1, 5]]}).shape == (2,)
    with pytest.raises(ValueError, match='not an edge'):
        CoarseBinning(lf, ranges={first: (e0[0] + 0.3 * (e0[1] - e0[0]), e0[3])})


def test_expected_coarse_and_coarse_counts_reach_the_context(recorded):
    from blueice_amd import coarse, inference
    lf, names, conf = recorded
    first = str(conf['analysis_space'][0][0])
    b = coarse.CoarseBinning(lf, rebin={first: 3})
    assert b.shape == (2, 5)
    pts = {names[0]: np.array([-0.5, 0.0, 0.5]), 's1_rate_multiplier': 1.5}
    z_want, scale_want, _ = lf._batch_terms(pts, None)

    mu = coarse.expected_coarse_points(lf, b, pts)
    kind, cells, z, scale, per_source = lf.ctx.calls[-1]
    assert (kind, cells, per_source) == ('expected_coarse', 10, False) and lf.ctx.calls[-2][0] == 'set_coarse_binning'
    np.testing.assert_array_equal(z, z_want)                     # the host terms of expected_counts_points
    np.testing.assert_array_equal(scale, scale_want)
    assert z.shape == (3, len(names)) and scale.shape == (3, 4) and list(z[:, 0]) == [-0.5, 0.0, 0.5]
    assert mu.shape == (3, 2, 5)
    np.testing.assert_array_equal(mu[1], 1.0 + np.arange(10).reshape(2, 5))
    parts = coarse.expected_coarse_points(lf, b, pts, per_source=True)
    assert lf.ctx.calls[-1][4] is True and parts.shape == (3, 4, 2, 5)
    np.testing.assert_array_equal(parts[2, 3], (1.0 + np.arange(10).reshape(2, 5)) * 4 / 10.0)
    # the fine-bin route gets the same host terms
    inference.expected_counts_points(lf, pts)
    assert lf.ctx.calls[-1] == ('expected_counts', 3, False)

    # one point: the one-row `_points` form
    one = coarse.expected_coarse(lf, b, per_source=True, **{names[0]: 0.5, 's1_rate_multiplier': 1.5})
    kind, cells, z, scale, per_source = lf.ctx.calls[-1]
    assert kind == 'expected_coarse' and z.shape == (1, len(names)) and per_source and one.shape == (4, 2, 5)
    np.testing.assert_array_equal(z[0], z_want[2])
    np.testing.assert_array_equal(scale[0], scale_want[2])
    assert coarse.expected_coarse(lf, b).shape == (2, 5)

    # counts need data
    from blueice_amd.exceptions import NotPreparedException
    with pytest.raises(NotPreparedException, match='set_data'):
        coarse.coarse_counts(lf, b)
    lf.set_binned_data(np.ones((3, 6, 5)))
    n = coarse.coarse_counts(lf, b)
    assert lf.ctx.calls[-1][:2] == ('coarse_counts', 10) and n.shape == (3, 2, 5)
    n = coarse.coarse_counts(lf, b, datasets=[2, 0])
    assert list(lf.ctx.calls[-1][2]) == [2, 0] and n.shape == (2, 2, 5) and n[0, 0, 0] == 2.0


def test_gof_statistics_over_the_cells(recorded):
    from blueice_amd import coarse, inference
    lf, names, conf = recorded
    last = str(conf['analysis_space'][-1][0])
    b = coarse.CoarseBinning(lf, keep=[last])
    lf.set_binned_data(np.ones((3, 6, 5)))
    del lf.ctx.calls[:]
    out = inference.gof_statistics(lf, {names[0]: np.array([0.1, 0.2, 0.3])}, datasets=np.array([0, 2, 1]), binning=b)
    kinds = [c[0] for c in lf.ctx.calls]
    assert kinds == ['set_coarse_binning', 'expected_coarse', 'coarse_counts'] and 'eval_gof' not in kinds
    assert list(lf.ctx.calls[-1][2]) == [0, 1, 2]                          # the datasets the points name, each once
    assert out['n_bins'] == b.n_cells == 5
    n = np.array([0.0, 2.0, 1.0])[:, None] + np.arange(5)[None, :]
    mu = np.broadcast_to(1.0 + np.arange(5), (3, 5))
    deviance, pearson = coarse.coarse_statistics(n, mu)
    np.testing.assert_array_equal(out['deviance'], deviance)
    np.testing.assert_array_equal(out['pearson'], pearson)
    np.testing.assert_array_equal(out['n_events'], n.sum(axis=1))
    assert not out['status'].any()
    # a dataset that does not exist: the status bit, +inf
    out = inference.gof_statistics(lf, {names[0]: np.array([0.1, 0.2])}, datasets=np.array([0, 3]), binning=b)
    assert list(out['status']) == [0, 16] and out['deviance'][1] == np.inf and np.isfinite(out['deviance'][0])


def test_goodness_of_fit_with_a_binning(recorded, monkeypatch):
    from blueice_amd import coarse, inference
    lf, names, conf = recorded
    b = coarse.CoarseBinning(lf, rebin={str(conf['analysis_space'][0][0]): 2})
    best = dict([('s%d_rate_multiplier' % s, 1.0) for s in range(4)] + [(n, 0.0) for n in names])

    def fake_fit(lf_, datasets=None, return_info=False, **kw):
        n = 1 if datasets is None else len(datasets)
        fit = {k: np.full(n, v) for k, v in best.items()}
        info = dict(failed=np.zeros(n, dtype=bool))
        return (fit, np.zeros(n), info) if return_info else (fit, np.zeros(n))

    monkeypatch.setattr(inference, 'bestfit_batched', fake_fit)
    lf.set_binned_data(np.ones((6, 5)))
    del lf.ctx.calls[:]
    res = inference.goodness_of_fit(lf, n_toys=3, chunk=2, seed=4, binning=b)
    assert res.ndof == b.n_cells - len(best) == 15 - len(best) and len(res.toys) == 3 and 0 < res.p_value <= 1
    kinds = [c[0] for c in lf.ctx.calls]
    assert 'eval_gof' not in kinds and kinds.count('expected_coarse') == 3 and kinds.count('generate_toys_points') == 2
    want, _ = coarse.coarse_statistics(np.arange(15.0), 1.0 + np.arange(15))
    assert res.observed == want
    assert lf.ctx.calls[-1] == ('set_counts', 1)                          # the likelihood's own data are handed back


def test_refusals_that_stay(recorded, monkeypatch):
    from blueice_amd import coarse, inference
    from blueice_amd.exceptions import NotPreparedException
    lf, names, conf = recorded
    b = coarse.CoarseBinning(lf, keep=[])
    lf.set_binned_data(np.ones((6, 5)))
    n_before = len(lf.ctx.calls)
    # the derivatives of coarse views
    for call in (lambda: coarse.expected_coarse_jacobian_points(lf, b, {names[0]: np.array([0.1])}),
                 lambda: coarse.expected_coarse_jacobian(lf, b, **{names[0]: 0.1}),
                 lambda: coarse.expected_coarse_band(lf, b, [names[0]], np.eye(1), **{names[0]: 0.1}),
                 lambda: coarse.coarse_information(lf, b, **{names[0]: 0.1})):
        with pytest.raises(NotImplementedError, match='source-wise'):
            call()
    # a binning that is no CoarseBinning
    with pytest.raises(NotImplementedError, match='binning'):
        inference.gof_statistics(lf, {names[0]: 0.1}, binning=object())
    with pytest.raises(NotImplementedError, match='binning'):
        inference.goodness_of_fit(lf, n_toys=2, binning=object())
    with pytest.raises(TypeError, match='CoarseBinning'):
        coarse.expected_coarse_points(lf, object(), {names[0]: np.array([0.1])})
    # the gates of everything else keep refusing the class
    for gate in (coarse._binned_for_gof, inference._binned_for_gof):
        with pytest.raises(NotImplementedError, match='BinnedLogLikelihood'):
            gate(lf, 'test')
    # the bound names refuse and name the spellings that work
    spellings = {'expected_coarse': 'blueice_amd.coarse.expected_coarse(lf, binning',
                 'expected_coarse_points': 'blueice_amd.coarse.expected_coarse_points(lf, binning, points)',
                 'coarse_counts': 'blueice_amd.coarse.coarse_counts(lf, binning'}
    for name, spelling in spellings.items():
        assert name in type(lf)._REFUSED
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            getattr(lf, name)(b)
        assert spelling in str(e.value), (name, str(e.value))
    for name in ('expected_coarse_jacobian', 'expected_coarse_jacobian_points', 'expected_coarse_band', 'coarse_information'):
        assert name in type(lf)._REFUSED
        with pytest.raises(NotImplementedError, match='source-wise'):
            getattr(lf, name)(b)
    assert len(lf.ctx.calls) == n_before                                  # nothing reached the context

    # an unprepared model
    raw, _, _ = make_lf(monkeypatch, prepare=False)
    assert coarse.CoarseBinning(raw, keep=[]).n_cells == 1                  # (the binning needs the analysis space only)
    with pytest.raises(NotPreparedException, match='prepare'):
        coarse.expected_coarse_points(raw, b, {names[0]: np.array([0.1])})
    with pytest.raises(NotPreparedException, match='prepare'):
        coarse.coarse_counts(raw, b)
    with pytest.raises(NotPreparedException, match='prepare'):
        inference.gof_statistics(raw, {names[0]: 0.1}, binning=b)

    # a binning made for another analysis space
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    conf2, names2, _ = many_nuisances_config(n_bins=(5, 6))
    other = sw.SourceWiseBinnedLogLikelihood(conf2, likelihood_config=dict(device_histograms=False))
    for n in names2:
        other.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    other.prepare()
    with pytest.raises(ValueError, match='another analysis space'):
        coarse.expected_coarse_points(other, b, {names2[0]: np.array([0.1])})
    assert not [c for c in other.ctx.calls if c[0] == 'set_coarse_binning']


def test_header_and_binding_of_the_three_symbols():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    build.build()
    lib = _capi.load()
    for s in SYMBOLS:
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text)
        assert proto, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.group(1).split(',') if a.strip()]), s
    assert _capi.SIGNATURES['bi_sourcewise_set_coarse_binning'] == _capi.SIGNATURES['bi_set_coarse_binning']
    assert _capi.SIGNATURES['bi_sourcewise_expected_coarse'] == _capi.SIGNATURES['bi_expected_coarse']
    assert _capi.SIGNATURES['bi_sourcewise_coarse_counts'] == _capi.SIGNATURES['bi_coarse_counts']
    assert 'tu_sourcewise_coarse' in build.UNITS
    one = np.ones(64)
    p = _capi.ptr
    assert lib.bi_sourcewise_set_coarse_binning(None, 0, None, None, None, None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_expected_coarse(None, 1, p(one), None, 0, p(one.copy()), None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_coarse_counts(None, 1, None, p(one.copy())) == _capi.ERR_INVALID
