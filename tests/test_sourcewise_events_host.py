"""Unbinned source-wise likelihoods without a GPU: the NumPy specification (sourcewise_events_oracle) against the exact oracle of
the expanded grid and against the reference's recorded values, the Python class over a recording context, and the header /
binding of the new C-ABI symbols."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import factored_oracle as fo
import model_zoo
import sourcewise_events_oracle as eo
from derivative_oracle import C_POISSON, check_entries, derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'api_source_wise.npz')

N_ANCHOR, OWN = (3, 2, 4), ((0,), (1, 2), ())


def event_model(rng, n_anchor, own, N, zero_quarter=(1,)):
    """pdf values at N events: factored_oracle.random_model's rows scaled to order one (a source of `zero_quarter` is exactly 0
    at a quarter of the events, the others comfortably positive)"""
    model = fo.random_model(rng, n_anchor, own, max(N, 1), zero_quarter=zero_quarter)
    model['ps'] = [np.nan_to_num(p, nan=0.0) for p in model['ps']]      # (N = 1: the zeroed source's only value, 0 / 0)
    model['ps'] = [p[..., :N] * max(N, 1) for p in model['ps']]
    return model


def points(model, rng):
    g = model['anchor_z']
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    S = len(model['own'])
    pts = [(lo + (hi - lo) * rng.uniform(0.05, 0.95, len(g)), rng.uniform(0.5, 1.6, S)) for _ in range(2)]
    on = lo + (hi - lo) * rng.uniform(0.05, 0.95, len(g))
    on[0] = g[0][1]                                         # an interior anchor
    pts.append((on, rng.uniform(0.5, 1.6, S)))
    pts.append((hi.copy(), rng.uniform(0.5, 1.6, S)))       # the closed last cell of every axis
    return pts


@pytest.mark.parametrize('N', [1, 63, 1001])
def test_specification_against_the_oracle_of_the_expansion(N):
    rng = np.random.default_rng(300 + N)
    worst = 0.0
    for k in range(3):
        model = event_model(rng, N_ANCHOR, OWN, N, zero_quarter=(1,) if k else ())
        if k == 2 and N > 1:
            for p in model['ps']:
                p[..., 5] = 0.0                             # an event every source gives 0: the clamp
            model['ps'][1][1, 2, 7] = np.nan                # one corner of one source at one event
        full = fo.expand(model)
        for outlier in (1e-12, 0.0):
            for z, rs in points(model, rng):
                got = eo.events_derivatives(model, z, rs, outlier=outlier)
                want = derivatives(full, z, rs, unbinned=True, outlier=outlier, hessian=False)
                if outlier == 0.0 and k == 2 and N > 1:
                    assert got['ll'] == -np.inf and np.isnan(got['grad']).all()
                    continue
                worst = max(worst, check_entries(got['ll'], want['ll'], want['ll_cond'], what='ll N=%d' % N))
                worst = max(worst, check_entries(got['grad'], want['grad'], want['grad_cond'], what='grad N=%d' % N))
                if outlier:
                    assert got['n_clamped'] == (1 if k == 2 and N > 1 else 0)
                    plain = eo.plain_ll(model, z, rs, outlier)
                    assert abs(plain - want['ll']) <= 1e-10 * max(1.0, abs(want['ll']))
    print('N = %d: worst |err| / (2^-52 cond) = %.3g of C = %d' % (N, worst, C_POISSON))


def test_no_events_is_minus_the_rates():
    rng = np.random.default_rng(5)
    model = event_model(rng, N_ANCHOR, OWN, 0)
    z, rs = points(model, rng)[0]
    got = eo.events_derivatives(model, z, rs)
    total, _ = eo.rate_terms(model, z, rs)
    assert got['ll'] == -float(total.v) and np.isfinite(got['grad']).all()


def test_specification_reproduces_the_reference_values(monkeypatch):
    """The per-source tensors the reference's interpolators hold give its recorded log likelihoods: the seven calls inside the box"""
    f = np.load(GOLDEN)
    model = eo.golden_model(f)
    assert model['own'] == [(0,), (1,), ()] and [len(g) for g in model['anchor_z']] == [3, 3]
    _, calls = golden_calls(monkeypatch)
    assert len(calls) == 9
    for j, kw in enumerate(calls[:7]):
        z, rs = eo.golden_point(kw)
        want = f['call_ll'][j]
        for got in (eo.events_derivatives(model, z, rs)['ll'], eo.plain_ll(model, z, rs)):
            assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (j, got, want)
    assert np.all(f['call_ll'][7:] == -np.inf)


# ---- the Python class over a recording context ----------------------------------------------------------------------------

class RecordingContext:
    """Stands where SourceWiseContext would: records the model's rows and the event uploads; cannot evaluate."""

    def __init__(self, device=None):
        self.T = 0
        self.rows = {}
        self.begun = 0
        self.log = []

    def begin_model(self, anchor_z, S, B, own_axes):
        self.anchor_z, self.S, self.B, self.own_axes = [np.asarray(g, float) for g in anchor_z], S, B, [tuple(o) for o in own_axes]
        self.rows = {}
        self.begun += 1

    def set_anchor(self, s, local_index, ps_row, mu):
        assert (s, local_index) not in self.rows
        self.rows[(s, local_index)] = (np.array(ps_row, float).reshape(self.B), float(mu))

    def end_model(self):
        self.ended = True

    def score_events(self, method, grid, coords, outlier_likelihood=0.0):
        self.log.append(('score', method, [np.asarray(g, float) for g in grid], coords, outlier_likelihood))
        self.T = len(coords)

    def set_event_rows(self, n_events, rows, outlier_likelihood=0.0):
        values = {key: np.array(rows(*key), float) for key in sorted(self.rows)}
        self.log.append(('rows', list(n_events), values, outlier_likelihood))
        self.T = len(n_events)

    def event_set_counts(self):
        return np.array(self.log[-1][1] if self.log[-1][0] == 'rows' else [len(cs[0]) for cs in self.log[-1][3]])

    def close(self):
        pass


def golden_calls(monkeypatch):
    """model_zoo.api_source_wise's configuration, data and calls with SourceWiseUnbinnedLogLikelihood in the place of
    UnbinnedLogLikelihood, over a recording context -> (lf, calls)"""
    import blueice_amd.source_wise as sw
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingContext)
    ns = model_zoo.namespace_of('blueice_amd')
    return model_zoo.api_source_wise(SimpleNamespace(**dict(vars(ns), UnbinnedLogLikelihood=SourceWiseUnbinnedLogLikelihood)))


def test_prepare_builds_exactly_the_projected_anchors_and_scores_on_the_host(monkeypatch):
    """model_zoo.api_source_wise's configuration: the base model + 3 anchors of mu + 3 of sigma = 7 models, a one-bin model on
    the device (geometry and rates), and -- analytic pdfs -- one pdf call per own anchor row, the reference's per-source tensors"""
    import blueice_amd.model as model_module
    built = []
    original = model_module.Model.__init__

    def counting(self, config, **kw):
        built.append((config.get('mu'), config.get('sigma')))
        original(self, config, **kw)

    monkeypatch.setattr(model_module.Model, '__init__', counting)
    lf, calls = golden_calls(monkeypatch)
    assert built == [(0, 1), (-1., 1), (0., 1), (1., 1), (0, 0.8), (0, 1.), (0, 1.5)]
    rec = lf.ctx
    assert isinstance(rec, RecordingContext) and rec.begun == 1 and rec.ended
    assert rec.S == 3 and rec.B == 1 and rec.own_axes == [(0,), (1,), ()] and len(rec.rows) == 7
    assert lf.scoring_route == 'host' and lf.last_scoring_route == 'host' and lf.outlier_likelihood == 1e-12
    f = np.load(GOLDEN)
    kind, n_events, values, outlier = rec.log[-1]
    assert kind == 'rows' and n_events == [63] and outlier == 1e-12 and len(rec.log) == 1
    for i in range(3):
        want_ps = f['sw_%d_ps' % i].reshape(-1, 63)
        want_mu = f['sw_%d_mus' % i].reshape(-1)
        for local in range(len(want_ps)):
            np.testing.assert_array_equal(values[(i, local)], want_ps[local])
            assert rec.rows[(i, local)][1] == want_mu[local] and rec.rows[(i, local)][0].tolist() == [1.0]
    assert lf.n_events_per_dataset.tolist() == [63]
    assert not lf.supports_hessian and lf.supports_gradient and lf.hessian_method == 'gradient-differences'


def histogram_likelihood(monkeypatch, method, **likelihood_config):
    import blueice_amd.source_wise as sw
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5), source_class=NuisanceHistogramSource)
    conf['pdf_interpolation_method'] = method
    lf = SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False, **likelihood_config))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    lf.prepare()
    return lf, conf


@pytest.mark.parametrize('method', ['piecewise', 'linear'])
def test_histogram_sources_are_scored_on_the_device(monkeypatch, method):
    """Eight nuisances of five anchors, four histogram sources of two own parameters: 4 x 25 density histograms are the model's
    rows, and set_data / set_datasets send coordinates only ('linear': clipped to the outer bin centres)"""
    lf, conf = histogram_likelihood(monkeypatch, method)
    rec = lf.ctx
    assert lf.scoring_route == 'device' and rec.B == 30 and len(rec.rows) == 100 and len(rec.anchor_z) == 8
    source = lf.anchor_sources['s1'][(-2., 1.)]
    local = list(lf.anchor_sources['s1']).index((-2., 1.))
    np.testing.assert_array_equal(rec.rows[(1, local)][0], source._pdf_histogram.histogram.ravel())
    assert rec.rows[(1, local)][1] == source.expected_events
    np.random.seed(3)
    sets = [lf.base_model.simulate() for _ in range(3)]
    sets[1] = sets[1][:0]
    sets[0]['x'][0], sets[0]['y'][1] = -0.5, 7.0            # outside the analysis space
    lf.set_datasets(sets)
    kind, got_method, grid, coords, outlier = rec.log[-1]
    assert kind == 'score' and got_method == method and outlier == 1e-12 and lf.last_scoring_route == 'device'
    edges = [np.asarray(e, float) for _, e in conf['analysis_space']]
    want_grid = edges if method == 'piecewise' else [0.5 * (e[:-1] + e[1:]) for e in edges]
    for g, w in zip(grid, want_grid):
        np.testing.assert_array_equal(g, w)
    assert [len(cs[0]) for cs in coords] == [len(d) for d in sets] and lf.n_events_per_dataset.tolist() == [len(d) for d in sets]
    if method == 'linear':
        assert coords[0][0][0] == want_grid[0][0] and coords[0][1][1] == want_grid[1][-1]
    else:
        assert coords[0][0][0] == -0.5 and coords[0][1][1] == 7.0
    # a coordinate that is not finite, or device_scoring = False: the host scores, through the same sources
    if method == 'piecewise':                               # ('linear': scipy's interpolator refuses such a coordinate, as in the reference)
        sets[2]['x'][0] = np.nan
        lf.set_data(sets[2])
        assert rec.log[-1][0] == 'rows' and lf.last_scoring_route == 'host' and rec.log[-1][1] == [len(sets[2])]
    lf2, _ = histogram_likelihood(monkeypatch, method, device_scoring=False)
    assert lf2.scoring_route == 'host' and lf2.ctx.B == 1


def test_refusals_name_the_scope(monkeypatch):
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    from blueice_amd.exceptions import NotPreparedException
    lf, conf = histogram_likelihood(monkeypatch, 'linear')
    np.random.seed(4)
    d = lf.base_model.simulate()
    lf.set_data(d)
    scope = 'unbinned source-wise model'
    for name in ('simulate_toy', 'simulate_toys', 'simulate_toys_points', 'eval_toys', 'sample_posterior', 'bestfit_emcee', 'grid_scan',
                 'set_binned_data', 'fisher_information_points', 'expected_errors', 'gof_statistics', 'goodness_of_fit',
                 'expected_counts_points', 'expected_coarse', 'asimov', 'toy_test_statistics', 'neyman_thresholds'):
        with pytest.raises(NotImplementedError, match=scope):
            getattr(lf, name)()
    with pytest.raises(NotImplementedError, match=scope):
        lf.data_events_per_bin
    for kw in (dict(compute_pdf=True), dict(full_output=True)):
        with pytest.raises(NotImplementedError, match='SourceWiseUnbinnedLogLikelihood'):
            lf(**kw)
    with pytest.raises(NotImplementedError, match='Beeston-Barlow'):
        SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(model_statistical_uncertainty_handling='bb_single'))
    unprepared = SourceWiseUnbinnedLogLikelihood(conf)
    unprepared.add_shape_parameter('np0', (-1., 0., 1.))
    with pytest.raises(NotPreparedException):
        unprepared.set_data(d)
    with pytest.raises(ValueError, match='analysis dimensions'):
        lf.set_datasets([d, np.zeros(3, dtype=[('x', float)])])
    # the limits of a source-wise model
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf4, names4, _ = many_nuisances_config(n_bins=(6, 5), own_per_source=2, source_class=NuisanceHistogramSource)
    conf4['sources'][0]['extra_dont_hash_settings'] = names4[4:]           # source 0 responds to four settings
    big = SourceWiseUnbinnedLogLikelihood(conf4, likelihood_config=dict(device_histograms=False))
    for n in names4:
        big.add_shape_parameter(n, (-1., 0., 1.))
    with pytest.raises(ValueError, match='at most 3 per source.*UnbinnedLogLikelihood'):
        big.prepare()
    neg = dict(conf)
    neg['sources'] = [dict(s, allow_negative=True) if i == 0 else s for i, s in enumerate(conf['sources'])]
    lf_neg = SourceWiseUnbinnedLogLikelihood(neg, likelihood_config=dict(device_histograms=False))
    assert lf_neg.source_allowed_negative == [True, False, False, False]
    lf_neg.add_shape_parameter('np0', (-1., 0., 1.))
    with pytest.raises(NotImplementedError, match='allow_negative'):
        lf_neg.prepare()


def test_the_full_grid_class_keeps_its_path(monkeypatch):
    """UnbinnedLogLikelihood(source_wise_interpolation=True) still uploads the Cartesian expansion to a DeviceContext"""
    import blueice_amd.likelihood as lk
    from test_host_layer import RecordingContext as GridRecorder
    monkeypatch.setattr(lk, 'DeviceContext', GridRecorder)
    lf, _ = model_zoo.api_source_wise(model_zoo.namespace_of('blueice_amd'))
    assert isinstance(lf.ctx, GridRecorder) and len(lf.ctx.anchors) == 9 and lf.ctx.B == 63


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ['bi_sourcewise_events_begin', 'bi_sourcewise_events_set_row', 'bi_sourcewise_events_end', 'bi_sourcewise_score_events',
               'bi_sourcewise_drop_events', 'bi_sourcewise_event_set_counts', 'bi_sourcewise_download_event_set']


def test_header_binding_and_build_list_agree_on_the_new_symbols():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(bi_[a-z_0-9]+)\s*\(', text))
    build.build()
    lib = _capi.load()
    for s in NEW_SYMBOLS:
        assert s in declared, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text).group(1)
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.split(',') if a.strip()]), s
    assert 'tu_sourcewise_events' in build.UNITS
    for name in ('tu_sourcewise_events.hip', 'bi_k_sourcewise_events.h', 'bi_sourcewise_events.h'):
        assert os.path.exists(os.path.join(build.CSRC, name))
    import ctypes as C
    n = lib.bi_list_params(None, 0)
    buf = C.create_string_buffer(n)
    lib.bi_list_params(buf, n)
    params = dict(line.split() for line in buf.value.decode().splitlines())
    assert params['sourcewise_events_ready'] == 'r' and params['sourcewise_events_bytes'] == 'r' and params['sourcewise_event_sets'] == 'r'


def test_a_null_context_is_an_error_code_at_every_entry_point():
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    n = np.zeros(4, dtype=np.int64)
    v = np.zeros(4)
    assert lib.bi_sourcewise_events_begin(None, 1, _capi.ptr(n), 0.0) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_events_set_row(None, 0, 0, _capi.ptr(v)) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_events_end(None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_score_events(None, 0, 1, None, None, 1, _capi.ptr(n), None, 0.0) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_drop_events(None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_event_set_counts(None, _capi.ptr(n)) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_download_event_set(None, 0, _capi.ptr(v)) == _capi.ERR_INVALID
