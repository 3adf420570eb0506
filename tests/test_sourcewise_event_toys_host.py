"""Event toys of unbinned source-wise likelihoods without a GPU: what the Python functions hand the context (over a recording
context), their refusals, the C-ABI symbols, and the oracle of the GPU tests' cases on its own."""
import os
import re

import numpy as np
import pytest

import sourcewise_event_toy_cases as cases
import toy_oracle as to
from test_sourcewise_events_host import RecordingContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ToyRecorder(RecordingContext):
    """... and records the generator call; the "toys" it reports have 3 + t + s events"""

    def simulate_event_toys(self, method, edges, z, rate_scale=None, n_toys=1, seed=0, outlier_likelihood=0.0):
        n_toys = np.atleast_1d(n_toys)
        self.log.append(('simulate', method, [np.asarray(e, float) for e in edges], None if z is None else np.array(z, float),
                         np.array(rate_scale, float), n_toys.copy(), seed, outlier_likelihood))
        self.T = int(n_toys.sum())
        return np.array([[3 + t + s for s in range(self.S)] for t in range(self.T)], dtype=np.int64)

    def set_param(self, name, value):
        self.log.append(('param', name, value))


def histogram_likelihood(monkeypatch, method, **likelihood_config):
    import blueice_amd.source_wise as sw
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', ToyRecorder)
    conf, names, own = many_nuisances_config(n_bins=(6, 5), n_params=4, n_sources=3, own_per_source=1, source_class=NuisanceHistogramSource)
    conf['pdf_interpolation_method'] = method
    lf = SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False, **likelihood_config))
    for s in range(3):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    lf.prepare()
    return lf, conf, names


@pytest.mark.parametrize('method', ['piecewise', 'linear'])
def test_the_functions_hand_the_context_method_edges_truths_and_seed(monkeypatch, method):
    from blueice_amd import sourcewise_event_toys, sourcewise_event_toys_points
    lf, conf, names = histogram_likelihood(monkeypatch, method)
    rec = lf.ctx
    edges = [np.asarray(e, float) for _, e in conf['analysis_space']]
    pts = {names[0]: np.array([-1.5, 0.25, 2.0]), names[2]: 0.5, 's1_rate_multiplier': np.array([1.0, 2.0, 0.0])}
    counts = sourcewise_event_toys_points(lf, pts, [2, 0, 3], seed=77, livetime_days=2.0)
    kind, got_method, got_edges, z, scale, n_toys, seed, outlier = rec.log[-1]
    assert kind == 'simulate' and got_method == method and seed == 77 and outlier == 1e-12 and n_toys.tolist() == [2, 0, 3]
    for g, w in zip(got_edges, edges):                      # the bin EDGES for both methods: the events are drawn from bins
        np.testing.assert_array_equal(g, w)
    want_z, want_scale, _ = lf._batch_terms(pts, 2.0)
    np.testing.assert_array_equal(z, np.broadcast_to(want_z, (3, 4)))
    np.testing.assert_array_equal(scale, np.broadcast_to(want_scale, (3, 3)))
    assert z[:, 0].tolist() == [-1.5, 0.25, 2.0] and z[:, 2].tolist() == [0.5] * 3 and (z[:, [1, 3]] == 0).all()
    assert scale[:, 1].tolist() == [2.0, 4.0, 0.0] and scale[:, 0].tolist() == [2.0] * 3      # (live time: two days of one)
    assert counts.shape == (5, 3) and lf.toy_truth.tolist() == [0, 0, 2, 2, 2]
    assert lf.is_data_set and lf.bin_shape == (int(counts[0].sum()),) and lf.last_scoring_route == 'device' and lf._data is None
    # an int broadcasts over the truths; the one-truth spelling is a one-row call
    sourcewise_event_toys_points(lf, {names[1]: np.array([0.0, 1.0])}, 4, seed=3)
    assert rec.log[-1][5].tolist() == [4, 4] and lf.toy_truth.tolist() == [0] * 4 + [1] * 4
    sourcewise_event_toys(lf, 6, seed=5, **{names[3]: -0.5, 's0_rate_multiplier': 3.0})
    kind, _, _, z, scale, n_toys, seed, _ = rec.log[-1]
    assert kind == 'simulate' and z.shape == (1, 4) and z[0, 3] == -0.5 and scale[0, 0] == 3.0 and n_toys.tolist() == [6] and seed == 5
    with pytest.raises(ValueError, match='at least 1'):
        sourcewise_event_toys(lf, 0)
    before = len(rec.log)
    with pytest.raises(ValueError, match='cannot simulate outside the anchor box'):
        sourcewise_event_toys_points(lf, {names[0]: np.array([0.0, 2.5])}, 1)
    with pytest.raises(ValueError, match='cannot simulate outside the anchor box'):
        sourcewise_event_toys(lf, 2, **{names[1]: -2.01})
    assert len(rec.log) == before                           # nothing reached the context


def test_the_host_scoring_route_says_so(monkeypatch):
    from blueice_amd import sourcewise_event_toys, sourcewise_event_toys_points
    from blueice_amd.exceptions import NotPreparedException
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    lf, conf, names = histogram_likelihood(monkeypatch, 'linear', device_scoring=False)
    assert lf.scoring_route == 'host'
    for call in (lambda: sourcewise_event_toys(lf, 2), lambda: sourcewise_event_toys_points(lf, {names[0]: np.zeros(2)}, 1)):
        with pytest.raises(NotImplementedError, match="scoring_route == 'device'"):
            call()
    assert not any(entry[0] == 'simulate' for entry in lf.ctx.log)
    unprepared = SourceWiseUnbinnedLogLikelihood(conf)
    with pytest.raises(NotPreparedException):
        sourcewise_event_toys(unprepared, 2)
    with pytest.raises(TypeError):
        sourcewise_event_toys(object(), 2)


def test_bound_names_refuse_and_name_the_functions(monkeypatch):
    lf, conf, names = histogram_likelihood(monkeypatch, 'piecewise')
    for name in ('simulate_toy', 'simulate_toys', 'simulate_toys_points', 'simulated_events', 'toy_mc_fits', 'toy_test_statistics',
                 'neyman_thresholds'):
        with pytest.raises(NotImplementedError, match='unbinned source-wise model') as err:
            getattr(lf, name)()
        for spelling in ('sourcewise_event_toys(lf', 'sourcewise_event_toys_points(lf', 'sourcewise_simulated_events(lf',
                         'inference.toy_mc_fits(lf'):
            assert spelling in str(err.value), (name, spelling)


def test_the_inference_layers_reach_the_generator_through_the_private_method(monkeypatch):
    """toy_mc_fits and toy_test_statistics call one helper, which takes this class through `_simulate_toys_points`: the truths,
    the numbers of toys per truth (chunks across hypothesis boundaries) and the toy offsets of every chunk"""
    from blueice_amd import inference
    lf, conf, names = histogram_likelihood(monkeypatch, 'piecewise')
    rec = lf.ctx
    fits = []

    def fake_fit(lf_, datasets=None, points=None, return_info=False, **kw):
        n = len(datasets)
        fits.append((n, None if points is None else {k: np.array(v) for k, v in points.items()}))
        best = {p: np.zeros(n) for p in ['s0_rate_multiplier', 's1_rate_multiplier', 's2_rate_multiplier'] + names}
        info = dict(calls=1, converged=np.ones(n, bool), stalled=np.zeros(n, bool), failed=np.zeros(n, bool))
        return (best, np.zeros(n), info) if return_info else (best, np.zeros(n))

    monkeypatch.setattr(inference, 'bestfit_batched', fake_fit)
    monkeypatch.setattr(inference, 'supports_batched_fits', lambda lf_: True)
    inference.toy_mc_fits(lf, 7, chunk=3, seed=9, truth={names[0]: 0.5}, first_toy=100)
    calls = [e for e in rec.log if e[0] in ('simulate', 'param')]
    assert [(e[1], e[2]) for e in calls if e[0] == 'param'] == [('toy_offset', 100), ('toy_offset', 103), ('toy_offset', 106), ('toy_offset', 0)]
    sims = [e for e in calls if e[0] == 'simulate']
    assert [e[5].tolist() for e in sims] == [[3], [3], [1]] and all(e[6] == 9 and e[3][0, 0] == 0.5 for e in sims)
    del rec.log[:]
    hyp = np.array([0.5, 1.0, 2.0])
    stats = inference.toy_test_statistics(lf, 's1_rate_multiplier', hyp, 4, seed=11, chunk=5, truth={names[1]: np.array([-1.0, 0.0, 1.0])})
    sims = [e for e in rec.log if e[0] == 'simulate']
    assert [e[5].tolist() for e in sims] == [[4, 1], [3, 2], [2]]                      # mixed chunks: 5 + 5 + 2 toys of 3 x 4
    assert [e[4][:, 1].tolist() for e in sims] == [[0.5, 1.0], [1.0, 2.0], [2.0]]
    assert [e[3][:, 1].tolist() for e in sims] == [[-1.0, 0.0], [0.0, 1.0], [1.0]]
    assert [e[2] for e in rec.log if e[0] == 'param'] == [0, 5, 10, 0]
    assert stats.t.shape == (3, 4)
    table = inference.neyman_thresholds(lf, 's1_rate_multiplier', hyp, 4, seed=11, chunk=12)
    assert table.t.shape == (3, 4)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ['bi_sourcewise_simulate_event_toys', 'bi_sourcewise_simulated_event_count', 'bi_sourcewise_download_events']


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
    assert 'tu_sourcewise_sim' in build.UNITS
    for name in ('tu_sourcewise_sim.hip', 'bi_k_sourcewise_sim.h', 'bi_sourcewise_sim.h', 'bi_k_draw.h'):
        assert os.path.exists(os.path.join(build.CSRC, name))
    import ctypes as C
    n = lib.bi_list_params(None, 0)
    buf = C.create_string_buffer(n)
    lib.bi_list_params(buf, n)
    params = dict(line.split() for line in buf.value.decode().splitlines())
    assert params['sim_truth_chunk'] == 'rw'


def test_a_null_context_is_an_error_code_at_every_new_entry_point():
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    n = np.ones(1, dtype=np.int64)
    ne = np.array([3], dtype=np.int32)
    e = np.array([0.0, 1.0, 2.0])
    v = np.zeros(4)
    s = np.zeros(4, dtype=np.int32)
    assert lib.bi_sourcewise_simulate_event_toys(None, 0, 1, _capi.ptr(ne), _capi.ptr(e), 1, None, None, _capi.ptr(n), 0, 0.0, None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_simulated_event_count(None) == -1
    assert lib.bi_sourcewise_download_events(None, _capi.ptr(v), _capi.ptr(s)) == _capi.ERR_INVALID


# ---- the oracle on its own ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', cases.NAMES)
def test_the_oracle_alone_stays_within_the_cap(name):
    """every replayed toy of every case: the undecided share of the oracle's own draws is within toy_oracle.CAP (a case whose
    oracle decides too little would make the GPU test vacuous)"""
    out = cases.check_oracle_alone(name)
    print('%s: draws %s, undecided %s of cap %g' % (name, [d for d, _ in out], [u for _, u in out], to.CAP))
    if not name.startswith('class_'):
        assert all(10000 < d < 25000 for d, _ in out)


def test_the_layout_case_has_sets_on_both_sides_of_a_tile():
    n = cases.layout_counts(cases.make_case('k1', 2)).sum(axis=1)
    print('layout set lengths', n.tolist())
    assert n.min() < cases.TILE < n.max() and (n > 0).all()
