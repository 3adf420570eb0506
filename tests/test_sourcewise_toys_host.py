"""Source-wise toys, goodness of fit and expected counts without a GPU: the conditions the GPU replay rests on (the undecided
share of every input, no expectation on the knife edge at 10, mutants of the stream that the comparison must reject on these
inputs), the header / binding of the four C-ABI symbols, and the Python layers over a recording context."""
import os
import re

import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_toy_cases as cases
import toy_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('bi_sourcewise_expected_counts', 'bi_eval_sourcewise_gof', 'bi_sourcewise_generate_toys', 'bi_sourcewise_download_counts')


def _replays():
    """(case, offset, truth, mu, replay) of every toy the GPU tests draw: the H = 3 calls at both offsets"""
    for name in cases.ALL_CASES:
        model, z, rs = cases.make_case(name)
        h_of = cases.truth_of_toy(cases.N_TOYS)
        for off in cases.TOY_OFFSETS:
            for h in range(3):
                toys = off + np.flatnonzero(h_of == h)
                if len(toys):
                    mu = fo.expectation(model, z[h], rs[h])
                    yield name, off, h, mu, orc.per_bin_toys(mu, cases.SEED, toys.astype(np.uint64))
    model, z, rs = cases.make_case('B1')                     # ... and the toys around the launch boundary of the 32 770-toy call
    mu = fo.expectation(model, z[0], rs[0])
    yield 'B1 launch boundary', 0, 0, mu, orc.per_bin_toys(mu, cases.SEED, np.array(cases.LAUNCH_BOUNDARY_TOYS, dtype=np.uint64))


def test_undecided_share_of_the_gpu_inputs_is_within_the_cap():
    """Pooled per bin count (a case of a few thousand draws cannot show a share of 10^-5) -- and, because compare_toys holds
    every single call to the cap, no call of these small cases may have an undecided draw at all with this seed."""
    pooled = {}
    for name, off, h, mu, rep in _replays():
        d, u = pooled.get(len(mu), (0, 0))
        pooled[len(mu)] = (d + rep.draws, u + rep.undecided)
        assert rep.undecided <= orc.CAP * rep.draws, (name, off, h, rep.undecided, rep.draws)
        orc.compare_toys(rep.counts, rep, what='%s offset %d truth %d' % (name, off, h))        # the oracle against itself
    report = ', '.join('B = %d: %d of %d' % (B, u, d) for B, (d, u) in sorted(pooled.items()))
    print(report)
    for B, (d, u) in pooled.items():
        assert u <= orc.CAP * d, "undecided share at B = %d is %g; all: %s" % (B, u / d, report)


def test_no_expectation_on_the_knife_edge_and_both_branches_are_exercised():
    """within 2^-40 relative of 10 an ulp of mu_b would switch the algorithm; `zero_both_sides` has bins of mu_b = 0 exactly, bins
    below 10 and bins from 10"""
    for name in cases.ALL_CASES:
        model, z, rs = cases.make_case(name)
        for h in range(3):
            mu = fo.expectation(model, z[h], rs[h])
            assert np.all(np.abs(mu - 10.0) > 2.0 ** -40 * 10.0), (name, h)
            assert np.all(np.isfinite(mu)) and np.all(mu >= 0.0)
            if name == 'zero_both_sides':
                live = np.setdiff1d(np.arange(len(mu)), cases.ZERO_BINS)
                assert np.all(mu[cases.ZERO_BINS] == 0.0) and np.all(mu[live] > 0.0)
                assert (mu[live] < 10.0).sum() >= 20 and (mu[live] >= 10.0).sum() >= 20, (h, (mu[live] < 10).sum())


@pytest.mark.parametrize('mutant', ['odd01', 'attempt0', 'shift05', 'us13'])
def test_per_bin_mutants_are_caught_on_these_inputs(mutant):
    """the mutants of per_bin_toys the oracle knows, on the input with both branches: the comparison rejects each of them"""
    model, z, rs = cases.make_case('zero_both_sides')
    mu = fo.expectation(model, z[0], rs[0])
    toys = np.arange(8, dtype=np.uint64)
    rep = orc.per_bin_toys(mu, cases.SEED, toys)
    with pytest.raises(AssertionError, match='mismatches'):
        orc.compare_toys(orc.per_bin_toys(mu, cases.SEED, toys, mutant=mutant).counts, rep)


def test_truncated_dataset_word_is_caught_at_the_offset_seam():
    model, z, rs = cases.make_case('B63')
    mu = fo.expectation(model, z[0], rs[0])
    toys = np.arange(cases.TOY_OFFSETS[1], cases.TOY_OFFSETS[1] + 8, dtype=np.uint64)
    rep = orc.per_bin_toys(mu, cases.SEED, toys)
    with pytest.raises(AssertionError, match='mismatches'):
        orc.compare_toys(orc.per_bin_toys(mu, cases.SEED, toys, mutant='trunc32').counts, rep)


def test_exact_expectation_agrees_with_the_float64_specification():
    for name in ('B63', 'mixed_padded', 'zero_both_sides'):
        model, z, rs = cases.make_case(name)
        mu, per = cases.exact_expectation(model, z[1], rs[1])
        np.testing.assert_allclose(mu.astype(float), fo.expectation(model, z[1], rs[1]), rtol=1e-14, atol=0)
        assert per.shape == (len(model['own']), fo.n_bins(model))


def test_header_and_binding_of_the_four_symbols():
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
    assert _capi.SIGNATURES['bi_eval_sourcewise_gof'] == _capi.SIGNATURES['bi_eval_gof']
    assert _capi.SIGNATURES['bi_sourcewise_expected_counts'] == _capi.SIGNATURES['bi_expected_counts']
    assert _capi.SIGNATURES['bi_sourcewise_download_counts'] == _capi.SIGNATURES['bi_download_counts']
    # the store's six symbols are still the only ones that say "factored"
    assert sorted(s for s in re.findall(r'\b(bi_[a-z_0-9]+)\s*\(', text) if 'factored' in s) == sorted(
        {'bi_factored_begin', 'bi_factored_set_anchor', 'bi_factored_end', 'bi_factored_set_counts', 'bi_eval_factored', 'bi_fit_batched_factored'})
    assert 'tu_sourcewise_expect' in build.UNITS and 'tu_sourcewise_gof' in build.UNITS
    one = np.ones(64)
    p = _capi.ptr
    assert lib.bi_sourcewise_expected_counts(None, 1, p(one), None, 0, p(one.copy())) == _capi.ERR_INVALID
    assert lib.bi_eval_sourcewise_gof(None, 1, p(one), None, None, p(one.copy()), p(one.copy()), None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_generate_toys(None, 1, p(one), None, p(np.ones(1, dtype=np.int64)), 1) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_download_counts(None, 0, p(one.copy())) == _capi.ERR_INVALID


# ---- the Python layers over a recording context -----------------------------------------------------------------------

class RecordingToyContext:
    """Stands where SourceWiseContext would: records what the inference layers ask of it and answers with plausible shapes"""

    def __init__(self, device=None):
        self.calls = []
        self.T = 0
        self.params = {}

    def begin_model(self, anchor_z, S, B, own_axes):
        self.d, self.S, self.B = len(anchor_z), S, B

    def set_anchor(self, s, local_index, ps_row, mu):
        pass

    def end_model(self):
        pass

    def set_counts(self, counts):
        self.T = np.asarray(counts).size // self.B
        self.calls.append(('set_counts', self.T))

    def set_param(self, name, value):
        self.params[name] = int(value)
        self.calls.append(('set_param', name, int(value)))

    def get_param(self, name):
        return self.params.get(name, 0)

    def download_counts(self, t=0):
        return np.full(self.B, float(t))

    def generate_toys_points(self, z, rate_scale=None, n_toys=1, seed=0):
        n_toys = np.atleast_1d(n_toys)
        self.calls.append(('generate_toys_points', np.array(z), np.array(rate_scale), n_toys.copy(), seed, self.params.get('toy_offset', 0)))
        self.T = int(n_toys.sum())
        return np.where(n_toys > 0, 0, -1).astype(np.int32)

    def eval_gof(self, z, rate_scale=None, dataset=None):
        P = len(z)
        self.calls.append(('eval_gof', P, None if dataset is None else np.array(dataset)))
        return np.full(P, 3.0), np.full(P, 7.0), np.zeros(P, dtype=np.int32)

    def expected_counts(self, z, rate_scale=None, per_source=False):
        P = len(z)
        self.calls.append(('expected_counts', P, bool(per_source)))
        return np.ones((P, self.S, self.B) if per_source else (P, self.B))

    def eval(self, z, rate_scale=None, dataset=None):
        P = len(np.atleast_2d(z))
        return np.zeros(P), np.zeros(P, dtype=np.int32)


@pytest.fixture
def recorded(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingToyContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    lf.prepare()
    return lf, names


PINNED = {'simulate_toys': 'lf.simulate_toys_points(', 'bestfit_toys': 'blueice_amd.inference.bestfit_toys(lf',
          'toy_mc_fits': 'blueice_amd.inference.toy_mc_fits(lf', 'gof_statistics': 'blueice_amd.inference.gof_statistics(lf',
          'goodness_of_fit': 'blueice_amd.inference.goodness_of_fit(lf', 'expected_counts': 'blueice_amd.inference.expected_counts_points(lf',
          'expected_counts_points': 'blueice_amd.inference.expected_counts_points(lf'}


def test_pinned_bound_names_refuse_and_name_the_spelling_that_works(recorded):
    lf, names = recorded
    lf.set_binned_data(np.ones((6, 5)))
    n_before = len(lf.ctx.calls)
    for name, spelling in PINNED.items():
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            getattr(lf, name)()
        assert spelling in str(e.value), (name, str(e.value))
    for name in ('asimov', 'real_data', 'grid_scan', 'expected_coarse', 'sample_posterior', 'eval_toys', 'eval_toys_points'):
        with pytest.raises(NotImplementedError, match='source-wise'):
            getattr(lf, name)()
    from blueice_amd import inference
    with pytest.raises(NotImplementedError):
        inference.expected_counts(lf)
    assert 'expected_counts_points' in inference.expected_counts.__doc__
    assert len(lf.ctx.calls) == n_before
    for name in ('simulate_toys_points', 'toy_test_statistics', 'neyman_thresholds'):
        assert name not in type(lf)._REFUSED and callable(getattr(lf, name))


def test_module_level_functions_reach_the_context(recorded, monkeypatch):
    from blueice_amd import inference
    lf, names = recorded
    calls = lf.ctx.calls
    F = 4 + len(names)

    # expected counts: no data needed
    mu = inference.expected_counts_points(lf, {names[0]: np.array([-0.5, 0.0, 0.5])})
    assert calls.pop() == ('expected_counts', 3, False) and mu.shape == (3, 6, 5)
    mu = inference.expected_counts_points(lf, {names[1]: np.array([0.25])}, per_source=True)
    assert calls.pop() == ('expected_counts', 1, True) and mu.shape == (1, 4, 6, 5)

    # toys at truth points: the host terms reach the generator, the truth's index is in the box error
    methods = lf.simulate_toys_points({names[0]: np.array([0.5, -0.5, 1.0]), 's1_rate_multiplier': 1.5}, [2, 0, 1], seed=11)
    kind, z, scale, n_toys, seed, _ = calls.pop()
    assert kind == 'generate_toys_points' and z.shape == (3, len(names)) and scale.shape == (3, 4) and seed == 11
    np.testing.assert_array_equal(z[:, 0], [0.5, -0.5, 1.0])
    np.testing.assert_array_equal(scale[:, 1], [1.5, 1.5, 1.5])
    np.testing.assert_array_equal(n_toys, [2, 0, 1])
    np.testing.assert_array_equal(methods, [0, -1, 0])
    np.testing.assert_array_equal(lf.toy_truth, [0, 0, 2])
    assert lf.is_data_set and lf.ctx.T == 3
    with pytest.raises(ValueError, match='truth 1'):
        lf.simulate_toys_points({names[0]: np.array([0.5, 2.5])}, 2)

    # goodness-of-fit statistics of the resident datasets
    out = inference.gof_statistics(lf, {names[0]: np.array([0.1, 0.2, 0.3])}, datasets=np.arange(3))
    last = calls.pop()
    assert last[:2] == ('eval_gof', 3) and list(last[2]) == [0, 1, 2]
    np.testing.assert_array_equal(out['deviance'], [6.0, 6.0, 6.0])
    np.testing.assert_array_equal(out['pearson'], [7.0, 7.0, 7.0])
    assert out['n_bins'] == 30
    with pytest.raises(NotImplementedError, match='binning'):
        inference.gof_statistics(lf, {names[0]: 0.1}, binning=object())
    with pytest.raises(NotImplementedError, match='binning'):
        inference.goodness_of_fit(lf, n_toys=2, binning=object())

    # toy_mc_fits / goodness_of_fit: the toys are drawn through simulate_toys_points with one truth, numbered by toy_offset
    best = dict([('s%d_rate_multiplier' % s, 1.0) for s in range(4)] + [(n, 0.0) for n in names])

    def fake_fit(lf_, datasets=None, return_info=False, **kw):
        n = 1 if datasets is None else len(datasets)
        b = {k: np.full(n, v) for k, v in best.items()}
        info = dict(failed=np.zeros(n, dtype=bool))
        return (b, np.zeros(n), info) if return_info else (b, np.zeros(n))

    monkeypatch.setattr(inference, 'bestfit_batched', fake_fit)
    del calls[:]
    fitted, ll = inference.toy_mc_fits(lf, 5, chunk=2, seed=3, truth={names[0]: 0.5}, first_toy=10)
    gen = [c for c in calls if c[0] == 'generate_toys_points']
    assert [int(c[3][0]) for c in gen] == [2, 2, 1] and [c[5] for c in gen] == [10, 12, 14] and all(c[4] == 3 for c in gen)
    assert all(c[1].shape == (1, len(names)) and c[1][0, 0] == 0.5 for c in gen)
    assert len(ll) == 5 and len(fitted) == F and lf.ctx.params['toy_offset'] == 0

    lf.set_binned_data(np.ones((6, 5)))
    del calls[:]
    res = inference.goodness_of_fit(lf, n_toys=3, chunk=2, seed=4)
    gen = [c for c in calls if c[0] == 'generate_toys_points']
    assert [int(c[3][0]) for c in gen] == [2, 1] and [c[5] for c in gen] == [0, 2]
    assert res.ndof == 30 - F and res.observed == 6.0 and len(res.toys) == 3 and 0 < res.p_value <= 1
    assert calls[-1] == ('set_counts', 1)                          # the likelihood's own data are handed back
    assert lf.ctx.params['toy_offset'] == 0
