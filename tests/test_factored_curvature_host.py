"""Second derivatives of source-wise (factored) models without a GPU: the NumPy specification (factored_curvature_oracle)
against the exact oracles of the expanded grid, the fixture of the unbounded counts, the header / binding of the two C-ABI
symbols, and the Python class over a recording context."""
import os
import re

import numpy as np
import pytest

import factored_curvature_oracle as fc
import factored_oracle as fo
import fisher_oracle
from derivative_oracle import C_POISSON, check_entries, derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ANCHOR = (3, 2, 4)
OWNERSHIPS = {'disjoint': ((0,), (1, 2), ()),                       # the models of test_factored_host.py
              'shared': ((0, 1), (0, 2), (1,), (0, 1, 2))}          # axes 0, 1 and 2 each have two or three owners


def small_points(model, rng):
    """points inside cells, exactly on interior anchors, and on the upper edge of the box (z [d], rs [S])"""
    g = model['anchor_z']
    S = len(model['own'])
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    pts = [(lo + (hi - lo) * rng.uniform(0.05, 0.95, 3), rng.uniform(0.5, 1.6, S)) for _ in range(2)]
    on = lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)
    on[0], on[2] = g[0][1], g[2][2]
    pts.append((on, rng.uniform(0.5, 1.6, S)))
    pts.append((hi.copy(), rng.uniform(0.5, 1.6, S)))
    return pts


@pytest.mark.parametrize('owners', sorted(OWNERSHIPS))
@pytest.mark.parametrize('B', [63, 1001])
def test_specification_against_the_oracles_of_the_expansion(B, owners):
    own = OWNERSHIPS[owners]
    rng = np.random.default_rng(300 + B + len(own))
    worst, worst_info = 0.0, 0.0
    for k in range(2):
        model = fo.random_model(rng, N_ANCHOR, own, B, zero_quarter=(1,) if k else ())
        full = fo.expand(model)
        for z, rs in small_points(model, rng):
            counts = rng.poisson(fo.expectation(model, z, rs)).astype(float)
            got = fc.curvature(model, z, rs, counts)
            want = derivatives(full, z, rs, counts, hessian=True)
            for key in ('ll', 'grad', 'hess'):
                worst = max(worst, check_entries(got[key], want[key], want[key + '_cond'], what='%s B=%d %s' % (key, B, owners)))
            np.testing.assert_array_equal(got['hess'], got['hess'].T)
            nobody = [i for i in range(3) if not any(i in o for o in own)]
            assert not got['hess'][nobody].any()
            info = fc.information(model, z, rs)
            want_info = fisher_oracle.information(full, z, rs)
            worst_info = max(worst_info, fisher_oracle.check(info['info'], want_info, what='info B=%d %s' % (B, owners)))
            np.testing.assert_array_equal(info['unbounded'], want_info['unbounded'])
            assert abs(info['total'] - want_info['total']) <= 1e-12 * want_info['total'] and not info['negative']
    print('B = %d, %s: worst |err| / (2^-52 cond) = %.3g of C = %d; information %.3g of 1e-10 max(1, cond)'
          % (B, owners, worst, C_POISSON, worst_info))


def test_unbounded_fixture_agrees_with_the_expanded_oracle():
    model, z, rs, want = fc.unbounded_fixture()
    got = fc.information(model, z, rs)
    full = fisher_oracle.information(fo.expand(model), z, rs)
    np.testing.assert_array_equal(got['unbounded'], want)
    np.testing.assert_array_equal(full['unbounded'], want)
    fisher_oracle.check(got['info'], full, what='unbounded fixture')


def test_header_and_binding_of_the_two_symbols():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    build.build()
    lib = _capi.load()
    for s in ('bi_eval_sourcewise_hess', 'bi_eval_sourcewise_fisher'):
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text)
        assert proto, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.group(1).split(',') if a.strip()]), s
    assert _capi.SIGNATURES['bi_eval_sourcewise_hess'] == _capi.SIGNATURES['bi_eval_hess']
    assert _capi.SIGNATURES['bi_eval_sourcewise_fisher'] == _capi.SIGNATURES['bi_eval_fisher']
    assert 'tu_factored_curv' in build.UNITS and 'tu_factored_fisher' in build.UNITS
    one = np.ones(64)
    p = _capi.ptr
    assert lib.bi_eval_sourcewise_hess(None, 1, p(one), None, None, p(one.copy()), p(one.copy()), p(one.copy()), None) == _capi.ERR_INVALID
    assert lib.bi_eval_sourcewise_fisher(None, 1, p(one), None, p(one.copy()), None, None, None) == _capi.ERR_INVALID


# ---- the Python class over a recording context ----------------------------------------------------------------------

class RecordingCurvatureContext:
    """Stands where SourceWiseContext would: records uploads and the second-order calls, answers them with -identity / identity"""

    def __init__(self, device=None):
        self.calls = []
        self.T = 0

    def begin_model(self, anchor_z, S, B, own_axes):
        self.d, self.S, self.B = len(anchor_z), S, B

    def set_anchor(self, s, local_index, ps_row, mu):
        pass

    def end_model(self):
        pass

    def set_counts(self, counts):
        self.T = np.asarray(counts).size // self.B

    def eval_hess(self, z, rate_scale=None, dataset=None):
        P, F = len(z), self.d + self.S
        self.calls.append(('eval_hess', P, None if dataset is None else np.array(dataset)))
        return np.zeros(P), np.zeros((P, self.d)), np.zeros((P, self.S)), np.tile(-np.eye(F), (P, 1, 1)), np.zeros(P, dtype=np.int32)

    def eval_fisher(self, z, rate_scale=None):
        P, F = len(z), self.d + self.S
        self.calls.append(('eval_fisher', P, None))
        return np.tile(np.eye(F), (P, 1, 1)), np.ones(P), np.zeros((P, F), dtype=np.int64), np.zeros(P, dtype=np.int32)


@pytest.fixture
def recorded(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingCurvatureContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    lf.prepare()
    return lf, names


def test_the_unrefused_names_reach_the_context(recorded, monkeypatch):
    from blueice_amd import inference
    lf, names = recorded
    assert not lf.supports_hessian                              # no data yet
    lf.set_binned_data(np.ones((6, 5)))
    assert lf.supports_hessian and lf.hessian_method == 'analytic'
    calls = lf.ctx.calls
    F = 4 + len(names)
    truth = {names[0]: 0.5, 's1_rate_multiplier': 1.2}

    ll, grads, order, H = lf.value_gradient_hessian(**truth)
    assert calls.pop() == ('eval_hess', 1, None) and H.shape == (F, F) and len(order) == F
    pts = {names[1]: np.array([-0.5, 0.0, 0.5])}
    ll, grads, order, H = lf.values_gradients_hessians(pts)
    assert calls.pop()[:2] == ('eval_hess', 3) and H.shape == (3, F, F) and lf.hessian_method == 'analytic'
    np.testing.assert_array_equal(H[1], -np.eye(F))

    floating, cov = inference.hesse(lf, {names[0]: 0.5, 's0_rate_multiplier': 1.0})
    assert calls.pop()[:2] == ('eval_hess', 1) and floating == ['s0_rate_multiplier', names[0]]
    np.testing.assert_allclose(cov, np.eye(2), atol=1e-15)
    lf.set_binned_data(np.ones((3, 6, 5)))
    floating, cov = inference.hesse(lf, {names[0]: np.array([0.5, 0.1, -0.3])}, datasets=np.arange(3))
    last = calls.pop()
    assert last[:2] == ('eval_hess', 3) and list(last[2]) == [0, 1, 2] and cov.shape == (3, 1, 1)
    floating, cov = inference.hesse(lf, {names[0]: 0.5}, information='expected')
    assert calls.pop() == ('eval_fisher', 1, None) and cov.shape == (1, 1)

    order, info, unb = lf.fisher_information_points({names[2]: np.array([0.0, 1.0])})
    assert calls.pop() == ('eval_fisher', 2, None) and info.shape == (2, F, F) and unb.shape == (2, F) and not unb.any()
    order, cov = lf.expected_covariance(**truth)
    assert calls.pop() == ('eval_fisher', 1, None) and cov.shape == (F, F)
    errors = lf.expected_errors(floating=['s1_rate_multiplier'], **truth)
    assert calls.pop() == ('eval_fisher', 1, None) and list(errors) == ['s1_rate_multiplier'] and errors['s1_rate_multiplier'] == 1.0

    # bestfit_minuit: the fit is the batched engine's (stubbed here), the errors come from the context's Hessian
    best = dict([('s%d_rate_multiplier' % s, 1.0) for s in range(4)] + [(n, 0.0) for n in names])
    monkeypatch.setattr(inference, 'bestfit_device', lambda lf_, guess=None, **kw: (dict(best), -1.0))
    result, value = lf.bestfit_minuit()
    assert calls.pop()[:2] == ('eval_hess', 1) and value == -1.0
    assert all(result[k + '_error'] == 1.0 for k in best)
    assert not calls


def test_the_two_bound_names_and_the_other_refusals_stay(recorded):
    lf, names = recorded
    lf.set_binned_data(np.ones((6, 5)))
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.hesse()
    assert 'blueice_amd.inference.hesse(lf, values)' in str(e.value)
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.fisher_information()
    assert 'lf.fisher_information_points' in str(e.value) and 'lf.expected_covariance' in str(e.value)
    with pytest.raises(NotImplementedError, match='source-wise'):          # an argument does not make the call special
        lf.hesse({names[0]: 0.0})
    for name in ('simulate_toys', 'bestfit_toys', 'toy_mc_fits', 'goodness_of_fit', 'gof_statistics', 'asimov', 'real_data',
                 'expected_upper_limit', 'grid_scan', 'expected_coarse', 'coarse_information', 'expected_coarse_jacobian',
                 'sample_posterior', 'bestfit_emcee', 'expected_counts', 'expected_counts_points', 'ps_interpolator'):
        with pytest.raises(NotImplementedError, match='source-wise'):
            getattr(lf, name)()
    # the gate of everything else behind _binned_for_gof keeps refusing the class
    from blueice_amd.coarse import _binned_for_gof
    with pytest.raises(NotImplementedError, match='BinnedLogLikelihood'):
        _binned_for_gof(lf, 'expected_counts')
    from blueice_amd import inference
    with pytest.raises(NotImplementedError):
        inference.expected_counts(lf)
    assert not lf.ctx.calls
