"""The analytic Hessian of unbinned source-wise likelihoods without a GPU: the NumPy specification
(sourcewise_events_curvature_oracle) against the exact oracle of the expanded grid, the `analytic_hessian` switch of
SourceWiseUnbinnedLogLikelihood over a recording context, and the header / binding / build list of the new C-ABI symbol.

Four tests validate the new NumPy oracle and pass without the feature (they touch no library code):
`test_specification_against_the_oracle_of_the_expansion[1|63|1001]`, against `derivative_oracle.derivatives(expand(model),
unbinned=True, hessian=True)`, and `test_no_events_is_the_curvature_of_minus_the_rates`.  Every other test here fails without
it."""
import os
import re

import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_events_curvature_oracle as co
import sourcewise_events_oracle as eo
from derivative_oracle import C_POISSON, check_entries, derivatives
from test_sourcewise_events_host import N_ANCHOR, OWN, RecordingContext, event_model, histogram_likelihood, points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = 'bi_eval_sourcewise_events_hess'


# ---- the specification against the oracle of the expansion ------------------------------------------------------------------

@pytest.mark.parametrize('N', [1, 63, 1001])
def test_specification_against_the_oracle_of_the_expansion(N):
    """plain models, a source that is exactly 0 at a quarter of the events, and (k = 2) a clamped event and a nan corner"""
    rng = np.random.default_rng(700 + N)
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
                got = co.events_curvature(model, z, rs, outlier=outlier)
                if outlier == 0.0 and k == 2 and N > 1:
                    assert got['ll'] == -np.inf and np.isnan(got['grad']).all() and np.isnan(got['hess']).all()
                    continue
                want = derivatives(full, z, rs, unbinned=True, outlier=outlier, hessian=True)
                worst = max(worst, check_entries(got['ll'], want['ll'], want['ll_cond'], what='ll N=%d' % N))
                worst = max(worst, check_entries(got['grad'], want['grad'], want['grad_cond'], what='grad N=%d' % N))
                worst = max(worst, check_entries(got['hess'], want['hess'], want['hess_cond'], what='hess N=%d' % N))
                assert np.array_equal(got['hess'], got['hess'].T)
                first = eo.events_derivatives(model, z, rs, outlier=outlier)
                assert got['ll'] == first['ll'] and np.array_equal(got['grad'], first['grad'])
                if outlier:
                    assert got['n_clamped'] == (1 if k == 2 and N > 1 else 0)
    print('N = %d: worst |err| / (2^-52 cond) = %.3g of C = %d' % (N, worst, C_POISSON))


def test_no_events_is_the_curvature_of_minus_the_rates():
    rng = np.random.default_rng(6)
    model = event_model(rng, N_ANCHOR, OWN, 0)
    z, rs = points(model, rng)[0]
    got = co.events_curvature(model, z, rs)
    total, dtotal, d2total = co.rate_curvature(model, z, rs)
    assert got['ll'] == -float(total.v) and np.array_equal(got['grad'], -dtotal.v)
    d = len(model['anchor_z'])
    H = got['hess']
    assert np.all(H[d:, d:] == 0.0) and np.all(np.diag(H) == 0.0) and H[1, 2] != 0.0 and H[0, d] != 0.0 and H[0, 1] == 0.0


# ---- the switch of the class over a recording context -----------------------------------------------------------------------

class HessianRecorder(RecordingContext):
    """RecordingContext that answers eval_events_hess with zeros of eval_hess's shapes and records that it was asked"""
    hess_calls = 0

    @property
    def d(self):
        return len(self.anchor_z)

    def eval_events_hess(self, z, rate_scale=None, dataset=None):
        type(self).hess_calls += 1
        P = len(rate_scale)
        F = self.d + self.S
        return np.zeros(P), np.zeros((P, self.d)), np.zeros((P, self.S)), np.zeros((P, F, F)), np.zeros(P, dtype=np.int32)

    def eval_hess(self, z, rate_scale=None, dataset=None):
        raise AssertionError("the binned entry point is not the event store's")


def test_the_config_switch(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd import LogLikelihoodSum
    import test_sourcewise_events_host as host
    monkeypatch.setattr(host, 'RecordingContext', HessianRecorder)
    HessianRecorder.hess_calls = 0
    off, _ = histogram_likelihood(monkeypatch, 'linear')
    on, _ = histogram_likelihood(monkeypatch, 'linear', analytic_hessian=True)
    assert isinstance(on.ctx, HessianRecorder) and sw.SourceWiseContext is HessianRecorder
    # before data: no Hessian either way
    assert not off.supports_hessian and not on.supports_hessian
    np.random.seed(4)
    d = on.base_model.simulate()
    for lf in (off, on):
        lf.set_data(d)
    assert not off.supports_hessian and off.hessian_method == 'gradient-differences'
    assert on.supports_hessian and on.hessian_method == 'analytic'
    assert LogLikelihoodSum([on, on]).hessian_method == 'analytic'
    assert LogLikelihoodSum([on, off]).hessian_method == 'gradient-differences'
    ll, grads, names, H = on.values_gradients_hessians({'np0': np.array([0.5, -0.5])})
    assert HessianRecorder.hess_calls == 1 and on.hessian_method == 'analytic'
    assert H.shape == (2, 12, 12) and len(names) == 12 and ll.shape == (2,)
    # the expected information stays refused: events carry none
    for name in ('fisher_information', 'fisher_information_points', 'expected_errors', 'expected_covariance'):
        with pytest.raises(NotImplementedError, match='unbinned source-wise model'):
            getattr(on, name)()
    assert 'analytic_hessian' in type(on).supports_hessian.__doc__


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_header_binding_and_build_list_agree_on_the_new_symbol():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(bi_[a-z_0-9]+)\s*\(', text))
    build.build()
    lib = _capi.load()
    assert 'factored' not in SYMBOL
    assert SYMBOL in declared, "%s is not declared in include/blueice_hip.h" % SYMBOL
    assert hasattr(lib, SYMBOL), "library does not export %s" % SYMBOL
    assert SYMBOL in _capi.SIGNATURES, "ctypes binding lacks %s" % SYMBOL
    proto = re.search(r'\b%s\s*\(([^)]*)\)' % SYMBOL, text).group(1)
    assert len(_capi.SIGNATURES[SYMBOL][1]) == len([a for a in proto.split(',') if a.strip()]) == 9
    assert _capi.SIGNATURES[SYMBOL] == _capi.SIGNATURES['bi_eval_sourcewise_hess']
    assert 'tu_sourcewise_events_curv' in build.UNITS
    for name in ('tu_sourcewise_events_curv.hip', 'bi_k_sourcewise_events_curv.h'):
        assert os.path.exists(os.path.join(build.CSRC, name))


def test_a_null_context_is_an_error_code():
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    v = np.zeros(16)
    st = np.zeros(1, dtype=np.int32)
    assert lib.bi_eval_sourcewise_events_hess(None, 1, _capi.ptr(v), _capi.ptr(v), None, _capi.ptr(v), _capi.ptr(v), _capi.ptr(v),
                                              _capi.ptr(st)) == _capi.ERR_INVALID
