"""Derivatives of the coarse views of a source-wise model without a GPU: the four `sourcewise_coarse_*` functions of
blueice_amd.coarse over a recording context that stands where SourceWiseContext would (its expected_coarse_jacobian records the
arguments and returns a recognisable pattern), the chain rule to the user's parameters at a live time other than the base one,
the refusals, and the header / binding of bi_sourcewise_expected_coarse_jacobian."""
import os
import re

import numpy as np
import pytest

from test_sourcewise_coarse_host import RecordingCoarseContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = 'bi_sourcewise_expected_coarse_jacobian'
NEW = ('sourcewise_coarse_jacobian_points', 'sourcewise_coarse_jacobian', 'sourcewise_coarse_band', 'sourcewise_coarse_information')
PINNED = {'expected_coarse_jacobian_points': 'blueice_amd.coarse.sourcewise_coarse_jacobian_points(lf, binning, points',
          'expected_coarse_jacobian': 'blueice_amd.coarse.sourcewise_coarse_jacobian(lf, binning',
          'expected_coarse_band': 'blueice_amd.coarse.sourcewise_coarse_band(lf, binning, names, covariance',
          'coarse_information': 'blueice_amd.coarse.sourcewise_coarse_information(lf, binning'}


def pattern(P, S, F, C, per_source):
    """mu of cell c: 1 + c (source s: (1 + s) / 10 of it); d mu_C / d theta_k of point p: (1 + k) (1 + c) + p / 8 (source s:
    (1 + s) / 10 of it): exact in binary where it matters"""
    mu = np.broadcast_to(1.0 + np.arange(C), (P, C)).copy()
    jac = (1.0 + np.arange(F))[None, :, None] * (1.0 + np.arange(C))[None, None, :] + np.arange(P)[:, None, None] / 8.0
    if per_source:
        share = (1.0 + np.arange(S)) / 10.0
        mu = mu[:, None, :] * share[None, :, None]
        jac = jac[:, None, :, :] * share[None, :, None, None]
    return mu, jac


class RecordingJacobianContext(RecordingCoarseContext):
    def expected_coarse_jacobian(self, n_cells, z, rate_scale=None, per_source=False):
        assert n_cells == self.cells
        self.calls.append(('expected_coarse_jacobian', n_cells, np.array(z), np.array(rate_scale), bool(per_source)))
        mu, jac = pattern(len(z), self.S, self.d + self.S, n_cells, per_source)
        return mu, jac, np.zeros(len(z), dtype=np.int32)


def make_lf(monkeypatch, prepare=True):
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingJacobianContext)
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


def user_matrix(lf, pts, P, livetime):
    from blueice_amd.hessian import user_jacobian
    z, scale, _ = lf._batch_terms(pts, livetime)
    mult, L, eff, eff_axis, rate_sources = lf._chain_rule_terms(pts, P, livetime)
    return z, scale, user_jacobian(P, z.shape[1], scale.shape[1], mult, L, eff, eff_axis, rate_sources)


def test_the_four_functions_reach_the_context_once_each(recorded):
    from blueice_amd import coarse
    lf, names, conf = recorded
    assert all(n in coarse.__all__ and callable(getattr(coarse, n)) for n in NEW)
    first = str(conf['analysis_space'][0][0])
    b = coarse.CoarseBinning(lf, rebin={first: 3})
    d, S, F = len(names), 4, len(names) + 4
    livetime = 2.5                                      # of a base live time of 1.0: U is not the identity
    pts = {names[0]: np.array([-0.5, 0.0, 0.5]), 's1_rate_multiplier': np.array([1.5, 0.75, 1.25])}
    z_want, scale_want, U = user_matrix(lf, pts, 3, livetime)
    assert not np.array_equal(U[0], np.eye(F)[list(range(d, F)) + list(range(d))])

    for per_source in (False, True):
        del lf.ctx.calls[:]
        got_names, mu, J = coarse.sourcewise_coarse_jacobian_points(lf, b, pts, per_source=per_source, livetime_days=livetime)
        assert [c[0] for c in lf.ctx.calls] == ['set_coarse_binning', 'expected_coarse_jacobian']
        kind, cells, z, scale, ps = lf.ctx.calls[-1]
        assert (cells, ps) == (10, per_source)
        np.testing.assert_array_equal(z, z_want)
        np.testing.assert_array_equal(scale, scale_want)
        assert got_names == lf._parameter_names() and len(got_names) == F
        mu_raw, jac_raw = pattern(3, S, F, 10, per_source)
        if per_source:
            assert mu.shape == (3, S, 2, 5) and J.shape == (3, S, F, 2, 5)
            want = np.einsum('pfk,pskc->psfc', U, jac_raw)
        else:
            assert mu.shape == (3, 2, 5) and J.shape == (3, F, 2, 5)
            want = np.einsum('pfk,pkc->pfc', U, jac_raw)
        np.testing.assert_array_equal(mu.reshape(mu_raw.shape), mu_raw)
        np.testing.assert_array_equal(J.reshape(want.shape), want)            # the chain rule is user_jacobian's
        if per_source:                                                        # ... the same U on every source's block
            np.testing.assert_allclose(J[:, 2], J[:, 0] * 3.0, rtol=1e-15)

        # the one-row form
        del lf.ctx.calls[:]
        one = coarse.sourcewise_coarse_jacobian(lf, b, per_source=per_source, livetime_days=livetime,
                                                **{names[0]: 0.5, 's1_rate_multiplier': 1.25})
        assert [c[0] for c in lf.ctx.calls] == ['set_coarse_binning', 'expected_coarse_jacobian'] and lf.ctx.calls[-1][2].shape == (1, d)
        np.testing.assert_array_equal(lf.ctx.calls[-1][2][0], z_want[2])
        np.testing.assert_array_equal(lf.ctx.calls[-1][3][0], scale_want[2])
        assert one[0] == got_names and one[1].shape == mu.shape[1:] and one[2].shape == J.shape[1:]
        _, _, U1 = user_matrix(lf, {names[0]: np.array([0.5]), 's1_rate_multiplier': np.array([1.25])}, 1, livetime)
        raw1 = pattern(1, S, F, 10, per_source)[1]
        want1 = np.einsum('pfk,pskc->psfc', U1, raw1) if per_source else np.einsum('pfk,pkc->pfc', U1, raw1)
        np.testing.assert_array_equal(one[2].reshape(want1.shape[1:]), want1[0])

    # band and information: one context call each, through propagate_covariance and information_per_cell
    at = {names[0]: 0.5, 's1_rate_multiplier': 1.25}
    del lf.ctx.calls[:]
    all_names, mu1, J1 = coarse.sourcewise_coarse_jacobian(lf, b, livetime_days=livetime, **at)
    del lf.ctx.calls[:]
    floating = ['s1_rate_multiplier', names[0]]
    cov = np.array([[0.04, 0.01], [0.01, 0.09]])
    mu, sigma, impacts = coarse.sourcewise_coarse_band(lf, b, floating, cov, livetime_days=livetime, **at)
    assert [c[0] for c in lf.ctx.calls] == ['set_coarse_binning', 'expected_coarse_jacobian'] and not lf.ctx.calls[-1][4]
    s2, i2 = coarse.propagate_covariance(all_names, J1, floating, cov)
    assert mu.shape == sigma.shape == (2, 5) and list(impacts) == floating
    np.testing.assert_array_equal(mu, mu1)
    np.testing.assert_array_equal(sigma, s2)
    for k in floating:
        np.testing.assert_array_equal(impacts[k], i2[k])
    with pytest.raises(ValueError, match='bogus'):
        coarse.sourcewise_coarse_band(lf, b, ['bogus'], np.eye(1), **at)
    del lf.ctx.calls[:]
    got_names, info, unbounded = coarse.sourcewise_coarse_information(lf, b, livetime_days=livetime, **at)
    assert [c[0] for c in lf.ctx.calls] == ['set_coarse_binning', 'expected_coarse_jacobian']
    assert got_names == all_names and info.shape == (F, F, 2, 5) and unbounded.shape == (F, 2, 5) and unbounded.dtype == bool
    want_info, want_unb = coarse.information_per_cell(J1, mu1)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(unbounded, want_unb)


def test_refusals_reach_no_context_call(recorded, monkeypatch):
    from blueice_amd import coarse
    from blueice_amd.exceptions import NotPreparedException
    from blueice_amd.likelihood import BinnedLogLikelihood
    lf, names, conf = recorded
    b = coarse.CoarseBinning(lf, keep=[])
    n_before = len(lf.ctx.calls)
    calls = {'sourcewise_coarse_jacobian_points': lambda f, x, bb: f(x, bb, {names[0]: np.array([0.1])}),
             'sourcewise_coarse_jacobian': lambda f, x, bb: f(x, bb, **{names[0]: 0.1}),
             'sourcewise_coarse_band': lambda f, x, bb: f(x, bb, [names[0]], np.eye(1), **{names[0]: 0.1}),
             'sourcewise_coarse_information': lambda f, x, bb: f(x, bb, **{names[0]: 0.1})}
    grid = {'sourcewise_coarse_jacobian_points': 'blueice_amd.coarse.expected_coarse_jacobian_points(',
            'sourcewise_coarse_jacobian': 'blueice_amd.coarse.expected_coarse_jacobian(',
            'sourcewise_coarse_band': 'blueice_amd.coarse.expected_coarse_band(',
            'sourcewise_coarse_information': 'blueice_amd.coarse.coarse_information('}
    # a plain binned likelihood: the grid spelling is named (the class alone is looked at: nothing of it is touched)
    plain = object.__new__(BinnedLogLikelihood)
    raw, _, _ = make_lf(monkeypatch, prepare=False)
    for name in NEW:
        f = getattr(coarse, name)
        with pytest.raises(NotImplementedError, match='BinnedLogLikelihood') as e:
            calls[name](f, plain, b)
        assert grid[name] in str(e.value), (name, str(e.value))
        with pytest.raises(TypeError, match='CoarseBinning'):
            calls[name](f, lf, object())
        with pytest.raises(NotPreparedException, match='prepare'):
            calls[name](f, raw, b)
    assert len(lf.ctx.calls) == n_before and raw.ctx is None                # (an unprepared likelihood has no context yet)

    # the four grid-model functions keep refusing a source-wise model, each naming its counterpart; so do the bound names
    old = {'expected_coarse_jacobian_points': lambda: coarse.expected_coarse_jacobian_points(lf, b, {names[0]: np.array([0.1])}),
           'expected_coarse_jacobian': lambda: coarse.expected_coarse_jacobian(lf, b, **{names[0]: 0.1}),
           'expected_coarse_band': lambda: coarse.expected_coarse_band(lf, b, [names[0]], np.eye(1), **{names[0]: 0.1}),
           'coarse_information': lambda: coarse.coarse_information(lf, b, **{names[0]: 0.1})}
    for name, spelling in PINNED.items():
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            old[name]()
        assert spelling in str(e.value), (name, str(e.value))
        assert name in type(lf)._REFUSED
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            getattr(lf, name)(b)
        assert spelling in str(e.value), (name, str(e.value))
    for name in NEW:
        assert not hasattr(type(lf), name)                                   # nothing new is bound on the class
    assert len(lf.ctx.calls) == n_before


def test_header_and_binding_of_the_symbol():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    build.build()
    lib = _capi.load()
    proto = re.search(r'\b%s\s*\(([^)]*)\)' % SYMBOL, text)
    assert proto, "%s is not declared in include/blueice_hip.h" % SYMBOL
    assert hasattr(lib, SYMBOL), "library does not export %s" % SYMBOL
    assert len(_capi.SIGNATURES[SYMBOL][1]) == len([a for a in proto.group(1).split(',') if a.strip()]) == 8
    assert 'tu_sourcewise_coarse_jac' in build.UNITS
    one = np.ones(64)
    p = _capi.ptr
    assert lib.bi_sourcewise_expected_coarse_jacobian(None, 1, p(one), None, 0, p(one.copy()), p(one.copy()), None) == _capi.ERR_INVALID
