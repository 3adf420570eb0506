"""Host side of the derivatives of coarse views, no device: the linear propagation of a covariance to the cells against a
brute-force double loop, its refusals and nan, the per-cell information formula with a cell that expects nothing, the new
symbol in the header and in the binding, and the refusals of the new methods where there are no bins."""
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import model_zoo
from blueice_amd import _capi, coarse, inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_METHODS = ('expected_coarse_jacobian', 'expected_coarse_jacobian_points', 'expected_coarse_band', 'coarse_information')


def test_propagation_against_a_double_loop():
    """sigma_C^2 = sum_kl J_kC cov_kl J_lC over the NAMED parameters only, in the covariance's own order (not the Jacobian's),
    cells of any shape; impacts J_k sqrt(cov_kk), signed."""
    rng = np.random.default_rng(3)
    all_names = ['a', 'b', 'c', 'd', 'e']
    J = rng.normal(size=(5, 4, 3))
    use = ['d', 'a', 'c']                                   # a subset, in another order
    A = rng.normal(size=(3, 3))
    cov = A @ A.T + 0.1 * np.eye(3)
    sigma, impacts = coarse.propagate_covariance(all_names, J, use, cov)
    assert sigma.shape == (4, 3) and isinstance(impacts, OrderedDict) and list(impacts) == use
    rows = [all_names.index(k) for k in use]
    for i in range(4):
        for j in range(3):
            var = 0.0
            for k in range(3):
                for l in range(3):
                    var += J[rows[k], i, j] * cov[k, l] * J[rows[l], i, j]
            assert abs(sigma[i, j] - np.sqrt(var)) <= 1e-13 * np.sqrt(var)
    for k, name in enumerate(use):
        np.testing.assert_array_equal(impacts[name], J[rows[k]] * np.sqrt(cov[k, k]))
    # a diagonal covariance: the impacts add in quadrature
    sigma, impacts = coarse.propagate_covariance(all_names, J, use, np.diag([0.5, 2.0, 0.25]))
    np.testing.assert_allclose(sigma, np.sqrt(sum(v ** 2 for v in impacts.values())), rtol=1e-14)
    # one cell (a signal box), and no floating parameter at all
    sigma, impacts = coarse.propagate_covariance(all_names, J[:, 0, 0], ['b'], [[4.0]])
    assert sigma.shape == () and sigma == abs(J[1, 0, 0]) * 2.0 and impacts['b'] == J[1, 0, 0] * 2.0
    sigma, impacts = coarse.propagate_covariance(all_names, J, [], np.zeros((0, 0)))
    assert sigma.shape == (4, 3) and np.all(sigma == 0.0) and not impacts


def test_propagation_refuses_unknown_names_and_keeps_nan():
    J = np.arange(6.0).reshape(2, 3) + 1.0
    with pytest.raises(ValueError, match='bogus'):
        coarse.propagate_covariance(['a', 'b'], J, ['a', 'bogus'], np.eye(2))
    with pytest.raises(ValueError, match='twice'):
        coarse.propagate_covariance(['a', 'b'], J, ['a', 'a'], np.eye(2))
    with pytest.raises(ValueError, match='covariance'):
        coarse.propagate_covariance(['a', 'b'], J, ['a', 'b'], np.eye(3))
    sigma, impacts = coarse.propagate_covariance(['a', 'b'], J, ['a', 'b'], np.full((2, 2), np.nan))
    assert np.isnan(sigma).all() and all(np.isnan(v).all() for v in impacts.values())
    # a nan Jacobian (a point outside the anchor box) gives a nan band too
    sigma, _ = coarse.propagate_covariance(['a', 'b'], np.full((2, 3), np.nan), ['a', 'b'], np.eye(2))
    assert np.isnan(sigma).all()


def test_information_per_cell_with_a_cell_that_expects_nothing():
    """I_C = J_C J_C^T / mu_C; mu_C = 0 contributes 0 and flags the parameters that move the cell; a negative or nan mu_C is nan."""
    J = np.array([[1.0, 0.0, 2.0, 1.0, 1.0],
                  [3.0, 0.0, 0.0, 1.0, 1.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0]])
    mu = np.array([2.0, 0.0, 0.0, -1.0, np.nan])
    info, unbounded = coarse.information_per_cell(J, mu)
    assert info.shape == (3, 3, 5) and unbounded.shape == (3, 5) and unbounded.dtype == bool
    np.testing.assert_array_equal(info[:, :, 0], np.outer(J[:, 0], J[:, 0]) / 2.0)
    assert np.all(info[:, :, 1] == 0.0) and np.all(info[:, :, 2] == 0.0)
    assert np.isnan(info[:, :, 3]).all() and np.isnan(info[:, :, 4]).all()
    assert unbounded.tolist() == [[False, False, True, False, False], [False] * 5, [False] * 5]
    # cells of any shape
    info2, unb2 = coarse.information_per_cell(J[:, :4].reshape(3, 2, 2), mu[:4].reshape(2, 2))
    assert info2.shape == (3, 3, 2, 2) and unb2.shape == (3, 2, 2)
    np.testing.assert_array_equal(info2.reshape(3, 3, 4), info[:, :, :4])
    # a counting experiment: one cell, mu = s m + b -> I_mm = s^2 / (s m + b)
    s, b = 7.0, 12.0
    info, _ = coarse.information_per_cell(np.array([s]), np.array(s + b))
    assert info.shape == (1, 1) and info[0, 0] == s * s / (s + b)


def test_header_and_binding_agree_on_the_new_symbol():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+bi_expected_coarse_jacobian\s*\(([^)]*)\)\s*;', text)
    assert m, "include/blueice_hip.h does not declare bi_expected_coarse_jacobian"
    args = [a.strip() for a in m.group(1).split(',') if a.strip()]
    assert len(args) == 7 and args[0].startswith('bi_ctx') and args[-1].startswith('int32_t')
    assert 'bi_expected_coarse_jacobian' in _capi.SIGNATURES
    restype, argtypes = _capi.SIGNATURES['bi_expected_coarse_jacobian']
    assert len(argtypes) == len(args) and restype is _capi.SIGNATURES['bi_expected_coarse'][0]
    from blueice_amd.device import DeviceContext
    assert callable(DeviceContext.expected_coarse_jacobian)


def test_names_are_public_and_methods():
    from blueice_amd.likelihood import BinnedLogLikelihood
    for name in NEW_METHODS:
        assert name in inference.__all__ and name in coarse.__all__
        assert getattr(BinnedLogLikelihood, name) is getattr(inference, name) is getattr(coarse, name)


def test_refused_where_there_are_no_bins():
    """A source-wise model, an unbinned likelihood, a sum and Beeston-Barlow: NotImplementedError from every new method,
    whatever the binning, before any device is touched."""
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    ns = model_zoo.namespace_of('blueice_amd')
    plain = ns.BinnedLogLikelihood(ns.conf_for_test(events_per_day=1, analysis_space=[['x', np.linspace(-5, 5, 11)]]))
    b = coarse.CoarseBinning(plain, rebin=dict(x=2))
    conf, _, _ = many_nuisances_config(n_bins=(4, 4))
    source_wise = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    unbinned = ns.UnbinnedLogLikelihood(ns.conf_for_test(events_per_day=1))
    anc = ns.LogAncillaryLikelihood(lambda values: 0.0, ['nuisance'], config=dict(nuisance=0.5))
    total = ns.LogLikelihoodSum([unbinned, anc])
    data, _ = ns.make_data([dict(n_events=32, x=0.5)])
    bb = ns.BinnedLogLikelihood(ns.conf_for_test(default_source_class=ns.FixedSampleSource, events_per_day=32 / 5,
                                                 analysis_space=[['x', [0, 1]]], data=data),
                                likelihood_config=dict(model_zoo.BB_LC))
    for lf in (source_wise, unbinned, total, bb):
        for call in (lambda o: o.expected_coarse_jacobian(b), lambda o: o.expected_coarse_jacobian_points(b, {}),
                     lambda o: o.expected_coarse_band(b, ['s0_rate_multiplier'], np.eye(1)), lambda o: o.coarse_information(b)):
            with pytest.raises(NotImplementedError):
                call(lf)
        assert getattr(lf, 'ctx', None) is None
    assert getattr(plain, 'ctx', None) is None            # making a binning touches no device either
