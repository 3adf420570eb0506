"""Hessian of the likelihood, the host-side pieces (no GPU): the numpy Hessian oracle against second differences of the CPU
oracle, the chain rule from (z, rate_scale) to the user's parameters against finite differences, and the public surface
(bi_eval_hess bound, hesse / bestfit_minuit methods of every likelihood class)."""
import numpy as np
import pytest

import hessian_oracle as ho
from golden_util import load_case
from oracle import blueice_oracle as orc


def interior_points(case, n, seed):
    """Points strictly inside a random grid cell of every axis (at least a fifth of the cell from its faces)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        z = []
        for g in case['model']['anchor_z']:
            g = np.asarray(g, dtype=float)
            if len(g) < 2:
                z.append(g[0])
                continue
            k = rng.integers(0, len(g) - 1)
            z.append(g[k] + rng.uniform(0.2, 0.8) * (g[k + 1] - g[k]))
        out.append(np.array(z))
    return out


@pytest.mark.parametrize('name', ['c1_like', 'd2_nonuniform', 'd3_small', 'd0_multi_source', 'unb_shape_2src'])
def test_oracle_hessian_matches_second_differences(name):
    c = load_case(name)
    model, d, S = c['model'], c['d'], c['S']
    unb = name.startswith('unb_')
    rng = np.random.default_rng(11)
    for z in interior_points(c, 4, seed=5):
        rs = rng.uniform(0.5, 1.5, S)
        if unb:
            ll, g, H = ho.hessian_unbinned(model, z, rs, c['outlier'])
            f = lambda x: orc.loglikelihood_unbinned(model, x[:d], x[d:], c['outlier'])
        else:
            ll, g, H = ho.hessian_binned(model, c['counts'], z, rs)
            f = lambda x: orc.loglikelihood(model, c['counts'], x[:d], x[d:])
        x = np.concatenate([z, rs])
        assert ll == f(x)
        h = np.zeros(d + S)
        for i, gr in enumerate(model['anchor_z']):
            lo_hi = ho.cell_of(gr, z[i])
            h[i] = 0.0 if lo_hi is None else 1e-3 * (lo_hi[1] - lo_hi[0])
        h[d:] = 1e-3 * np.maximum(1.0, rs)
        want = ho.second_differences(f, x, None, None, h)
        scale = np.abs(want).max()
        assert scale > 0
        np.testing.assert_allclose(H, want, rtol=0, atol=1e-5 * scale)
        assert np.array_equal(H, H.T) or np.allclose(H, H.T, rtol=1e-13, atol=1e-13 * scale)
        # the gradient too, by first differences (a cheap consistency check of the same derivative columns)
        gd = np.array([(f(x + e) - f(x - e)) / (2 * e.sum()) if e.sum() else 0.0 for e in np.diag(h)])
        np.testing.assert_allclose(g, gd, rtol=0, atol=1e-5 * max(1.0, np.abs(gd).max()))


def test_oracle_hessian_on_an_anchor_is_the_assigned_cell():
    """On an interior anchor the oracle takes the cell above (g[k] <= z < g[k+1]); one-sided second differences into that
    cell agree with it."""
    c = load_case('c1_like')
    model = c['model']
    g = np.asarray(model['anchor_z'][0], dtype=float)
    z = np.array([g[1]])
    rs = np.array([0.9, 1.2])
    _, _, H = ho.hessian_binned(model, c['counts'], z, rs)
    h = 1e-3 * (g[2] - g[1])
    f = lambda t: orc.loglikelihood(model, c['counts'], np.array([t]), rs)
    fwd = (2 * f(z[0]) - 5 * f(z[0] + h) + 4 * f(z[0] + 2 * h) - f(z[0] + 3 * h)) / h ** 2
    assert abs(H[0, 0] - fwd) <= 1e-4 * max(1.0, abs(fwd))


# ---- the chain rule ------------------------------------------------------------------------------------------------

def _theta_function(d, S, seed):
    """A smooth test function of theta = (z [d], rate_scale [S]) with its exact gradient and Hessian."""
    rng = np.random.default_rng(seed)
    F = d + S
    A = rng.normal(size=(F, F))
    A = A + A.T
    b = rng.normal(size=F)
    c3 = rng.normal(size=F) * 0.1

    def f(t):
        return float(b @ t + 0.5 * t @ A @ t + np.sum(c3 * t ** 3))

    def grad(t):
        return b + A @ t + 3 * c3 * t ** 2

    def hess(t):
        return A + np.diag(6 * c3 * t)
    return f, grad, hess


def test_chain_rule_matches_finite_differences():
    """Two shape parameters (the second is also the efficiency of sources 0 and 2), three sources of which 0 and 1 have rate
    multipliers, a live-time factor, priors on a rate multiplier and a shape parameter, and the same in log10 rates."""
    from blueice_amd.hessian import chain_rule_hessian, prior_derivatives, to_log10
    d, S = 2, 3
    f, grad, hess = _theta_function(d, S, seed=4)
    L = 1.7
    eff_axis = [1, -1, 1]
    rate_sources = [0, 1]
    m_fixed = np.array([1.0, 1.0, 0.8])             # source 2 has no rate parameter: its multiplier stays fixed
    prior_m0 = lambda x: -0.5 * ((np.asarray(x) - 1.0) / 0.3) ** 2
    prior_x0 = lambda x: np.log(1.0 + np.asarray(x) ** 2)

    def theta_of(u):
        m = m_fixed.copy()
        m[0], m[1] = u[0], u[1]
        x = u[2:]
        eff = np.array([x[1], 1.0, x[1]])
        return np.concatenate([x, m * L * eff])

    def user_ll(u):
        return f(theta_of(u)) + prior_m0(u[0]) + prior_x0(u[2])

    u = np.array([1.3, 0.7, 0.4, 0.9])
    t = theta_of(u)
    gth = grad(t)
    mult = m_fixed.copy()
    mult[0], mult[1] = u[0], u[1]
    eff = np.array([[u[3], 1.0, u[3]]])
    pg, ph = np.zeros((1, 4)), np.zeros((1, 4))
    pg[0, 0], ph[0, 0] = (v[0] for v in prior_derivatives(prior_m0, np.array([u[0]])))
    pg[0, 2], ph[0, 2] = (v[0] for v in prior_derivatives(prior_x0, np.array([u[2]])))
    g, H = chain_rule_hessian(gth[None, :d], gth[None, d:], hess(t)[None], mult[None], L, eff, eff_axis, rate_sources, pg, ph)
    h = 1e-4 * np.ones(4)
    want_H = ho.second_differences(user_ll, u, None, None, h)
    want_g = np.array([(user_ll(u + e) - user_ll(u - e)) / (2 * e.sum()) for e in np.diag(h)])
    np.testing.assert_allclose(g[0], want_g, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(H[0], want_H, rtol=1e-5, atol=1e-5 * np.abs(want_H).max())
    assert np.allclose(H[0], H[0].T)

    # log10 rate multipliers: y_j = log10(m_j) for the two rate parameters
    def user_ll_log(y):
        v = y.copy()
        v[:2] = 10.0 ** y[:2]
        return user_ll(v)
    y = u.copy()
    y[:2] = np.log10(u[:2])
    g2, H2 = to_log10(g, H, u[None], [True, True, False, False])
    want_H2 = ho.second_differences(user_ll_log, y, None, None, h)
    want_g2 = np.array([(user_ll_log(y + e) - user_ll_log(y - e)) / (2 * e.sum()) for e in np.diag(h)])
    np.testing.assert_allclose(g2[0], want_g2, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(H2[0], want_H2, rtol=1e-5, atol=1e-5 * np.abs(want_H2).max())


def test_difference_steps_stay_in_the_cell():
    from blueice_amd.hessian import difference_steps
    x = np.array([0.5, 1.0, 0.0, 1.999999, 2.0])
    lo = np.array([0.0, 1.0, 0.0, 1.0, 1.0])
    hi = np.array([1.0, 2.0, 1.0, 2.0, 2.0])
    last = np.array([False, False, False, False, True])
    xp, xm = difference_steps(x, lo, hi, last, 1e-3)
    np.testing.assert_allclose(xp, [0.501, 1.001, 0.001, 1.999999, 2.0])       # below an interior edge: one-sided
    np.testing.assert_allclose(xm, [0.499, 1.0, 0.0, 1.998999, 1.999])
    assert np.all(xp >= xm) and np.all(xp - xm > 0)


# ---- the public surface --------------------------------------------------------------------------------------------

def test_hesse_and_bestfit_minuit_are_likelihood_methods():
    from blueice_amd import inference
    from blueice_amd.likelihood import BinnedLogLikelihood, LogLikelihoodSum, UnbinnedLogLikelihood
    assert 'hesse' in inference.__all__ and 'bestfit_minuit' in inference.__all__
    for cls in (BinnedLogLikelihood, UnbinnedLogLikelihood, LogLikelihoodSum):
        assert cls.hesse is inference.hesse
        assert cls.bestfit_minuit is inference.bestfit_minuit
    for cls in (BinnedLogLikelihood, UnbinnedLogLikelihood, LogLikelihoodSum):
        for attr in ('values_gradients_hessians', 'supports_hessian', 'hessian_method'):
            assert hasattr(cls, attr), (cls.__name__, attr)
    assert hasattr(BinnedLogLikelihood, 'value_gradient_hessian')


def test_bi_eval_hess_is_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from blueice_amd import _capi, build
    header = open(build.HDR).read()
    assert re.search(r'\bint bi_eval_hess\(bi_ctx\* ctx, int64_t P,', header)
    assert 'bi_eval_hess' in _capi.SIGNATURES
    restype, args = _capi.SIGNATURES['bi_eval_hess']
    assert len(args) == 9
    if os.path.exists(build.OUT):
        assert hasattr(ctypes.CDLL(build.OUT), 'bi_eval_hess')


def test_bestfit_minuit_rejects_unknown_minimize_kwargs():
    from blueice_amd.inference import bestfit_minuit
    with pytest.raises(ValueError):
        bestfit_minuit(object(), minimize_kwargs={'tol': 1e-3})
