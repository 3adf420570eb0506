"""The device Hessian (bi_eval_hess) and what is built on it: against the numpy Hessian oracle (tests/hessian_oracle.py) on
the golden fixtures, its edges and batching, the likelihood classes' values_gradients_hessians (analytic and by gradient
differences), hesse, bestfit_minuit, and the pulls of a toy ensemble."""
import warnings
from collections import OrderedDict

import numpy as np
import pytest

import derivative_oracle as do
import hessian_oracle as ho
import model_zoo
from golden_util import case_names, load_case
from oracle import blueice_oracle as orc

pytestmark = pytest.mark.gpu

BINNED = [n for n in case_names() if load_case(n)['bb_source'] < 0]


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


def binned_ctx(c, sparse=0):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', sparse)
    ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'])
    if c['allow_negative'] and any(c['allow_negative']):
        ctx.set_allow_negative([1 if a else 0 for a in c['allow_negative']])
    ctx.upload_counts(c['counts'])
    return ctx


def unbinned_ctx(c, ps):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    n_ev = c['bins'][0]
    ctx.begin_model(c['model']['anchor_z'], c['S'], n_ev)
    ps = ps.reshape((-1, c['S'], n_ev))
    mus = c['model']['mus'].reshape((-1, c['S']))
    for a in range(len(mus)):
        ctx.set_anchor(a, ps[a], mus[a])
    ctx.end_model()
    ctx.set_unbinned(c['outlier'])
    return ctx


def random_points(c, n, seed, anchors=False):
    rng = np.random.default_rng(seed)
    zs = []
    for _ in range(n):
        z = []
        for g in c['model']['anchor_z']:
            g = np.asarray(g, dtype=float)
            z.append(g[rng.integers(0, len(g))] if anchors else rng.uniform(g[0], g[-1]))
        zs.append(z)
    return np.array(zs, dtype=float).reshape(n, c['d']), rng.uniform(0.4, 1.6, size=(n, c['S']))


def check_against_oracle(ctx, c, zs, rs, H, ll, grad=None, unbinned_model=None):
    for p in range(len(rs)):
        if not np.isfinite(ll[p]):
            assert np.isnan(H[p]).all()
            continue
        if unbinned_model is not None:
            want_ll, want_g, want = ho.hessian_unbinned(unbinned_model, zs[p], rs[p], c['outlier'])
        else:
            want_ll, want_g, want = ho.hessian_binned(c['model'], c['counts'], zs[p], rs[p])
        tol = 1e-9 * max(1.0, np.abs(want).max())
        np.testing.assert_allclose(H[p], want, rtol=0, atol=tol, err_msg='point %d' % p)
        # per entry: within C 2^-52 cond of the exact derivative oracle (the small rate-rate entries included)
        model = unbinned_model if unbinned_model is not None else c['model']
        exact = do.derivatives(model, zs[p], rs[p], counts=None if unbinned_model is not None else c['counts'],
                               unbinned=unbinned_model is not None, outlier=c['outlier'])
        do.check_entries(H[p], exact['hess'], exact['hess_cond'], what='point %d hess' % p)
        do.check_entries(ll[p], exact['ll'], exact['ll_cond'], what='point %d ll' % p)
        if grad is not None:
            do.check_entries(grad[p], exact['grad'], exact['grad_cond'], what='point %d grad' % p)
        assert abs(ll[p] - want_ll) <= 1e-10 * max(1.0, abs(want_ll))
        if grad is not None:
            np.testing.assert_allclose(grad[p], want_g, rtol=0, atol=1e-9 * max(1.0, np.abs(want_g).max()))


@pytest.mark.parametrize('sparse', [0, 2])
@pytest.mark.parametrize('name', BINNED)
def test_bi_eval_hess_matches_the_oracle(name, sparse):
    c = load_case(name)
    ctx = binned_ctx(c, sparse)
    try:
        for anchors in (False, True):
            zs, rs = random_points(c, 6, seed=7 + anchors, anchors=anchors)
            z_arg = zs if c['d'] else None
            ll, gz, gs, H, st = ctx.eval_hess(z_arg, rs)
            ll2, gz2, gs2, st2 = ctx.eval_grad(z_arg, rs)
            assert np.array_equal(st, st2)
            fin = np.isfinite(ll2)
            assert np.array_equal(np.isfinite(ll), fin)
            np.testing.assert_allclose(ll[fin], ll2[fin], rtol=1e-12)
            g, g2 = np.concatenate([gz, gs], axis=1), np.concatenate([gz2, gs2], axis=1)
            np.testing.assert_allclose(g[fin], g2[fin], rtol=1e-12, atol=1e-12 * max(1.0, np.abs(g2[fin]).max(initial=0)))
            assert np.array_equal(H, np.swapaxes(H, 1, 2), equal_nan=True)          # exactly symmetric
            ok = st == 0
            check_against_oracle(ctx, c, zs[ok], rs[ok], H[ok], ll[ok], g[ok])
    finally:
        ctx.close()


def test_bi_eval_hess_edges_out_of_bounds_and_unphysical():
    from blueice_amd import _capi
    c = load_case('d2_nonuniform')
    ctx = binned_ctx(c)
    try:
        zs, rs = random_points(c, 4, seed=3)
        zs[0, 0] = c['model']['anchor_z'][0][-1] + 0.5            # out of the box
        rs[1, 2] = -0.5                                           # unphysical rate
        ll, _, _, H, st = ctx.eval_hess(zs, rs)
        _, st_eval = ctx.eval(zs, rs)
        assert np.array_equal(st, st_eval)
        assert st[0] & _capi.ST_OUT_OF_BOUNDS and st[1] & _capi.ST_UNPHYSICAL
        assert ll[0] == -np.inf and ll[1] == -np.inf
        assert np.isnan(H[:2]).all() and np.isfinite(H[2:]).all()
    finally:
        ctx.close()


@pytest.mark.parametrize('name', ['edge_mu_zero_hit', 'edge_mu_zero_ok'])
def test_bi_eval_hess_where_mu_is_zero(name):
    c = load_case(name)
    ctx = binned_ctx(c)
    try:
        n = len(c['call_ll'])
        zs = np.asarray(c['call_z'], dtype=float).reshape(n, c['d'])
        rs = np.array([np.asarray(c['call_mult'][j], dtype=float) for j in range(n)])
        ll, _, _, H, st = ctx.eval_hess(zs, rs)
        ref, _ = ctx.eval(zs, rs)
        np.testing.assert_allclose(ll, ref, rtol=1e-12)
        if name == 'edge_mu_zero_hit':
            assert np.any(ll == -np.inf)
        else:
            assert np.isfinite(ll).any()
        assert np.isnan(H[~np.isfinite(ll)]).all() and np.isfinite(H[np.isfinite(ll)]).all()
        ok = st == 0
        check_against_oracle(ctx, c, zs[ok], rs[ok], H[ok], ll[ok])
    finally:
        ctx.close()


@pytest.mark.parametrize('clamp', [False, True])
@pytest.mark.parametrize('name', ['unb_shape_2src', 'unb_d0_three_sources'])
def test_bi_eval_hess_unbinned(name, clamp):
    c = load_case(name)
    ps = np.array(c['model']['ps'], dtype=float)
    if clamp:                     # events 0 and 3 have density 0 at every anchor: they sit on the outlier clamp
        ps[..., 0] = 0.0
        ps[..., 3] = 0.0
    model = dict(c['model'], ps=ps)
    ctx = unbinned_ctx(c, ps)
    try:
        zs, rs = random_points(c, 5, seed=9)
        z_arg = zs if c['d'] else None
        ll, gz, gs, H, st = ctx.eval_hess(z_arg, rs)
        ll2, gz2, gs2, _ = ctx.eval_grad(z_arg, rs)
        np.testing.assert_allclose(ll, ll2, rtol=1e-12)
        np.testing.assert_allclose(np.concatenate([gz, gs], 1), np.concatenate([gz2, gs2], 1), rtol=1e-11, atol=1e-11)
        assert np.array_equal(H, np.swapaxes(H, 1, 2))
        check_against_oracle(ctx, c, zs, rs, H, ll, np.concatenate([gz, gs], 1), unbinned_model=model)
    finally:
        ctx.close()


@pytest.mark.parametrize('P', [1, 7, 300, 70000])
def test_bi_eval_hess_batches_over_datasets(P):
    """P points over four datasets (P = 70 000 crosses the 65 535-item launch chunk): equal to the same points one dataset at
    a time, and a sample equal to the oracle."""
    c = load_case('d2_nonuniform')
    rng = np.random.default_rng(P)
    T = 4
    counts = np.stack([c['counts']] + [rng.poisson(c['counts'] + 1.0) for _ in range(T - 1)]).astype(float)
    ctx = binned_ctx(dict(c, counts=counts))
    try:
        zs, rs = random_points(c, P, seed=P)
        ds = rng.integers(0, T, size=P)
        ll, gz, gs, H, st = ctx.eval_hess(zs, rs, ds)
        assert not st.any() and H.shape == (P, 5, 5)
        ll2, gz2, gs2, _ = ctx.eval_grad(zs, rs, ds)
        np.testing.assert_allclose(ll, ll2, rtol=1e-12)
        for p in rng.choice(P, size=min(P, 25), replace=False):
            _, _, want = ho.hessian_binned(c['model'], counts[ds[p]], zs[p], rs[p])
            np.testing.assert_allclose(H[p], want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
    finally:
        ctx.close()


def test_device_toys_give_the_hessians_of_their_uploaded_counts(ns):
    lf = model_zoo.fit_c1_like(ns)
    T = 64
    lf.simulate_toys(T, seed=3, s0_rate_multiplier=1.1, shift=0.2)
    rng = np.random.default_rng(1)
    points = dict(s0_rate_multiplier=rng.uniform(0.8, 1.3, T), s1_rate_multiplier=rng.uniform(0.8, 1.3, T),
                  shift=rng.uniform(-0.9, 0.9, T))
    ll, grads, names, H = lf.values_gradients_hessians(points, dataset=np.arange(T))
    assert lf.hessian_method == 'analytic'
    stack = np.stack([lf.ctx.download_counts(t) for t in range(T)]).reshape((T,) + tuple(lf.bin_shape))
    lf.set_binned_data(stack)
    ll2, grads2, names2, H2 = lf.values_gradients_hessians(points, dataset=np.arange(T))
    assert names == names2
    np.testing.assert_allclose(ll, ll2, rtol=1e-11)
    np.testing.assert_allclose(H, H2, rtol=1e-9, atol=1e-9 * np.abs(H2).max())


# ---- the likelihood classes --------------------------------------------------------------------------------------

def gradient_differences(lf, kw, names, h=1e-5, **options):
    """Central differences of values_and_gradients (the analytic gradient) around one point."""
    F = len(names)
    H = np.zeros((F, F))
    for j, n in enumerate(names):
        step = h * max(1.0, abs(kw[n]))
        up, dn = dict(kw), dict(kw)
        up[n] += step
        dn[n] -= step
        _, gu = lf.values_and_gradients({k: np.array([v]) for k, v in up.items()}, **options)
        _, gd = lf.values_and_gradients({k: np.array([v]) for k, v in dn.items()}, **options)
        H[j] = [(gu[m][0] - gd[m][0]) / (2 * step) for m in names]
    return 0.5 * (H + H.T)


def test_values_gradients_hessians_with_efficiency_prior_and_livetime(ns):
    lf, _, _ = model_zoo.efficiency_param(ns)
    lf.pdf_base_config['livetime_days'] = 1.0          # (the sources' default live-time: what livetime_days scales from)
    lf.rate_parameters['a'] = lambda x: -0.5 * ((np.asarray(x) - 1.0) / 0.3) ** 2
    anchors, _, base = lf.shape_parameters['shift']
    lf.shape_parameters['shift'] = (anchors, lambda x: -np.asarray(x) ** 2, base)
    kw = dict(eff=1.2, shift=0.3, a_rate_multiplier=0.9, b_rate_multiplier=1.4, c_rate_multiplier=0.6)
    for lt in (None, 2.5):
        ll, grads, names, H = lf.values_gradients_hessians({k: np.array([v]) for k, v in kw.items()}, livetime_days=lt)
        assert names == ['a_rate_multiplier', 'b_rate_multiplier', 'c_rate_multiplier', 'shift', 'eff']
        assert lf.hessian_method == 'analytic' and lf.supports_hessian
        assert abs(ll[0] - lf(livetime_days=lt, **kw)) <= 1e-11 * abs(ll[0])
        ll_g, g = lf.values_and_gradients({k: np.array([v]) for k, v in kw.items()}, livetime_days=lt)
        for n in names:
            assert abs(grads[n][0] - g[n][0]) <= 1e-9 * max(1.0, abs(g[n][0])), n
        want = gradient_differences(lf, kw, names, livetime_days=lt)
        np.testing.assert_allclose(H[0], want, rtol=0, atol=1e-6 * np.abs(want).max())
        v, g1, n1, H1 = lf.value_gradient_hessian(livetime_days=lt, **kw)
        assert v == ll[0] and n1 == names and np.array_equal(H1, H[0])


def test_sum_of_likelihoods_adds_the_hessians(ns):
    lf1, _, _ = model_zoo.efficiency_param(ns)
    lf2, _, _ = model_zoo.efficiency_param(ns)
    lf2.set_data(lf2.base_model.simulate())
    total = ns.LogLikelihoodSum([lf1, lf2], likelihood_weights=[1.0, 0.5])
    kw = dict(eff=0.9, shift=-0.4, a_rate_multiplier=1.1, b_rate_multiplier=0.8, c_rate_multiplier=1.3)
    pts = {k: np.array([v, v * 0.95]) for k, v in kw.items()}
    ll, grads, names, H = total.values_gradients_hessians(pts)
    l1, _, n1, H1 = lf1.values_gradients_hessians(pts)
    l2, _, n2, H2 = lf2.values_gradients_hessians(pts)
    assert names == n1 == n2 and total.hessian_method == 'analytic'
    np.testing.assert_allclose(ll, l1 + 0.5 * l2, rtol=1e-13)
    np.testing.assert_allclose(H, H1 + 0.5 * H2, rtol=1e-13)


@pytest.mark.parametrize('name', ['ref_bb_multi_bin', 'bb_d2', 'unb_nan_pdf'])
def test_fallback_by_gradient_differences(ns, name):
    lf, _, _ = model_zoo.CASES[name](ns) if name in model_zoo.CASES else model_zoo.UNBINNED_CASES[name](ns)
    assert not lf.supports_hessian
    names = ['%s_rate_multiplier' % s for s in lf.source_name_list if s in lf.rate_parameters] + list(lf.shape_parameters)
    c = load_case(name)
    if name == 'unb_nan_pdf':
        kw = dict(sigma=1.3, a_rate_multiplier=1.2, b_rate_multiplier=0.9, c_rate_multiplier=1.1)
    elif name == 'bb_d2':
        kw = dict(shift=0.4, stretch=0.6)
    else:
        kw = {}
    if not names:                                   # a likelihood without parameters: give it one to differentiate
        lf.add_rate_parameter('s0')
        names = ['s0_rate_multiplier']
        kw = dict(s0_rate_multiplier=1.1)
    names = [n for n in names]
    pts = {n: np.array([kw.get(n, 1.0 if n.endswith('_rate_multiplier') else lf.pdf_base_config[n])]) for n in names}
    ll, grads, out_names, H = lf.values_gradients_hessians(pts)
    assert lf.hessian_method == 'gradient-differences' and out_names == names
    assert np.isfinite(H).all() and np.array_equal(H[0], H[0].T)
    # against central second differences of the oracle on the golden tensors (Beeston-Barlow: forgiving U = 0 bins, as the
    # gradient tests do) or of the likelihood itself, inside the point's cell
    x = np.array([pts[n][0] for n in names])
    if name == 'unb_nan_pdf':
        f = lambda v: lf(**dict(zip(names, v)))
    else:
        shapes = [j for j, n in enumerate(names) if n in lf.shape_parameters]
        rates = {n: j for j, n in enumerate(names) if n.endswith('_rate_multiplier')}

        def f(v):
            rs = np.array([v[rates[s + '_rate_multiplier']] if s + '_rate_multiplier' in rates else 1.0 for s in lf.source_name_list])
            return orc.loglikelihood(c['model'], c['counts'], v[shapes], rs, bb_source=c['bb_source'], forgive_zero_u=True)
    h = 1e-3 * np.maximum(1.0, np.abs(x))
    for j, n in enumerate(names):
        if n in lf.shape_parameters:
            grid = np.array(sorted(lf.shape_parameters[n][0]), dtype=float)
            lo_hi = ho.cell_of(grid, x[j])
            h[j] = 1e-3 * (lo_hi[1] - lo_hi[0])
    want = ho.second_differences(f, x, None, None, h)
    np.testing.assert_allclose(H[0], want, rtol=0, atol=1e-5 * np.abs(want).max())


# ---- hesse / bestfit_minuit ---------------------------------------------------------------------------------------

def _mc_source_class(ns):
    """GaussianMCSource (a binned pdf from its own Monte Carlo) with GaussianSource's rate settings some_multiplier and
    strlen_multiplier, so that the reference's shape parameters act on a binned likelihood too."""
    class GaussianMCWithMultipliers(ns.GaussianMCSource):
        def compute_pdf(self):
            self.events_per_day = self.events_per_day * self.config.get('some_multiplier', 1) * \
                len(self.config.get('strlen_multiplier', 'x'))
            super().compute_pdf()
    return GaussianMCWithMultipliers


def _conf_lf(ns, cls, rate=False, shape=None, strlen=False):
    conf = ns.conf_for_test(events_per_day=1000.)
    if cls == 'binned':
        conf['default_source_class'] = _mc_source_class(ns)
        conf['n_events_for_pdf'] = int(2e5)
        lf = ns.BinnedLogLikelihood(conf)
    else:
        lf = ns.UnbinnedLogLikelihood(conf)
    if rate:
        lf.add_rate_parameter('s0')
    if shape:
        lf.add_shape_parameter('some_multiplier', (0.5, 1, 1.5, 2))
    if strlen:
        lf.add_shape_parameter('strlen_multiplier', {1: 'x', 2: 'hi', 3: 'wha'}, base_value=1)
    lf.prepare()
    np.random.seed(1)
    lf.set_data(lf.base_model.simulate())
    return lf


@pytest.mark.parametrize('cls', ['unbinned', 'binned'])
def test_bestfit_minuit_restates_the_reference_test(ns, cls):
    from blueice_amd.inference import bestfit_device, bestfit_minuit
    # single rate parameter
    lf = _conf_lf(ns, cls, rate=True)
    fit, ll = bestfit_minuit(lf)
    assert isinstance(fit, dict) and 's0_rate_multiplier' in fit
    assert np.isfinite(fit['s0_rate_multiplier_error']) and fit['s0_rate_multiplier_error'] > 0
    best, ll_dev = bestfit_device(lf)
    assert fit['s0_rate_multiplier'] == best['s0_rate_multiplier'] and ll == ll_dev
    # the Poisson error of a rate-only fit: sqrt(N) / mu per unit multiplier
    assert abs(fit['s0_rate_multiplier_error'] - np.sqrt(fit['s0_rate_multiplier'] * 1000.) / 1000.) < 0.05 * fit['s0_rate_multiplier_error']
    # don't fit
    res, ll = bestfit_minuit(lf, s0_rate_multiplier=1)
    assert len(res) == 0 and ll == lf(s0_rate_multiplier=1)
    # display options are accepted and ignored
    fit2, _ = bestfit_minuit(lf, minimize_kwargs=dict(print_level=0, pedantic=False, errordef=0.5))
    assert fit2 == fit
    # single shape parameter
    lf = _conf_lf(ns, cls, shape=True)
    fit, ll = bestfit_minuit(lf)
    assert 'some_multiplier' in fit and np.isfinite(fit['some_multiplier_error']) and fit['some_multiplier_error'] > 0
    # shape and rate parameter
    lf = _conf_lf(ns, cls, rate=True, shape=True)
    fit, ll = bestfit_minuit(lf)
    assert 'some_multiplier' in fit and 's0_rate_multiplier' in fit
    best, ll_dev = bestfit_device(lf)
    for k, v in best.items():
        assert fit[k] == v
    # rate and rate-like shape parameter are degenerate here: -H is singular or nearly so; whatever comes back is nan or
    # positive, never a negative error
    for k in ('some_multiplier_error', 's0_rate_multiplier_error'):
        assert np.isnan(fit[k]) or fit[k] > 0
    # non-numeric shape parameter
    lf = _conf_lf(ns, cls, strlen=True)
    fit, ll = bestfit_minuit(lf)
    assert 'strlen_multiplier' in fit and 'strlen_multiplier_error' in fit
    assert np.isfinite(fit['strlen_multiplier_error']) and fit['strlen_multiplier_error'] > 0


def test_bestfit_minuit_log_space_rates(ns):
    from blueice_amd.inference import bestfit_minuit
    lf = _conf_lf(ns, 'binned', rate=True)
    fit, ll = bestfit_minuit(lf)
    fit_log, ll_log = bestfit_minuit(lf, rates_in_log_space=True)
    m, e = fit['s0_rate_multiplier'], fit['s0_rate_multiplier_error']
    assert abs(fit_log['s0_rate_multiplier'] - np.log10(m)) < 1e-12
    assert abs(fit_log['s0_rate_multiplier_error'] - e / (m * np.log(10))) < 1e-3 * fit_log['s0_rate_multiplier_error']


def test_hesse_scalar_and_ensemble_and_not_positive_definite(ns):
    from blueice_amd.inference import hesse
    lf = model_zoo.fit_c1_like(ns)
    best, ll = lf.bestfit_device()
    names, cov = hesse(lf, best)
    assert names == list(best) and cov.shape == (3, 3)
    assert np.all(np.linalg.eigvalsh(cov) > 0)
    pts = {k: np.array([v, v]) for k, v in best.items()}
    names2, cov2 = hesse(lf, pts)
    assert cov2.shape == (2, 3, 3)
    np.testing.assert_allclose(cov2[0], cov, rtol=1e-12)
    # far from the maximum -H need not be positive definite: nan, one warning
    bad = dict(best)
    bad['s0_rate_multiplier'] = 40.0
    bad['s1_rate_multiplier'] = 0.0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        _, cov3 = hesse(lf, {k: np.array([best[k], bad[k]]) for k in best})
    assert np.isfinite(cov3[0]).all()
    if not np.isfinite(cov3[1]).all():
        assert np.isnan(cov3[1]).all() and len(rec) == 1


def _rate_only_binned(ns):
    conf = ns.conf_for_test(n_sources=2, mc=True, n_events_for_pdf=int(2e5))
    conf['sources'] = [dict(name='s0', mu=-1.0, sigma=1.0, events_per_day=2000.),
                       dict(name='s1', mu=1.5, sigma=2.0, events_per_day=1500.)]
    lf = ns.BinnedLogLikelihood(conf)
    lf.add_rate_parameter('s0')
    lf.add_rate_parameter('s1')
    lf.prepare()
    lf.set_data(lf.base_model.simulate())
    return lf


def test_pulls_of_a_toy_ensemble(ns):
    """2048 toys drawn at the truth and fitted 256 at a time (the loop of toy_mc_fits), with hesse over each chunk's toys in
    one device call: (fit - truth) / error is standard normal."""
    from blueice_amd.inference import bestfit_toys, hesse
    lf = _rate_only_binned(ns)
    pulls = []
    try:
        for t0 in range(0, 2048, 256):
            lf.ctx.set_param('toy_offset', t0)
            lf.simulate_toys(256, seed=17)
            best, ll = bestfit_toys(lf)
            names, cov = hesse(lf, best, datasets=np.arange(256))
            assert cov.shape == (256, 2, 2) and np.isfinite(cov).all()
            err = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
            pulls.append((np.stack([best[n] for n in names], axis=1) - 1.0) / err)
    finally:
        lf.ctx.set_param('toy_offset', 0)
    pulls = np.concatenate(pulls)
    for j in range(2):
        assert abs(pulls[:, j].mean()) < 0.1, pulls[:, j].mean()
        assert 0.9 <= pulls[:, j].std() <= 1.1, pulls[:, j].std()
