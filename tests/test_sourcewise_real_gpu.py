"""Real-valued data of source-wise models on the device: bi_eval_sourcewise_real against real_counts_oracle.point on the expanded
grid at every case of sourcewise_toy_cases, the Asimov sets of bi_sourcewise_set_asimov_counts against
bi_sourcewise_expected_counts bit for bit and exact zeros at their truths, the refusals of the C ABI, native fits on the views
against bi_fit_batched_real on the expanded grid model, the asymptotic formulae against the closed forms of a counting
experiment, and the factories on the twelve-parameter example.

The bars are tests/test_real_counts_gpu.py's: a finite value is held to 1e-10 max(1, |want|), a gradient entry to
1e-10 max(1, cond) with cond = sum_b |d_q mu_b| |1 - n_b / mu_b| from the oracle; +-inf, nan, status words and "bitwise" are
exact.  Profile minima: tests/test_profile_gpu.py's two bars, never above the other route's by more than 1e-8 max(1, D) and
equal to 1e-6 max(1, D)."""
import numpy as np
import pytest
from scipy import stats
from scipy.optimize import brentq

import factored_oracle as fo
import sourcewise_real_oracle as sro
import sourcewise_toy_cases as cases

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope='module')
def inputs():
    """name -> (model, its expansion, truths z [3, d], rs [3, S]): built once and left unchanged"""
    out = {}
    for name in cases.ALL_CASES:
        model, z, rs = cases.make_case(name)
        out[name] = (model, fo.expand(model), z, rs)
    return out


def check_against_oracle(got, wants, what, gradient=True):
    half, gz, gs, st = got
    worst = worst_g = 0.0
    for p, want in enumerate(wants):
        assert st[p] == want['status'], '%s point %d: status %d, want %d' % (what, p, st[p], want['status'])
        w = want['half_deviance']
        if np.isfinite(w):
            worst = max(worst, abs(half[p] - w) / max(1.0, abs(w)))
            assert abs(half[p] - w) <= TOL * max(1.0, abs(w)), '%s point %d: half-deviance %r, want %r' % (what, p, half[p], w)
        else:
            assert (np.isnan(half[p]) if np.isnan(w) else half[p] == w), '%s point %d: half-deviance %r, want %r' % (what, p, half[p], w)
        if not gradient:
            continue
        g = np.concatenate([gz[p], gs[p]])
        if not np.isfinite(w):
            assert np.isnan(g).all(), '%s point %d: gradient %r where the value is %r' % (what, p, g, w)
            continue
        bound = TOL * np.maximum(1.0, want['grad_cond'])
        err = np.abs(g - want['grad'])
        worst_g = max(worst_g, float(np.max(err / bound)) * TOL)
        assert np.all(err <= bound), '%s point %d: gradient %r, want %r (cond %r)' % (what, p, g, want['grad'], want['grad_cond'])
    print('%s: largest deviation %.3g of max(1, |want|)%s' % (what, worst, ', gradient %.3g of max(1, cond)' % worst_g if gradient else ''))


# ---- 1. the evaluation against the oracle ---------------------------------------------------------------------------------

@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_bi_eval_sourcewise_real_against_the_oracle(inputs, name):
    """Nine points (seven live, the last of them on the box edge; one outside the box, one with a negative rate) against the
    datasets in turn, with the gradient and value-only; no ordinary counts are resident."""
    model, full, zt, rst = inputs[name]
    counts = sro.real_datasets(name, model, zt, rst)
    z, rs, ds = sro.points_of(name, model, len(counts))
    wants = [sro.want_point(model, full, counts[ds[p]], z[p], rs[p]) for p in range(len(ds))]
    assert [w['status'] for w in wants[sro.N_LIVE:]] == [sro.ST_OUT_OF_BOUNDS, sro.ST_UNPHYSICAL]
    ctx = cases.upload(model)
    try:
        ctx.set_real_counts(counts)
        assert ctx.real_count_sets == len(counts) and ctx.T == 0
        np.testing.assert_array_equal(ctx.download_real_counts(1), counts[1])
        got = ctx.eval_real(z, rs, ds)
        check_against_oracle(got, wants, name)
        value_only = ctx.eval_real(z, rs, ds, gradient=False)
        check_against_oracle(value_only, wants, name + ', value only', gradient=False)
        # the value-only call gives the bits of the value of the gradient call; a second call is bitwise identical
        np.testing.assert_array_equal(value_only[0], got[0])
        np.testing.assert_array_equal(value_only[3], got[3])
        again = ctx.eval_real(z, rs, ds)
        for a, b in zip(again, got):
            np.testing.assert_array_equal(a, b)
        assert np.all(got[0][sro.N_LIVE:] == np.inf) and np.isnan(got[1][sro.N_LIVE:]).all() and np.isnan(got[2][sro.N_LIVE:]).all()
        # a point alone has the bits it has inside the batch of seven
        L = sro.N_LIVE
        batch = ctx.eval_real(z[:L], rs[:L], ds[:L])
        for a, b in zip(batch, got):
            np.testing.assert_array_equal(a, b[:L])
        for p in range(L):
            alone = ctx.eval_real(z[p:p + 1], rs[p:p + 1], ds[p:p + 1])
            for a, b in zip(alone, batch):
                np.testing.assert_array_equal(a[0], b[p])
            assert ctx.eval_real(z[p:p + 1], rs[p:p + 1], ds[p:p + 1], gradient=False)[0][0] == batch[0][p]
        if name == 'zero_both_sides':
            hit = ds[:L] == 3                                   # the dataset with an event where mu_b = 0
            assert hit.any() and np.all(batch[0][hit] == np.inf) and np.isnan(batch[1][hit]).all() and np.isnan(batch[2][hit]).all()
            assert np.all(np.isfinite(batch[0][~hit]))
        else:
            assert np.all(np.isfinite(batch[0])) and np.all(batch[0] > 0)
        dev = ctx._dev
        assert dev._lib.bi_eval_sourcewise_real(dev._h, 0, None, None, None, None, None, None) == 0          # P = 0
    finally:
        ctx.close()


# ---- 2. Asimov sets -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_asimov_sets_are_the_expected_counts_and_exact_at_the_truth(inputs, name):
    """Set h is bit for bit row h of bi_sourcewise_expected_counts; at its own truth (the third lies on the box edge) the value
    and every gradient entry are 0.0 exactly; at another truth the value is > 0 and the oracle's."""
    model, full, z, rs = inputs[name]
    ctx = cases.upload(model)
    try:
        assert ctx.set_asimov_counts(z, rs) == 3 and ctx.real_count_sets == 3
        rows = np.stack([ctx.download_real_counts(h) for h in range(3)])
        assert np.array_equal(rows, ctx.expected_counts(z, rs))
        for h in range(3):
            want = cases.exact_expectation(model, z[h], rs[h])[0].astype(float)
            assert np.all(np.abs(rows[h] - want) <= TOL * np.maximum(1.0, want))
        half, gz, gs, st = ctx.eval_real(z, rs, np.arange(3))
        assert np.all(st == 0) and np.all(half == 0.0) and np.all(gz == 0.0) and np.all(gs == 0.0), (half, gz, gs)
        assert np.all(ctx.eval_real(z, rs, np.arange(3), gradient=False)[0] == 0.0)
        other = (np.arange(3) + 1) % 3                          # set h at the truth of set h + 1
        got = ctx.eval_real(z[other], rs[other], np.arange(3))
        assert np.all(got[0] > 0)
        check_against_oracle(got, [sro.want_point(model, full, rows[h], z[other[h]], rs[other[h]]) for h in range(3)], name + ', another truth')
        for h in range(3):                                      # one call of three truths equals three calls of one
            assert ctx.set_asimov_counts(z[h:h + 1], rs[h:h + 1]) == 1 and ctx.real_count_sets == 1
            assert np.array_equal(ctx.download_real_counts(0), rows[h])
        assert ctx.set_asimov_counts(z[:1], None) == 1          # rate_scale NULL: ones
        assert np.array_equal(ctx.download_real_counts(0), ctx.expected_counts(z[:1], np.ones_like(rs[:1]))[0])
    finally:
        ctx.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------

def test_the_c_abi_refuses_what_it_cannot_do(inputs):
    from blueice_amd.exceptions import NotPreparedException
    model, full, z, rs = inputs['B1001']
    B = fo.n_bins(model)
    rng = np.random.default_rng(31)
    ordinary = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    ctx = cases.upload(model, ordinary)
    try:
        ll_before = ctx.eval_grad(z, rs)
        for call in (lambda: ctx.eval_real(z[:1], rs[:1]), lambda: ctx.download_real_counts(0)):          # no store yet
            with pytest.raises(NotPreparedException, match='no real-valued dataset'):
                call()
        assert ctx.real_count_sets == 0
        ctx.set_asimov_counts(z[:2], rs[:2])
        before = [ctx.download_real_counts(h) for h in range(2)]

        def unchanged():
            assert ctx.real_count_sets == 2
            for h in range(2):
                assert np.array_equal(ctx.download_real_counts(h), before[h])

        # a truth outside the box, a negative rate: the error names the truth
        zb = z.copy()
        zb[1, 0] = model['anchor_z'][0][-1] + 0.5
        with pytest.raises(ValueError, match=r'\(truth 1\): point is outside the anchor box'):
            ctx.set_asimov_counts(zb, rs)
        unchanged()
        rb = rs.copy()
        rb[2, 1] = -1.0
        with pytest.raises(ValueError, match=r'\(truth 2\): a rate is outside'):
            ctx.set_asimov_counts(z, rb)
        unchanged()
        # a nan / negative / inf count: dataset and bin
        for bad in (np.nan, -0.5, np.inf):
            c = np.stack([before[0], before[1]])
            c[1, 17] = bad
            with pytest.raises(ValueError, match='dataset 1, bin 17'):
                ctx.set_real_counts(c)
            unchanged()
        # a dataset index outside the store
        for t in (2, -1):
            with pytest.raises(ValueError, match='outside the 2 real-valued sets'):
                ctx.eval_real(z[:2], rs[:2], [0, t])
            with pytest.raises(ValueError):
                ctx.download_real_counts(t)
        unchanged()
        assert ctx.eval_real(z[:1], rs[:1])[0][0] == 0.0          # still usable
        # the ordinary counts: the same bi_eval_factored bits with the real store filled, and after it is dropped
        for a, b in zip(ctx.eval_grad(z, rs), ll_before):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ctx.download_counts(0), ordinary)
        ctx.set_real_counts(before[0] * 0.5)
        assert ctx.real_count_sets == 1 and ctx.T == 1
        ctx.set_real_counts(None)
        assert ctx.real_count_sets == 0
        with pytest.raises(NotPreparedException, match='no real-valued dataset'):
            ctx.eval_real(z[:1], rs[:1])
        for a, b in zip(ctx.eval_grad(z, rs), ll_before):
            np.testing.assert_array_equal(a, b)
    finally:
        ctx.close()
    assert B == 1001
    # an expectation that is not finite: every rate is finite (1.2e308) but their sum over the three sources is not
    model, full, z, rs = inputs['B1']
    ctx = cases.upload(model)
    try:
        ctx.set_asimov_counts(z[:1], rs[:1])
        before = ctx.download_real_counts(0)
        huge = np.stack([rs[0], 1.2e308 / ctx.interpolate('mus', z[1])])
        assert np.all(np.isfinite(huge[1] * ctx.interpolate('mus', z[1])))
        with pytest.raises(ValueError, match=r'\(truth 1\): the expectation is not finite in bin 0'):
            ctx.set_asimov_counts(z[:2], huge)
        assert ctx.real_count_sets == 1 and np.array_equal(ctx.download_real_counts(0), before)
    finally:
        ctx.close()


# ---- 4. native fits -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def mixed(inputs):
    model, full, z, rs = inputs['mixed']
    sw, plain = sro.likelihoods(model)
    return model, z, rs, sw, plain


def _truths(z, rs):
    pts = {'shape%d' % i: z[:, i].copy() for i in range(z.shape[1])}
    pts.update({'s%d_rate_multiplier' % s: rs[:, s].copy() for s in range(rs.shape[1])})
    return pts


def test_native_fits_come_back_to_the_truth_of_every_asimov_set(mixed):
    """Class `mixed` at B = 1027: asimov_points at three truths (the last on the box edge), all eight parameters free, from a
    displaced guess: every fit ends with -1e-10 <= D <= 1e-10, on the native loop (no Python between the iterations)."""
    from blueice_amd import asimov
    from blueice_amd.inference import bestfit_batched
    model, z, rs, sw, plain = mixed
    view = asimov.asimov_points(sw, _truths(z, rs))
    assert view.n_sets == 3 and view.ctx.T == 3 and not sw.is_data_set
    calls = [0]
    inner = view.values_and_gradients

    def counted(points, livetime_days=None, dataset=None):
        calls[0] += 1
        return inner(points, livetime_days=livetime_days, dataset=dataset)
    view.values_and_gradients = counted
    mid = {'shape%d' % i: float(0.5 * (g[0] + g[-1])) for i, g in enumerate(model['anchor_z'])}
    guess = dict(mid, **{'s%d_rate_multiplier' % s: 1.0 for s in range(rs.shape[1])})
    best, ll, info = bestfit_batched(view, datasets=np.arange(3), guess=guess, gtol=1e-9, return_info=True)
    assert calls[0] == 0 and info['evaluations'] > 0 and info['analytic_gradient']
    print('D at the fits: %s, %d evaluations' % (-ll, info['evaluations']))
    for h in range(3):
        assert -ll[h] <= 1e-10 and -ll[h] >= -TOL, (h, ll[h])


def test_profiled_minima_against_the_grid_model(mixed):
    """One Asimov set; one rate multiplier at five hypotheses, everything else free: bi_fit_batched_sourcewise_real against
    bi_fit_batched_real on the expanded grid model holding the same data (bi_set_real_counts), from the same starts."""
    from blueice_amd import asimov
    from blueice_amd.inference import bestfit_batched
    model, z, rs, sw, plain = mixed
    truth = {k: float(v[0]) for k, v in _truths(z, rs).items()}
    view = asimov.asimov(sw, **truth)
    n = view.counts(0)
    grid_view = asimov.real_data(plain, n)
    assert np.array_equal(grid_view.counts(0), n)
    hyps = truth['s1_rate_multiplier'] * np.array([0.6, 0.8, 1.0, 1.25, 1.5])
    start = {k: v for k, v in truth.items() if k != 's1_rate_multiplier'}
    res = []
    for v in (view, grid_view):
        best, ll, info = bestfit_batched(v, points={'s1_rate_multiplier': hyps}, guess=start, gtol=1e-9, return_info=True)
        assert info['evaluations'] > 0
        res.append(-np.asarray(ll))
    D_sw, D_grid = res
    print('profiled D, source-wise %s\n            grid model  %s' % (D_sw, D_grid))
    for h in range(len(hyps)):
        bar = max(1.0, D_grid[h])
        assert D_sw[h] <= D_grid[h] + 1e-8 * bar, (h, D_sw[h], D_grid[h])
        assert abs(D_sw[h] - D_grid[h]) <= 1e-6 * bar, (h, D_sw[h], D_grid[h])
    assert abs(D_sw[2]) <= 1e-10 and D_sw[0] > 1.0 and D_sw[-1] > 1.0


# ---- 5. a counting experiment ---------------------------------------------------------------------------------------------

def test_closed_forms_of_a_counting_experiment():
    """d = 0, S = 2, B = 1, s = 10 and b = 50 events, the signal's rate the only parameter; no data are ever set"""
    from blueice_amd import SourceWiseBinnedLogLikelihood, inference
    import model_zoo
    ns = model_zoo.namespace_of('blueice_amd')
    data, _ = ns.make_data([dict(n_events=8, x=0.5)])
    conf = ns.conf_for_test(default_source_class=ns.FixedSampleSource, analysis_space=[['x', [0, 1]]], data=data)
    conf['sources'] = [dict(name='s0', events_per_day=10.0), dict(name='s1', events_per_day=50.0)]
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False))
    lf.add_rate_parameter('s0')
    lf.prepare()
    s, b = [float(v) for v in lf.base_model.expected_events()]
    assert abs(s - 10.0) <= 1e-12 and abs(b - 50.0) <= 1e-12 and not lf.is_data_set and lf.ctx.d == 0 and lf.ctx.B == 1

    def q_closed(mu):
        return 2.0 * (mu * s - b * np.log1p(mu * s / b))
    hyps = np.array([0.25, 0.5, 1.0, 2.0, 3.5])
    q = inference.asimov_test_statistic(lf, 's0_rate_multiplier', hyps)
    print('q_A %s, closed form %s' % (q, q_closed(hyps)))
    assert np.all(np.abs(q - q_closed(hyps)) <= TOL * np.maximum(1.0, q_closed(hyps)))
    zs = inference.expected_discovery_significance(lf, 's0_rate_multiplier', dict(s0_rate_multiplier=1.0))
    want = np.sqrt(2.0 * ((s + b) * np.log1p(s / b) - s))
    assert abs(zs - want) <= TOL * max(1.0, want), (zs, want)
    limits = inference.expected_upper_limit(lf, 's0_rate_multiplier', 20.0, confidence_level=0.9, n_sigma=(-1, 0, 1, 2))
    for n in (-1, 0, 1, 2):
        c = stats.norm.ppf(0.9) + n
        want = brentq(lambda mu: q_closed(mu) - c ** 2, 1e-9, 20.0, xtol=1e-14, rtol=1e-14)
        print('N = %+d: expected limit %.10f, closed form %.10f' % (n, limits[n], want))
        assert abs(limits[n] - want) <= 1e-8 * want, (n, limits[n], want)
    assert limits[-1] < limits[0] < limits[1] < limits[2] and not lf.is_data_set


# ---- 6. through the class -------------------------------------------------------------------------------------------------

def test_the_factories_on_the_twelve_parameter_example():
    from blueice_amd import SourceWiseBinnedLogLikelihood, asimov, inference
    from blueice_amd.asimov import AsimovLikelihood
    from blueice_amd.exceptions import NotPreparedException
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0, device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    lf.prepare()
    truth = {names[0]: 0.5, names[3]: -0.25, 's0_rate_multiplier': 0.0}
    view = asimov.asimov(lf, **truth)
    assert isinstance(view, AsimovLikelihood) and view.n_sets == 1 and not view.supports_hessian and view.supports_gradient
    assert not lf.is_data_set and lf.ctx.T == 0                  # no data were needed, none are claimed
    mu = inference.expected_counts_points(lf, {k: np.array([v]) for k, v in truth.items()})[0]
    assert np.array_equal(view.counts(0), mu) and mu.shape == (6, 5)
    assert view(**truth) == 0.0
    value, grads = view.value_and_gradient(**truth)
    assert value == 0.0 and all(g == 0.0 for g in grads.values()) and len(grads) == 4 + len(names)
    off = dict(truth, s0_rate_multiplier=0.7)
    assert view(**off) < 0 and view.eval_points({k: [v] for k, v in off.items()})[0] == view(**off)
    ll, g = view.values_and_gradients({k: [v] for k, v in off.items()})
    assert ll[0] == view(**off) and g['s0_rate_multiplier'][0] < 0
    scan = view.likelihood_ratio_scan(('s0_rate_multiplier', np.array([0.0, 0.5, 1.0])), **{n: truth.get(n, 0.0) for n in names},
                                      s1_rate_multiplier=1.0, s2_rate_multiplier=1.0, s3_rate_multiplier=1.0)
    assert scan[0] == 0.0 and scan[1] > 0 and scan[2] > scan[1]
    best, top = view.bestfit_device(**{n: truth.get(n, 0.0) for n in names})
    assert abs(top) <= 1e-9 and abs(best['s0_rate_multiplier']) <= 1e-3

    # the bound names against the module functions
    many = lf.asimov_points({names[0]: np.array([-0.5, 0.5])})
    assert isinstance(many, AsimovLikelihood) and many.n_sets == 2
    with pytest.raises(NotPreparedException, match='stale'):
        view(**truth)
    with pytest.raises(NotPreparedException, match='stale'):
        view.bestfit_batched()
    assert np.all(many.eval_points({names[0]: np.array([-0.5, 0.5])}, dataset=np.arange(2)) == 0.0)
    fixed = {n: 0.0 for n in names}
    hyps = np.array([0.5, 1.5])
    q_bound = lf.asimov_test_statistic('s0_rate_multiplier', hyps, **fixed)
    q_module = inference.asimov_test_statistic(lf, 's0_rate_multiplier', hyps, **fixed)
    assert np.array_equal(q_bound, q_module) and np.all(q_bound > 0) and q_bound[1] > q_bound[0]
    z_bound = lf.expected_discovery_significance('s0_rate_multiplier', dict(s0_rate_multiplier=1.0), **fixed)
    assert z_bound == inference.expected_discovery_significance(lf, 's0_rate_multiplier', dict(s0_rate_multiplier=1.0), **fixed) and z_bound > 0
    limits = inference.expected_upper_limit(lf, 's0_rate_multiplier', 6.0, n_sigma=(0, 1), **fixed)
    assert 0.0 < limits[0] < limits[1] < 6.0
    for name, spelling in (('asimov', 'blueice_amd.asimov.asimov(lf, **truth)'), ('real_data', 'blueice_amd.asimov.real_data(lf, counts)'),
                           ('expected_upper_limit', 'blueice_amd.inference.expected_upper_limit(lf, target, bound)')):
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            getattr(lf, name)()
        assert spelling in str(e.value)
    pseudo = 0.25 * mu
    weighted = asimov.real_data(lf, pseudo)
    assert np.array_equal(weighted.counts(0), pseudo) and np.isfinite(weighted(**truth)) and weighted(**truth) < 0
    assert not lf.is_data_set
