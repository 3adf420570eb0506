"""Real-valued counts on the device: bi_eval_real against the numpy oracle (tests/real_counts_oracle.py) at every shape,
the Asimov datasets of bi_set_asimov_counts against bi_expected_counts bit for bit, exact zeros at the truth, native fits on
the views, the asymptotic formulae against closed forms of a counting experiment, and the refusals of the C ABI.

The bar for finite values is the project's fp64 bar as tests/test_gof_gpu.py states it, 1e-10 max(1, |want|); a gradient
entry is held to 1e-10 max(1, cond) with cond = sum_b |d_q mu_b| |1 - n_b / mu_b|, the entry's own condition from the
oracle; +-inf, nan and the status words are exact."""
from collections import OrderedDict

import numpy as np
import pytest
from scipy import stats
from scipy.optimize import brentq, minimize

import gof_oracle
import model_zoo
import real_counts_oracle as rco
from golden_util import load_case
from test_gof_gpu import SHAPES, case_of

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


@pytest.fixture(scope='module')
def zoo(ns):
    """name -> (likelihood, its anchor tensors): built once; no test changes a likelihood's own data"""
    out = OrderedDict()
    for i, (name, s) in enumerate(SHAPES.items()):
        lf = model_zoo.morph_lf(ns, np.random.default_rng(100 + i), s['S'], s['space'], s['anchors'], 20000, 150, livetime=s.get('livetime'))
        out[name] = (lf, gof_oracle.tensors_of(lf))
    return out


COUNTING = dict(anchor_z=[], ps=np.ones((2, 1)), mus=np.array([10.0, 50.0]), n_model=None)     # B = 1: s = 10, b = 50
ALL_SHAPES = list(SHAPES) + ['counting_B1']


def real_case(zoo, name, seed):
    """The tensors (test_gof_gpu.case_of: a floor under every template, one bin where every template is 0), four real-valued
    datasets -- the expectation at another point, 0.3 x an expectation (counts inside (0, 1)), all zeros, one with a count in
    the bin where nothing is expected -- and the points: on an anchor, inside a cell, on the box edge, outside, a negative
    rate; every point against every dataset."""
    if name == 'counting_B1':
        model = COUNTING
        counts = np.array([[57.25], [0.3 * 60.0], [0.0], [7.5]])
        zs = np.zeros((6, 0))
        rs = np.array([[1.0, 1.0], [0.37, 1.2], [0.0, 1.0], [2.5, 0.4], [-0.5, 1.0], [0.0, 0.0]])     # the last: nothing expected at all
    else:
        model, _, zs, rs, _, dead = case_of(zoo[name][1], seed)
        zs, rs = zs[::3], rs[::3]
        d, S, B = zs.shape[1], rs.shape[1], model['ps'].shape[-1]
        other = rco.expectation(model, [0.2, -0.3][:d], np.full(S, 1.1))
        hit = other.copy()
        hit[dead] = 0.75
        counts = np.stack([other, 0.3 * rco.expectation(model, [0.0] * d, np.ones(S)), np.zeros(B), hit])
        assert np.count_nonzero((counts[1] > 0) & (counts[1] < 1)) > B // 2
    P, T = len(zs), len(counts)
    return model, counts, np.repeat(zs, T, axis=0), np.repeat(rs, T, axis=0), np.tile(np.arange(T), P)


def context_of(model, allow_negative=None):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])
    if allow_negative is not None:
        ctx.set_allow_negative([1 if a else 0 for a in allow_negative])
    return ctx


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


@pytest.fixture(scope='module')
def oracle_results(zoo):
    """name -> (case, the oracle's result for every (point, dataset)): computed once, shared by the tests that need it"""
    out = {}
    for name in ALL_SHAPES:
        case = real_case(zoo, name, seed=7)
        model, counts, zs, rs, ds = case
        out[name] = (case, [rco.point(model, counts[ds[p]], zs[p], rs[p]) for p in range(len(ds))])
    return out


@pytest.mark.parametrize('name', ALL_SHAPES)
def test_bi_eval_real_against_the_oracle(oracle_results, name):
    """Every point against every dataset in one call, value-only and with the gradient; no ordinary data are resident.  With
    tile_chunks 1 and 8: B = 600 is two tiles, and every item's two blocks take one each."""
    (model, counts, zs, rs, ds), wants = oracle_results[name]
    d = zs.shape[1]
    ctx = context_of(model)
    try:
        ctx.set_real_counts(counts)
        assert ctx.real_count_sets == len(counts)
        np.testing.assert_array_equal(ctx.download_real_counts(1), counts[1])
        for chunks in (8, 1):
            ctx.set_param('tile_chunks', chunks)
            what = '%s, tile_chunks %d' % (name, chunks)
            check_against_oracle(ctx.eval_real(zs if d else None, rs, ds), wants, what)
            check_against_oracle(ctx.eval_real(zs if d else None, rs, ds, gradient=False), wants, what + ', value only', gradient=False)
        half, _, _, st = ctx.eval_real(zs if d else None, rs, ds)
        live = st == 0
        assert np.count_nonzero(live) >= 12 and np.all(half[~live] == np.inf)
        assert np.all(np.isfinite(half[live & (ds != 3)]) | (name == 'counting_B1')) and np.all(half[live & (ds == 2)] >= 0)
        if name != 'counting_B1':
            assert np.all(half[live & (ds == 3)] == np.inf)          # the count where every template is 0
    finally:
        ctx.close()


def test_bi_eval_real_is_nan_where_an_expectation_is_negative(zoo):
    """A source that may go negative: where a bin's expectation is negative the value is nan, as ll is, and so is the gradient"""
    model, counts, zs, rs, ds = real_case(zoo, 'd1_S3_B600', seed=8)
    S = rs.shape[1]
    allow = [False] * (S - 1) + [True]
    rs = rs.copy()
    rs[4:8, S - 1] = -0.05
    rs[8:12, :S - 1] = 1.0                  # the point on the edge: nearly all of the other sources' rate taken away again
    rs[8:12, S - 1] = -0.9 * (model['mus'][..., :S - 1].sum(axis=-1).min() / model['mus'][..., S - 1].max())
    wants = [rco.point(model, counts[ds[p]], zs[p], rs[p], allow) for p in range(len(ds))]
    assert any(np.isnan(w['half_deviance']) for w in wants)
    ctx = context_of(model, allow)
    try:
        ctx.set_real_counts(counts)
        check_against_oracle(ctx.eval_real(zs, rs, ds), wants, 'allow-negative')
    finally:
        ctx.close()


@pytest.mark.parametrize('name', ALL_SHAPES)
def test_asimov_counts_are_the_expected_counts_and_exact_at_the_truth(zoo, name):
    """bi_set_asimov_counts: rows bit for bit bi_expected_counts, the oracle's mu to the bar, H = 3 truths in one call equal
    three calls of one.  At its own truth every set has half_deviance == 0.0 and every gradient entry == 0.0 EXACTLY (the same
    fused multiply-add chain forms mu on both sides): on an anchor, inside a cell and on the box edge, with both tile orders."""
    if name == 'counting_B1':
        model, zs = COUNTING, np.zeros((3, 0))
    else:
        model, _, zs, _, _, _ = case_of(zoo[name][1], seed=7)
        zs = zs[::3][:3]
    d, S = zs.shape[1], np.shape(model['mus'])[-1]
    rs = np.random.default_rng(11).uniform(0.6, 1.5, size=(3, S))
    ctx = context_of(model)
    try:
        assert ctx.set_asimov_counts(zs if d else None, rs) == 3 and ctx.real_count_sets == 3
        rows = np.stack([ctx.download_real_counts(h) for h in range(3)])
        assert np.array_equal(rows, ctx.expected_counts(zs if d else None, rs))
        for h in range(3):
            want = rco.expectation(model, zs[h], rs[h])
            assert np.all(np.abs(rows[h] - want) <= TOL * np.maximum(1.0, np.abs(want)))
        for chunks in (8, 1):
            ctx.set_param('tile_chunks', chunks)
            half, gz, gs, st = ctx.eval_real(zs if d else None, rs, np.arange(3))
            assert np.all(st == 0) and np.all(half == 0.0) and np.all(gz == 0.0) and np.all(gs == 0.0), (half, gz, gs)
            assert np.all(ctx.eval_real(zs if d else None, rs, np.arange(3), gradient=False)[0] == 0.0)
        # away from the truth it is not zero
        assert np.all(ctx.eval_real(zs if d else None, rs * 1.1, np.arange(3))[0] > 0)
        for h in range(3):
            assert ctx.set_asimov_counts(zs[h:h + 1] if d else None, rs[h:h + 1]) == 1
            assert np.array_equal(ctx.download_real_counts(0), rows[h])
    finally:
        ctx.close()


def test_the_c_abi_refuses_what_it_cannot_do(zoo):
    from blueice_amd.device import DeviceContext
    from blueice_amd.exceptions import NotPreparedException
    model, counts, zs, rs, ds = real_case(zoo, 'd1_S3_B600', seed=7)
    ctx = context_of(model)
    try:
        with pytest.raises(NotPreparedException):                     # no store yet
            ctx.eval_real(zs[:1], rs[:1])
        ctx.set_asimov_counts([[0.25]], rs[:1])
        before = ctx.download_real_counts(0)
        # a truth outside the box, unphysical rates: the error names the truth, the previous store is intact
        with pytest.raises(ValueError, match='truth 1 lies outside'):
            ctx.set_asimov_counts([[0.5], [1.5], [0.0]], np.ones((3, 3)))
        with pytest.raises(ValueError, match='truth 2 has unphysical'):
            ctx.set_asimov_counts([[0.5], [0.5], [0.0]], [[1, 1, 1], [1, 1, 1], [1, -1, 1]])
        # nan / negative / inf counts: dataset and bin
        for bad in (np.nan, -0.5, np.inf):
            c = counts[:2].copy()
            c[1, 17] = bad
            with pytest.raises(ValueError, match='dataset 1, bin 17'):
                ctx.set_real_counts(c)
        assert ctx.real_count_sets == 1 and np.array_equal(ctx.download_real_counts(0), before)
        # a dataset index out of range
        for t in (1, -1):
            with pytest.raises(ValueError, match='outside the 1 real-valued sets'):
                ctx.eval_real(zs[:2], rs[:2], [0, t])
        with pytest.raises(ValueError):
            ctx.download_real_counts(1)
        assert ctx.eval_real([[0.25]], rs[:1])[0][0] == 0.0          # still usable
        ctx.set_real_counts(None)
        assert ctx.real_count_sets == 0
    finally:
        ctx.close()
    # an expectation with a negative bin (a source that may go negative): no dataset
    neg = dict(anchor_z=[], ps=np.array([[1.0, 0.0], [0.0, 1.0]]), mus=np.array([10.0, 5.0]), n_model=None)
    ctx = context_of(neg, [False, True])
    try:
        ctx.set_asimov_counts(None, [[1.0, 0.5]])
        with pytest.raises(ValueError, match='truth 1 is negative or nan in bin 1'):
            ctx.set_asimov_counts(None, [[1.0, 1.0], [1.0, -1.0]])
        np.testing.assert_array_equal(ctx.download_real_counts(0), [10.0, 2.5])
    finally:
        ctx.close()
    # 1 + d + S = 17 gradient columns: refused; the value alone has no such limit
    wide = dict(anchor_z=[], ps=np.full((16, 5), 0.2), mus=np.arange(1.0, 17.0), n_model=None)
    ctx = context_of(wide)
    try:
        ctx.set_real_counts(np.full(5, 30.0))
        with pytest.raises(ValueError, match='17'):
            ctx.eval_real(None, np.ones((1, 16)))
        want = rco.point(wide, np.full(5, 30.0), [], np.ones(16))['half_deviance']
        assert abs(ctx.eval_real(None, np.ones((1, 16)), gradient=False)[0][0] - want) <= TOL * max(1.0, want)
    finally:
        ctx.close()
    # Beeston-Barlow and unbinned contexts
    c = load_case('ref_bb_multi_bin')
    ctx = DeviceContext(0)
    try:
        ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'], n_model=c['model']['n_model'], bb_source=c['bb_source'])
        ctx.upload_counts(c['counts'])
        for call in (lambda: ctx.set_real_counts(np.asarray(c['counts'], dtype=float)), lambda: ctx.set_asimov_counts(None, np.ones((1, c['S']))),
                     lambda: ctx.eval_real(None, np.ones((1, c['S']))), lambda: ctx.download_real_counts(0)):
            with pytest.raises(ValueError, match='Beeston-Barlow'):
                call()
        ll, st = ctx.eval(None, np.ones((1, c['S'])))          # the context is as usable as before
        assert np.isfinite(ll[0]) and st[0] == 0
    finally:
        ctx.close()
    c = load_case('unb_d0_three_sources')
    ctx = DeviceContext(0)
    try:
        n_ev = c['bins'][0]
        ctx.begin_model(c['model']['anchor_z'], c['S'], n_ev)
        ctx.set_anchor(0, np.asarray(c['model']['ps']).reshape(c['S'], n_ev), np.asarray(c['model']['mus']).reshape(c['S']))
        ctx.end_model()
        ctx.set_unbinned(c['outlier'])
        for call in (lambda: ctx.set_real_counts(np.ones(n_ev)), lambda: ctx.set_asimov_counts(None, np.ones((1, c['S']))),
                     lambda: ctx.eval_real(None, np.ones((1, c['S'])))):
            with pytest.raises(ValueError, match='unbinned'):
                call()
    finally:
        ctx.close()


def test_native_fits_on_the_asimov_view(zoo):
    """d1_S3_B600, the shape parameter and one rate floating.  The native loop on the Asimov view, from a displaced start,
    comes back to the truth; `asimov_test_statistic` over 8 hypotheses is held against scipy's minimiser on the oracle's D as
    tests/test_profile_gpu.py holds profile fits: never above the oracle's minimum by more than 1e-8 max(1, D), equal to 1e-6
    where scipy converged."""
    lf, model = zoo['d1_S3_B600']
    truth = dict(shift=0.37, s0_rate_multiplier=1.3)
    fixed = dict(s1_rate_multiplier=1.0, s2_rate_multiplier=1.0)
    view = lf.asimov(**truth, **fixed)
    calls = [0]
    inner = view.values_and_gradients

    def counted(points, livetime_days=None, dataset=None):
        calls[0] += 1
        return inner(points, livetime_days=livetime_days, dataset=dataset)
    view.values_and_gradients = counted
    best, ll, info = view.bestfit_batched(guess=dict(shift=-0.5, s0_rate_multiplier=0.7), gtol=1e-9, return_info=True, **fixed)
    assert calls[0] == 0 and info['evaluations'] > 0 and info['analytic_gradient']          # the loop ran natively
    print('fit on the Asimov view: shift %.9f, s0 %.9f, D %.3g' % (best['shift'][0], best['s0_rate_multiplier'][0], -ll[0]))
    assert abs(best['shift'][0] - truth['shift']) <= 1e-6 and abs(best['s0_rate_multiplier'][0] - truth['s0_rate_multiplier']) <= 1e-6
    assert -ll[0] <= 1e-10 and -ll[0] >= -TOL          # D <= 1e-10 (and, D >= 0 being a sum of rounded terms, not below 0 by more than the bar)
    # the other entry points of the view agree with the oracle at a point of its own
    n = view.counts(0).ravel()
    unit = 1.0                                   # (no live-time scaling in these calls)
    # (in the truth's grid cell: the sampled templates have bins that only one anchor fills, so across the anchor at 0 some
    #  filled bin of the Asimov data expects nothing and the value is -inf, which the oracle tests above cover)
    at = dict(shift=0.2, s0_rate_multiplier=0.9, **fixed)
    want = rco.point(model, n, [at['shift']], [0.9 * unit, 1.0, 1.0])
    value, grads = view.value_and_gradient(**at)
    assert abs(view(**at) + want['half_deviance']) <= TOL * max(1.0, want['half_deviance'])
    assert abs(view(**at) - value) <= TOL * max(1.0, abs(value))          # (the value-only kernel and the gradient kernel)
    assert abs(grads['shift'] + want['grad'][0]) <= TOL * max(1.0, want['grad_cond'][0])
    assert abs(grads['s0_rate_multiplier'] + want['grad'][1]) <= TOL * max(1.0, want['grad_cond'][1])
    assert abs(view.eval_points({k: [v] for k, v in at.items()})[0] - value) <= TOL * max(1.0, abs(value))
    assert view.supports_gradient and not view.supports_hessian and view.get_bounds('shift') == lf.get_bounds('shift')
    print('saturated_ll %.6g, value %.6g' % (view.saturated_ll(0), value))

    # the test statistic against scipy on the oracle
    hyps = np.linspace(0.6, 2.0, 8)
    q = lf.asimov_test_statistic('s0_rate_multiplier', hyps, truth=dict(truth, **fixed), fit_options=dict(gtol=1e-9), **fixed)
    n = lf.asimov(**truth, **fixed).counts(0).ravel()
    worst, n_converged = 0.0, 0
    for h, qa in zip(hyps, q):
        def fun(x):
            r = rco.point(model, n, [x[0]], [h, 1.0, 1.0])
            return r['half_deviance'], r['grad'][:1]
        runs = []
        # (the cells are searched a hair inside their anchors: ON one the other anchor's weight is 0, a bin only that one fills
        #  expects nothing, D is +inf and scipy's line search has nothing to interpolate)
        for a, b in ((-1.0 + 1e-6, -1e-6), (1e-6, 1.0 - 1e-6)):
            if not np.isfinite(fun([0.5 * (a + b)])[0]):          # (a cell where D is +inf has no minimum)
                continue
            res = minimize(fun, [0.5 * (a + b)], jac=True, bounds=[(a, b)], method='L-BFGS-B', options=dict(ftol=1e-15, gtol=1e-9))
            for _ in range(5):          # (its ftol stop can fire after one short step: go on from there)
                res = minimize(fun, res.x, jac=True, bounds=[(a, b)], method='L-BFGS-B', options=dict(ftol=1e-15, gtol=1e-9))
            # converged: scipy says so AND the slope is gone, or points out of the cell at its edge
            g, x = float(res.jac[0]), float(res.x[0])
            res.success = bool(res.success and (abs(g) <= 1e-6 or (x <= a and g > 0) or (x >= b and g < 0)))
            runs.append(res)
        assert runs
        res = min(runs, key=lambda r: r.fun)
        got = 0.5 * qa
        worst = max(worst, abs(got - res.fun) / max(1.0, res.fun))
        assert got <= res.fun + 1e-8 * max(1.0, res.fun), (h, got, res.fun)
        n_converged += bool(res.success)
        if res.success:
            assert abs(got - res.fun) <= 1e-6 * max(1.0, res.fun), (h, got, res.fun)
    print('q_A / 2 against scipy on the oracle: largest deviation %.3g of max(1, D), scipy converged at %d of %d; q_A = %s' % (
        worst, n_converged, len(hyps), np.array2string(q, precision=4)))
    assert n_converged >= len(hyps) // 2          # (the comparison is not an empty one)
    assert q[np.argmin(np.abs(hyps - 1.3))] < q[0] and q[-1] > 1.0


@pytest.fixture(scope='module')
def counting_lf(ns):
    """One bin, signal s = 10 and background b = 50 events, the signal's rate the only parameter; no data are ever set"""
    data, _ = ns.make_data([dict(n_events=8, x=0.5)])
    conf = ns.conf_for_test(default_source_class=ns.FixedSampleSource, analysis_space=[['x', [0, 1]]], data=data)
    conf['sources'] = [dict(name='sig', events_per_day=10.0), dict(name='bkg', events_per_day=50.0)]
    lf = ns.BinnedLogLikelihood(conf)
    lf.add_rate_parameter('sig')
    lf.prepare()
    return lf


def test_closed_forms_of_a_counting_experiment(counting_lf):
    lf = counting_lf
    s, b = [float(v) for v in lf.base_model.expected_events()]
    assert abs(s - 10.0) <= 1e-12 and abs(b - 50.0) <= 1e-12 and not lf.is_data_set

    def q_closed(mu):
        return 2.0 * (mu * s - b * np.log1p(mu * s / b))
    hyps = np.array([0.25, 0.5, 1.0, 2.0, 3.5])
    q = lf.asimov_test_statistic('sig_rate_multiplier', hyps)
    print('q_A %s, closed form %s' % (q, q_closed(hyps)))
    assert np.all(np.abs(q - q_closed(hyps)) <= TOL * np.maximum(1.0, q_closed(hyps)))
    z = lf.expected_discovery_significance('sig_rate_multiplier', dict(sig_rate_multiplier=1.0))
    want = np.sqrt(2.0 * ((s + b) * np.log1p(s / b) - s))
    assert abs(z - want) <= TOL * max(1.0, want), (z, want)
    limits = lf.expected_upper_limit('sig_rate_multiplier', 20.0, confidence_level=0.9)
    assert list(limits) == [-2, -1, 0, 1, 2] and limits[-2] == 0.0
    for n in (-1, 0, 1, 2):
        c = stats.norm.ppf(0.9) + n
        want = brentq(lambda mu: q_closed(mu) - c ** 2, 1e-9, 20.0, xtol=1e-14, rtol=1e-14)
        print('N = %+d: expected limit %.10f, closed form %.10f' % (n, limits[n], want))
        assert abs(limits[n] - want) <= 1e-8 * want, (n, limits[n], want)
    assert limits[-1] < limits[0] < limits[1] < limits[2]


def test_the_parent_is_untouched_and_stale_views_raise(zoo, ns):
    from blueice_amd.exceptions import NotPreparedException
    lf, _ = zoo['d1_S3_B600']
    other, _ = zoo['d2_S2_B63']
    p = dict(shift=0.2, s0_rate_multiplier=1.1, s1_rate_multiplier=0.9)
    before = (lf(**p), lf.ctx.download_counts(0), lf.bestfit_device())
    view = lf.asimov(shift=0.37)
    view.bestfit_batched(s2_rate_multiplier=1.0)
    many = lf.asimov_points(dict(shift=[-0.5, 0.0, 0.5]))
    assert many.n_sets == 3 and many.ctx.T == 3
    with pytest.raises(NotPreparedException, match='stale'):
        view(**p)
    with pytest.raises(NotPreparedException, match='stale'):
        view.bestfit_batched(s2_rate_multiplier=1.0)
    at = many.eval_points(dict(shift=[-0.5, 0.0, 0.5]), dataset=np.arange(3))
    assert np.all(at == 0.0) and many(shift=0.5, dataset=2) == 0.0 and many(shift=0.5, dataset=0) < 0
    best, ll = many.bestfit_batched(datasets=np.arange(3), s1_rate_multiplier=1.0, s2_rate_multiplier=1.0)
    assert np.all(np.abs(best['shift'] - [-0.5, 0.0, 0.5]) <= 1e-5) and np.all(ll >= -1e-9)
    pseudo = 0.25 * lf.expected_counts(shift=0.3, s0_rate_multiplier=1.4)          # a weighted histogram as pseudo-data
    weighted = lf.real_data(pseudo)
    assert np.isfinite(weighted(**p)) and weighted(**p) < 0 and np.array_equal(weighted.counts(0), pseudo)
    lf.expected_upper_limit('s0_rate_multiplier', 6.0, n_sigma=(0,), s1_rate_multiplier=1.0, s2_rate_multiplier=1.0)
    after = (lf(**p), lf.ctx.download_counts(0), lf.bestfit_device())
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    assert after[2][1] == before[2][1] and list(after[2][0].items()) == list(before[2][0].items())
    # a sum of views of different likelihoods: the host combinator
    a, b = lf.asimov(shift=0.37), other.asimov(shift=0.3, stretch=0.4)
    total = ns.LogLikelihoodSum([a, b])
    q = dict(shift=0.1, stretch=0.3, s0_rate_multiplier=1.2)
    want = a(shift=0.1, s0_rate_multiplier=1.2) + b(**q)
    assert total(**q) == want and np.isfinite(want) and want < 0
    assert total.eval_points({k: [v] for k, v in q.items()})[0] == want
