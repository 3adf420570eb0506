"""Gridded likelihoods on the device (bi_grid_reduce): the reduction kernels alone against NumPy (bi_selftest_grid_reduce), the
whole path -- grid points made on the device, resident planner, evaluation, reduction -- against the CPU oracle, chunking,
several datasets in one call, the two engines of lf.grid_scan against each other, and the grid profile against fits."""
from collections import OrderedDict

import numpy as np
import pytest
from scipy.special import logsumexp

from golden_util import load_case
from oracle import blueice_oracle as orc

pytestmark = pytest.mark.gpu


def make_ctx(c, sparse=1):
    """a device context with the golden case's model and data"""
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    if c['kind'] == 1 or c['name'].startswith('unb_'):
        n_ev = c['bins'][0]
        ctx.begin_model(c['model']['anchor_z'], c['S'], n_ev)
        ps = c['model']['ps'].reshape((-1, c['S'], n_ev))
        mus = c['model']['mus'].reshape((-1, c['S']))
        for a in range(len(mus)):
            ctx.set_anchor(a, ps[a], mus[a])
        ctx.end_model()
        ctx.set_unbinned(c['outlier'])
        return ctx
    ctx.set_param('sparse', sparse)
    bb = c['bb_source']
    ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'], n_model=c['model']['n_model'] if bb >= 0 else None, bb_source=bb)
    if c.get('allow_negative') is not None and any(c['allow_negative']):
        ctx.set_allow_negative([1 if a else 0 for a in c['allow_negative']])
    ctx.upload_counts(c['counts'])
    return ctx


# ---- the reduction alone ---------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def ctx():
    from blueice_amd.device import DeviceContext
    c = DeviceContext(0)
    yield c
    c.close()


def numpy_reduce(t, q):
    cells = len(t)
    lm, prof, arg = np.empty(cells), np.empty(cells), np.empty(cells, dtype=np.int64)
    for k in range(cells):
        if np.isnan(t[k]).any():
            lm[k], prof[k], arg[k] = np.nan, np.nan, -1
            continue
        ok = t[k] > -np.inf
        if not ok.any():
            lm[k], prof[k], arg[k] = -np.inf, -np.inf, -1
            continue
        u = t[k][ok] if q is None else (t[k] + q[k])[ok]
        lm[k] = logsumexp(u) if np.any(u > -np.inf) else -np.inf
        prof[k] = t[k][ok].max()
        arg[k] = np.flatnonzero(t[k] == prof[k])[0]
    return lm, prof, arg


def reduction_case(cells, R, seed):
    """values with everything the reduction has to get right: a wide spread (exp underflows), a cell near -1e5, an empty
    cell, a cell with one finite point, exact ties, a nan, log weights with a -inf"""
    rng = np.random.default_rng(seed)
    t = rng.normal(0.0, 300.0, (cells, R))                    # spread far beyond 800
    t[0] = -1e5 + rng.normal(0.0, 3.0, R)
    q = rng.normal(0.0, 2.0, (cells, R))
    t[rng.random((cells, R)) < 0.1] = -np.inf                 # excluded points
    if cells > 1:
        t[1] = -np.inf                                        # a cell with no point
    if cells > 2:
        t[2] = -np.inf
        t[2, R // 2] = -7.25                                  # ... with one
    if cells > 3:
        t[3] = np.round(t[3] / 100.0)                         # ties: the smallest r wins
        t[3, -1] = t[3].max()
    if cells > 4:
        t[4, (2 * R) // 3] = np.nan
    if cells > 5:
        q[5, ::2] = -np.inf                                   # weights of zero: out of the marginal, still in the profile
    if cells > 6:
        t[6] = 12.5                                           # all equal
    return t, q


def chunks_of(cells, R):
    return sorted({c for c in (1, 7, 64, R - 1, R, R + 1, cells * R, cells * R + 5) if c >= 1})


def check_reduction(got, want):
    lm, prof, arg = got
    wlm, wprof, warg = want
    assert np.array_equal(prof, wprof, equal_nan=True)
    assert np.array_equal(arg, warg)
    fin = np.isfinite(wlm)
    assert np.array_equal(lm[~fin], wlm[~fin], equal_nan=True)
    err = np.abs(lm[fin] - wlm[fin]) / np.maximum(1.0, np.abs(wlm[fin]))
    assert np.all(err <= 1e-12), err.max()


@pytest.mark.parametrize('with_q', [False, True])
@pytest.mark.parametrize('R, cells', [(1, 7), (63, 5), (64, 7), (65, 3), (256, 2), (257, 4), (1000, 7), (1000, 1), (5000, 2)])
def test_reduction_against_numpy(ctx, R, cells, with_q):
    """R = 256 / 257: where a cell goes from one wave to a block of four; the chunk sizes make cells lie inside one chunk,
    straddle two and span many"""
    t, q = reduction_case(cells, R, 100 * R + cells)
    q = q if with_q else None
    want = numpy_reduce(t, q)
    for chunk in chunks_of(cells, R):
        got = ctx.selftest_grid_reduce(t, q, chunk)
        check_reduction(got, want)
        again = ctx.selftest_grid_reduce(t, q, chunk)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()


# ---- the whole path against the CPU oracle ---------------------------------------------------------------------------

CASES = [('d2_nonuniform', 1), ('c1_like', 1), ('d3_small', 0), ('d3_small', 2), ('unb_shape_2src', 1), ('bb_d2', 1)]
_oracle_cache = {}


def grid_of(c):
    """three variables -- a rate multiplier, a shape parameter, and a second shape parameter or rate multiplier -- with 5 x 7
    x 9 nodes: anchors, nodes outside the anchor box, a rate of zero"""
    d = c['d']
    g0 = np.asarray(c['model']['anchor_z'][0], dtype=float)
    span = g0[-1] - g0[0]
    # (the zero rate goes to a source whose absence leaves the likelihood dependent on every other variable: no exact ties)
    kind, index = [1, 0], [1 if c['name'].startswith('unb_') else 0, 0]
    nodes = [np.array([0.0, 0.6, 1.0, 1.25, 1.9]),
             np.array([g0[0] - 0.1 * span, g0[0], g0[0] + 0.37 * span, g0[len(g0) // 2], g0[0] + 0.81 * span, g0[-1], g0[-1] + 0.05 * span])]
    if d >= 2:
        g1 = np.asarray(c['model']['anchor_z'][1], dtype=float)
        kind.append(0)
        index.append(1)
        nodes.append(np.concatenate([np.linspace(g1[0], g1[-1], 7), [g1[-1] + 1.0, g1[0] + 0.3 * (g1[1] - g1[0])]]))
    else:
        kind.append(1)
        index.append(1)
        nodes.append(np.array([0.3, 0.7, 0.9, 1.0, 1.05, 1.2, 1.6, 2.4, 0.0]))
    return np.array(kind, dtype=np.int32), np.array(index, dtype=np.int32), nodes


def settings_of(c):
    z0 = np.array([0.5 * (g[0] + g[-1]) for g in c['model']['anchor_z']], dtype=float)
    scale0 = np.linspace(0.9, 1.1, c['S'])
    unit = np.linspace(1.0, 1.3, c['S'])
    return z0, scale0, unit


def oracle_grid(c):
    """ll of the oracle at every grid point [5, 7, 9]: -inf where the reference returns it, nan where one of its
    Beeston-Barlow assertions fires (the device reports those in the status word: excluded, as the -inf are)"""
    if c['name'] in _oracle_cache:
        return _oracle_cache[c['name']]
    kind, index, nodes = grid_of(c)
    z0, scale0, unit = settings_of(c)
    mesh = [m.ravel() for m in np.meshgrid(*nodes, indexing='ij')]
    z, rs = np.tile(z0, (len(mesh[0]), 1)), np.tile(scale0, (len(mesh[0]), 1))
    for k, i, m in zip(kind, index, mesh):
        if k == 0:
            z[:, i] = m
        else:
            rs[:, i] = m * unit[i]
    if c['name'].startswith('unb_'):
        ll = np.array([orc.loglikelihood_unbinned(c['model'], zz, rr, c['outlier']) for zz, rr in zip(z, rs)])
    else:
        ll = orc.loglikelihood_batch(c['model'], c['counts'], z, rs, bb_source=c['bb_source'] if c['bb_source'] >= 0 else None,
                                     allow_negative=c['allow_negative'])
    ll = np.where(np.isnan(ll), -np.inf, ll).reshape([len(v) for v in nodes])
    ll.setflags(write=False)
    _oracle_cache[c['name']] = ll
    return ll


def additive_terms(nodes, seed):
    rng = np.random.default_rng(seed)
    term = [rng.normal(0.0, 1.5, len(v)) for v in nodes]
    term[1][4] = -np.inf                                      # a prior of zero at one node
    logw = [rng.normal(0.0, 1.0, len(v)) for v in nodes]
    logw[2][3] = -np.inf                                      # a weight of zero at one node
    return term, logw


def reference(ll, nodes, n_keep, term, logw):
    """-> (log_marginal, profile, argmax, excluded, scale [K]: max finite |ll| of the cell, sure [K]: the oracle's best is
    clear of its runner-up)"""
    shapes = [len(v) for v in nodes]
    p = np.zeros(shapes)
    q = np.zeros(shapes)
    for j in range(len(nodes)):
        view = [1] * len(nodes)
        view[j] = -1
        if term is not None:
            p = p + term[j].reshape(view)
        if logw is not None and j >= n_keep:
            q = q + logw[j].reshape(view)
    K = int(np.prod(shapes[:n_keep]))
    gone = (ll == -np.inf) | (p == -np.inf)
    with np.errstate(invalid='ignore'):
        t = np.where(gone, -np.inf, ll + p).reshape(K, -1)
        u = t + q.reshape(K, -1)
    lls = np.where(gone, np.nan, ll).reshape(K, -1)
    lm, prof, arg, scale, sure = np.empty(K), np.empty(K), np.empty(K, dtype=np.int64), np.ones(K), np.ones(K, dtype=bool)
    for k in range(K):
        ok = t[k] > -np.inf
        if not ok.any():
            lm[k], prof[k], arg[k] = -np.inf, -np.inf, -1
            continue
        lm[k] = logsumexp(u[k][ok]) if np.any(u[k][ok] > -np.inf) else -np.inf
        prof[k] = t[k][ok].max()
        arg[k] = np.flatnonzero(t[k] == prof[k])[0]
        scale[k] = max(1.0, np.nanmax(np.abs(lls[k])))
        rest = np.delete(t[k], arg[k])
        sure[k] = rest.max(initial=-np.inf) < prof[k] - 4e-10 * max(1.0, abs(prof[k]))
    return lm, prof, arg, int(gone.sum()), scale, sure


@pytest.mark.parametrize('name, sparse', CASES)
def test_whole_path_against_the_oracle(name, sparse):
    """log_marginal and profile within 2e-10 max(1, max finite |ll| of the cell) -- twice the per-point parity bound, once
    for the point and once for the sums around it --, the excluded count and the empty cells exactly, argmax wherever the
    oracle's best is clear of its runner-up by 4e-10 max(1, |best|) (at most 10 % of the cells are not)"""
    from blueice_amd.exceptions import PlannerRefused
    c = load_case(name)
    dev = make_ctx(c, sparse)
    try:
        kind, index, nodes = grid_of(c)
        z0, scale0, unit = settings_of(c)
        ll = oracle_grid(c)
        term, logw = additive_terms(nodes, 5)
        ran = 0
        for n_keep, use_term, use_logw, chunk in ((0, False, False, 0), (1, True, True, 100), (3, True, False, 0), (1, False, True, 64),
                                                  (2, True, True, 0)):
            tm, lw = (term if use_term else None), (logw if use_logw else None)
            try:
                lm, prof, arg, counters = dev.grid_reduce(kind, index, z0, scale0, unit, None, n_keep, nodes, term=tm, logw=lw, chunk=chunk)
            except PlannerRefused as e:
                assert name == 'bb_d2' and 'exact totals' in str(e)          # the one refusal this list may meet
                continue
            ran += 1
            wlm, wprof, warg, excluded, scale, sure = reference(ll, nodes, n_keep, tm, lw)
            K = len(wlm)
            assert lm.shape == prof.shape == arg.shape == (1, K)
            lm, prof, arg = lm[0], prof[0], arg[0]
            assert counters[1] == 315 and counters[0] == -(-315 // (chunk or 315)) and counters[2] == excluded and counters[3] >= counters[0]
            for got, want in ((lm, wlm), (prof, wprof)):
                fin = np.isfinite(want)
                assert np.array_equal(got[~fin], want[~fin])
                err = np.abs(got[fin] - want[fin]) / scale[fin]
                print('%s n_keep=%d term=%s logw=%s: max error %.3g of the bound' % (name, n_keep, use_term, use_logw, err.max(initial=0.0) / 2e-10))
                assert np.all(err <= 2e-10)
            assert np.count_nonzero(~sure) <= 0.1 * K
            assert np.array_equal(arg[sure], warg[sure]) and np.all((arg >= 0) == (warg >= 0))
        assert ran > 0 or name == 'bb_d2'
    finally:
        dev.close()


def test_chunks_agree():
    c = load_case('c1_like')
    dev = make_ctx(c)
    try:
        kind, index, nodes = grid_of(c)
        z0, scale0, unit = settings_of(c)
        term, logw = additive_terms(nodes, 9)
        for n_keep in (0, 1, 2):
            runs = [dev.grid_reduce(kind, index, z0, scale0, unit, None, n_keep, nodes, term=term, logw=logw, chunk=chunk)
                    for chunk in (1, 7, 100, 315, 4096)]
            lm0, prof0, arg0, _ = runs[-1]
            for chunk, (lm, prof, arg, counters) in zip((1, 7, 100, 315, 4096), runs):
                assert counters[0] == -(-315 // min(chunk, 315)) and counters[1] == 315
                assert np.array_equal(prof, prof0) and np.array_equal(arg, arg0)
                fin = np.isfinite(lm0)
                assert np.array_equal(lm[~fin], lm0[~fin])
                assert np.all(np.abs(lm[fin] - lm0[fin]) <= 1e-12 * np.abs(lm0[fin]))
            again = dev.grid_reduce(kind, index, z0, scale0, unit, None, n_keep, nodes, term=term, logw=logw, chunk=7)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], runs[1][:3]))
    finally:
        dev.close()


def test_argument_errors():
    c = load_case('c1_like')
    dev = make_ctx(c)
    try:
        kind, index, nodes = grid_of(c)
        z0, scale0, unit = settings_of(c)
        call = lambda **kw: dev.grid_reduce(kw.pop('kind', kind), kw.pop('index', index), z0, scale0, unit, kw.pop('dataset', None),
                                            kw.pop('n_keep', 1), kw.pop('nodes', nodes), **kw)
        bad = lambda j, v: [np.array(v, dtype=float) if i == j else n for i, n in enumerate(nodes)]
        one = [np.zeros(1)]
        for kwargs, match in [(dict(kind=kind[:0], index=index[:0], nodes=[]), '1 <= F <= 16'),
                              (dict(kind=np.ones(17, dtype=np.int32), index=np.zeros(17, dtype=np.int32), nodes=one * 17), '1 <= F <= 16'),
                              (dict(n_keep=-1), 'n_keep'), (dict(n_keep=4), 'n_keep'),
                              (dict(nodes=bad(1, [])), 'at least 1'),
                              (dict(nodes=bad(2, [0.0, np.inf])), 'not finite'), (dict(nodes=bad(0, [np.nan])), 'not finite'),
                              (dict(term=bad(0, [0.0, np.inf, 0.0, 0.0, 0.0])), 'finite or -inf'),
                              (dict(logw=bad(0, [0.0, np.nan, 0.0, 0.0, 0.0])), 'finite or -inf'),
                              (dict(kind=kind[:2], index=index[:2], n_keep=2, nodes=[np.zeros(4097), np.zeros(4097)]), '2\\^24 cells'),
                              (dict(chunk=-1), 'chunk'), (dict(chunk=2 ** 26 + 1), 'chunk'),
                              (dict(kind=np.array([1, 0, 2], dtype=np.int32)), 'neither a shape parameter nor a rate multiplier'),
                              (dict(index=np.array([0, 5, 1], dtype=np.int32)), 'neither a shape parameter nor a rate multiplier'),
                              (dict(kind=np.array([1, 0, 1], dtype=np.int32), index=np.array([0, 0, 0], dtype=np.int32)), 'same parameter'),
                              (dict(dataset=[3]), 'dataset 3 of entry 0')]:
            with pytest.raises(ValueError, match=match):
                call(**kwargs)
        lm, prof, arg, counters = call()                            # the context still works
        assert counters[1] == 315 and np.all(np.isfinite(lm))
    finally:
        dev.close()


# ---- lf.grid_scan ----------------------------------------------------------------------------------------------------

def zoo_lf(seed=8, S=2, n_data=300):
    import model_zoo
    ns = model_zoo.namespace_of('blueice_amd')
    space = [('x', np.linspace(0, 1, 13)), ('y', np.linspace(0, 1, 9))]
    return model_zoo.morph_lf(ns, np.random.default_rng(seed), S, space, OrderedDict(shift=(-1., 0., 1.)), 4000, n_data)


def close(a, b, scale, bound=2e-10):
    fin = np.isfinite(b)
    return np.array_equal(a[~fin], b[~fin], equal_nan=True) and np.all(np.abs(a[fin] - b[fin]) <= bound * np.maximum(1.0, np.abs(scale[fin])))


def test_datasets_in_one_call_equal_single_calls():
    lf = zoo_lf()
    lf.simulate_toys(8, seed=12)
    axes = dict(keep=[('s0_rate_multiplier', np.linspace(0.0, 2.0, 5))],
                reduce=[('shift', np.linspace(-1.2, 1.0, 7)), ('s1_rate_multiplier', np.linspace(0.5, 1.5, 9))])
    joint = lf.grid_scan(datasets=np.arange(8), **axes)
    assert joint.engine == 'native' and joint.profile.shape == (8, 5) and joint.counters[1] == 8 * 315
    excluded = 0
    for e in range(8):
        solo = lf.grid_scan(datasets=[e], **axes)
        assert solo.engine == 'native' and solo.profile.shape == (1, 5)
        assert np.array_equal(solo.profile[0], joint.profile[e]) and np.array_equal(solo.argmax[0], joint.argmax[e])
        assert np.all(np.abs(solo.log_marginal[0] - joint.log_marginal[e]) <= 1e-12 * np.abs(joint.log_marginal[e]))
        for name in ('shift', 's1_rate_multiplier'):
            assert np.array_equal(solo.best[name][0], joint.best[name][e])
        excluded += solo.excluded
    assert excluded == joint.excluded >= 8 * 5 * 9                    # at least the nodes at shift = -1.2
    assert not np.array_equal(joint.profile[0], joint.profile[1])


def test_engines_agree_with_priors():
    """a GaussianPrior on a rate, a plain callable on the shape parameter (zero below -0.9), a callable on a fixed rate: the
    native engine takes every callable prior (evaluated at the nodes); native and host agree to the per-point parity bound"""
    from scipy import stats
    from blueice_amd.likelihood import LogLikelihoodSum
    from blueice_amd.priors import GaussianPrior
    lf = zoo_lf(S=3)
    lf.rate_parameters['s1'] = GaussianPrior(1.0, 0.2)
    lf.rate_parameters['s2'] = stats.norm(1.0, 0.5).logpdf
    anchors, _, base = lf.shape_parameters['shift']
    lf.shape_parameters['shift'] = (anchors, lambda x: np.where(x < -0.9, -np.inf, -0.5 * (x / 0.4) ** 2), base)
    axes = dict(keep=[('s0_rate_multiplier', np.linspace(-0.5, 2.0, 6))],
                reduce=[('shift', np.linspace(-1.0, 1.0, 9)), ('s1_rate_multiplier', np.linspace(0.4, 1.6, 7))], s2_rate_multiplier=1.2)
    for weights, chunk in (('trapezoid', None), (None, 50)):
        nat = lf.grid_scan(weights=weights, chunk=chunk, engine='native', **axes)
        host = lf.grid_scan(weights=weights, chunk=chunk, engine='host', **axes)
        auto = lf.grid_scan(weights=weights, chunk=chunk, **axes)
        assert nat.engine == auto.engine == 'native' and host.engine == 'host'
        assert nat.counters[1] == host.counters[1] == 6 * 9 * 7 and nat.excluded == host.excluded >= 9 * 7 + 5 * 7
        scale = np.abs(host.profile)
        assert close(nat.profile, host.profile, scale) and close(nat.log_marginal, host.log_marginal, scale)
        assert np.array_equal(nat.argmax, host.argmax)
        assert np.array_equal(auto.profile, nat.profile) and np.array_equal(auto.log_marginal, nat.log_marginal)
        assert all(np.array_equal(nat.best[k], host.best[k], equal_nan=True) for k in host.best)
        assert nat.profile[0] == -np.inf and nat.argmax[0] == -1 and np.isnan(nat.best['shift'][0])     # a negative rate: no point left
    assert 0.0 < nat.credible_upper_limit(0.9) < 2.0
    # a sum is not one device context: host engine, and a refusal where the native one is asked for
    both = LogLikelihoodSum([lf, zoo_lf(seed=9, S=3)])
    res = both.grid_scan(**axes)
    assert res.engine == 'host' and np.all(np.isfinite(res.profile[2:]))
    with pytest.raises(ValueError, match="engine='host'"):
        both.grid_scan(engine='native', **axes)


def test_profile_against_fits():
    """the grid profile never lies above the fitted profile (by more than 1e-7 |ll|), and reaches it when the fitted
    nuisances are among the reduce nodes"""
    from blueice_amd.profile import bestfit_batched
    lf = zoo_lf(seed=21)
    pts = np.array([0.4, 0.8, 1.0, 1.3, 1.9])
    best, ll = bestfit_batched(lf, points={'s0_rate_multiplier': pts})
    coarse = lf.grid_scan(keep=[('s0_rate_multiplier', pts)], weights=None,
                          reduce=[('s1_rate_multiplier', np.linspace(0.2, 2.0, 19)), ('shift', np.linspace(-1.0, 1.0, 21))])
    assert coarse.engine == 'native'
    print('fitted - grid profile (coarse):', ll - coarse.profile)
    assert np.all(coarse.profile <= ll + 1e-7 * np.abs(ll))
    fine = lf.grid_scan(keep=[('s0_rate_multiplier', pts)], weights=None,
                        reduce=[('s1_rate_multiplier', np.unique(np.concatenate([np.linspace(0.2, 2.0, 19), best['s1_rate_multiplier']]))),
                                ('shift', np.unique(np.concatenate([np.linspace(-1.0, 1.0, 21), best['shift']])))])
    print('fitted - grid profile (with the fitted nodes):', ll - fine.profile)
    assert np.all(fine.profile <= ll + 1e-7 * np.abs(ll)) and np.all(fine.profile >= ll - 2e-10 * np.maximum(1.0, np.abs(ll)))
    assert np.all(fine.profile >= coarse.profile)
