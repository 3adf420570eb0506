"""Gridded likelihoods of source-wise models on the device (bi_grid_reduce_sourcewise): both routes of the evaluation step, the
likelihood layer (blueice_amd.grid.grid_scan on a prepared SourceWiseBinnedLogLikelihood) and the argument errors.

route 0 (points): log_marginal, profile and argmax equal blueice_amd.grid.reduce_cells over ctx.eval_planned of the same points bit
for bit when one chunk covers the grid (and the reduction kernels on those values, bi_selftest_grid_reduce, bit for bit); chunks
that split cells agree to test_grid_gpu.close's bound with equal argmax.
route 1 (scan): against the long-double NumPy reduction of the expanded-grid oracle's values at test_grid_gpu's whole-path bound,
2e-10 max(1, max finite |ll| of the cell)."""
import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_nonempty_oracle as no
import sourcewise_toy_cases as toy_cases
from test_grid_gpu import close
from test_sourcewise_nonempty_gpu import built, expanded_oracle, nuisance_lf
from test_sourcewise_sampler_gpu import bits

pytestmark = pytest.mark.gpu

B = 1027                                    # three tiles, the last of three bins
KIND, INDEX = np.array([1, 0, 1], dtype=np.int32), np.array([0, 0, 1], dtype=np.int32)      # rate of source 0 | axis 0, rate of source 1
N_KEEP = 1


@pytest.fixture(scope='module')
def case():
    """toy_cases' small geometry -- (3, 2, 4) anchors, sources owning (0,), (1, 2) and nothing -- at B = 1027 with two sparse toys;
    the grid: 2 kept nodes x 5 x 4 reduced nodes, one node of axis 0 below its first anchor"""
    rng = np.random.default_rng(2024)
    model = fo.random_model(rng, toy_cases.N_ANCHOR, toy_cases.OWN, B)
    counts = np.stack([no.sparse_counts(rng, B, 300), no.sparse_counts(rng, B, 40)])
    g = model['anchor_z']
    nodes = [np.array([0.7, 1.3]), np.array([g[0][0] - 0.5, g[0][0], 0.5 * (g[0][0] + g[0][1]), g[0][1], g[0][2]]),
             np.array([0.5, 0.9, 1.2, 1.6])]
    term = [rng.normal(0.0, 1.5, len(v)) for v in nodes]
    logw = [rng.normal(0.0, 1.0, len(v)) for v in nodes]
    term[2][1] = -np.inf                                    # a prior of zero at one node
    logw[1][3] = -np.inf                                    # a weight of zero at one node
    z0 = np.array([[0.0, 0.5 * (g[1][0] + g[1][1]), 0.3 * g[2][0] + 0.7 * g[2][2]]] * 2)
    z0[1, 2] = g[2][3]                                      # entry 1: on the upper edge of axis 2
    scale0 = np.array([[1.0, 1.0, 0.8], [1.0, 1.0, 1.1]])
    unit = np.array([[1.0, 1.1, 1.0], [0.9, 1.0, 1.0]])
    datasets = np.array([1, 0], dtype=np.int64)
    return dict(model=model, counts=counts, nodes=nodes, term=term, logw=logw, z0=z0, scale0=scale0, unit=unit, datasets=datasets)


def grid_points(c):
    """the grid's points in the library's order, g = (e K + k) R + r with variable 0 slowest -> z, rs, ds, p [G], q [G]; p and q
    are summed as the header states: variables ascending from 0.0, every addition rounded on its own"""
    nodes = c['nodes']
    shape = tuple(len(v) for v in nodes)
    E, GK = len(c['datasets']), int(np.prod(shape))
    z, rs, ds, p, q = [], [], [], [], []
    for e in range(E):
        for g in range(GK):
            at = np.unravel_index(g, shape)
            zz, rr = c['z0'][e].copy(), c['scale0'][e].copy()
            pp = qq = 0.0
            for j, i in enumerate(at):
                if KIND[j] == 0:
                    zz[INDEX[j]] = nodes[j][i]
                else:
                    rr[INDEX[j]] = nodes[j][i] * c['unit'][e][INDEX[j]]
                pp = pp + c['term'][j][i]
                if j >= N_KEEP:
                    qq = qq + c['logw'][j][i]
            z.append(zz), rs.append(rr), ds.append(c['datasets'][e]), p.append(pp), q.append(qq)
    return np.array(z), np.array(rs), np.array(ds, dtype=np.int64), np.array(p), np.array(q)


def longdouble_reduce(t, q):
    """-> (log_marginal, profile, argmax, excluded) of t [cells, R] (-inf: excluded), q [cells, R], the sums in long double"""
    cells, R = t.shape
    lm, prof, arg = np.empty(cells), np.empty(cells), np.empty(cells, dtype=np.int64)
    for k in range(cells):
        ok = t[k] > -np.inf
        if not ok.any():
            lm[k], prof[k], arg[k] = -np.inf, -np.inf, -1
            continue
        prof[k] = t[k][ok].max()
        arg[k] = np.flatnonzero(t[k] == prof[k])[0]
        u = (t[k].astype(np.longdouble) + q[k].astype(np.longdouble))[ok]
        u = u[u > -np.inf]
        lm[k] = float(u.max() + np.log(np.sum(np.exp(u - u.max())))) if len(u) else -np.inf
    return lm, prof, arg, int((t == -np.inf).sum())


def run(ctx, c, route, chunk=0):
    return ctx.grid_reduce(KIND, INDEX, c['z0'], c['scale0'], c['unit'], c['datasets'], N_KEEP, c['nodes'], term=c['term'], logw=c['logw'],
                           chunk=chunk, route=route)


@pytest.mark.parametrize('form', ['dense', 'nonempty'])
def test_route_points(case, form):
    from blueice_amd.grid import reduce_cells
    c = case
    ctx = toy_cases.upload(c['model'], c['counts'])
    try:
        if form == 'nonempty':
            built(ctx, [300, 40])
        z, rs, ds, p, q = grid_points(c)
        ll, st = ctx.eval_planned(z, rs, ds)
        assert set(np.unique(st)) == {0, 1} and np.count_nonzero(st) == 2 * 2 * 4
        with np.errstate(invalid='ignore'):
            t = np.where((st != 0) | (ll == -np.inf) | (p == -np.inf), -np.inf, ll + p).reshape(4, 20)
        wlm, wprof, warg, wexcl = reduce_cells(t, q.reshape(4, 20))
        klm, kprof, karg = ctx._dev.selftest_grid_reduce(t, q.reshape(4, 20))
        lm, prof, arg, counters = run(ctx, c, 0)
        assert lm.shape == prof.shape == arg.shape == (2, 2) and list(counters) == [1, 80, wexcl, counters[3], 0] and counters[3] >= 3
        assert wexcl == 2 * 2 * 4 + 2 * 2 * 4 and np.all(warg >= 0)
        assert np.array_equal(bits(prof.ravel()), bits(wprof)) and np.array_equal(arg.ravel(), warg)
        assert np.array_equal(bits(prof.ravel()), bits(kprof)) and np.array_equal(arg.ravel(), karg)
        assert np.array_equal(bits(lm.ravel()), bits(klm))
        ulp = np.abs(lm.ravel() - wlm) / np.spacing(np.abs(wlm))
        print('%s: log_marginal against NumPy reduce_cells: %s ulp' % (form, ulp))
        assert np.array_equal(bits(lm.ravel()), bits(wlm))
        again = run(ctx, c, 0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (lm, prof, arg)))
        scale = np.abs(wprof).reshape(2, 2)
        for chunk in (7, 64, 80, 1000):
            lm2, prof2, arg2, counters2 = run(ctx, c, 0, chunk)
            assert counters2[0] == -(-80 // min(chunk, 80)) and list(counters2[1:3]) == [80, wexcl] and counters2[4] == 0
            assert close(prof2, prof, scale) and close(lm2, lm, scale) and np.array_equal(arg2, arg)
            if chunk >= 80:
                assert all(a.tobytes() == b.tobytes() for a, b in zip((lm2, prof2, arg2), (lm, prof, arg)))
        # route -1 without the form is route 0; with it, the scan route
        auto = run(ctx, c, -1)
        assert auto[3][4] == (1 if form == 'nonempty' else 0)
        if form == 'dense':
            assert all(a.tobytes() == b.tobytes() for a, b in zip(auto[:3], (lm, prof, arg)))
            with pytest.raises(ValueError, match='bi_grid_reduce_sourcewise.*bi_sourcewise_build_nonempty'):
                run(ctx, c, 1)
    finally:
        ctx.close()


def test_route_scan(case):
    c = case
    ctx = toy_cases.upload(c['model'], c['counts'])
    try:
        built(ctx, [300, 40])
        z, rs, ds, p, q = grid_points(c)
        oracle = expanded_oracle(c['model'])
        g0 = c['model']['anchor_z'][0]
        inside = (z[:, 0] >= g0[0]) & (z[:, 0] <= g0[-1])
        ll = np.array([oracle(z[i], rs[i], c['counts'][ds[i]])['ll'] if inside[i] else -np.inf for i in range(len(z))])
        with np.errstate(invalid='ignore'):
            t = np.where((ll == -np.inf) | (p == -np.inf), -np.inf, ll + p).reshape(4, 20)
        wlm, wprof, warg, wexcl = longdouble_reduce(t, q.reshape(4, 20))
        scale = np.array([np.abs(ll.reshape(4, 20)[k][np.isfinite(ll.reshape(4, 20)[k])]).max() for k in range(4)]).reshape(2, 2)
        before = ctx.get_param('n_scan_launches')
        for chunk in (0, 33):
            lm, prof, arg, counters = run(ctx, c, 1, chunk)
            assert list(counters[:3]) == [-(-80 // (chunk or 80)), 80, wexcl] and counters[4] == 1 and wexcl == 32
            for got, want, what in ((lm, wlm, 'log_marginal'), (prof, wprof, 'profile')):
                err = np.abs(got - want.reshape(2, 2)) / np.maximum(1.0, scale)
                print('route scan, chunk %d, %s: max error %.3g of the bound' % (chunk, what, err.max() / 2e-10))
            assert close(lm, wlm.reshape(2, 2), scale) and close(prof, wprof.reshape(2, 2), scale)
            assert np.array_equal(arg, warg.reshape(2, 2))
            again = run(ctx, c, 1, chunk)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:3], (lm, prof, arg)))
        assert ctx.get_param('n_scan_launches') == before + 2 * (1 + 3)
        assert ctx.get_param('last_scan_groups') >= 2
    finally:
        ctx.close()


def test_through_the_likelihood():
    """blueice_amd.grid.grid_scan on a prepared source-wise model: the native engine on both routes against the host engine
    (eval_points in chunks, reduce_cells), with priors, two toys, and the credible limit"""
    from blueice_amd import grid
    lf, names = nuisance_lf(nonempty_bins=True, device_histograms=False)
    lf.simulate_toys_points({names[0]: np.array([0.3]), 's0_rate_multiplier': np.array([0.4])}, 2, seed=4)
    assert lf.ctx.get_param('sourcewise_nonempty_ready') == 1
    axes = dict(keep=[('s0_rate_multiplier', np.linspace(0.0, 3.0, 7))],
                reduce=[(names[0], np.linspace(-2.5, 2.0, 6)), ('s1_rate_multiplier', np.linspace(0.6, 1.4, 5))], datasets=[1, 0])
    axes[names[3]] = 0.25
    host = grid.grid_scan(lf, engine='host', **axes)
    assert host.engine == 'host' and host.excluded == 2 * 7 * 5
    scale = np.abs(host.profile)
    limits = {}
    for setting, route in (('points', 0), ('scan', 1), ('auto', None)):
        lf.config['sourcewise_grid_route'] = setting
        for chunk in (None, 50):
            nat = grid.grid_scan(lf, engine='native', chunk=chunk, **axes)
            assert nat.engine == 'native' and nat.counters[1] == 2 * 7 * 6 * 5 and nat.excluded == host.excluded
            assert route is None or nat.counters[4] == route
            assert close(nat.profile, host.profile, scale) and close(nat.log_marginal, host.log_marginal, scale)
            assert np.array_equal(nat.argmax, host.argmax)
            assert all(np.array_equal(nat.best[k], host.best[k], equal_nan=True) for k in host.best)
        limits[setting] = nat.credible_upper_limit(0.9)
    want = host.credible_upper_limit(0.9)
    for setting, got in limits.items():
        assert got.shape == (2,) and np.all(np.abs(got - want) <= 2e-10 * np.maximum(1.0, np.abs(want))), (setting, got, want)
    assert grid.grid_scan(lf, **axes).engine == 'native'
    with pytest.raises(NotImplementedError, match='blueice_amd.grid.grid_scan'):
        lf.grid_scan(**axes)
    pts = {names[0]: np.linspace(-1.5, 1.5, 40), 's1_rate_multiplier': np.linspace(0.6, 1.4, 40)}
    a, b = lf.eval_points_scan(pts), lf.eval_points(pts)
    assert np.all(np.abs(a - b) <= 2e-10 * np.maximum(1.0, np.abs(b)))
    lf.ctx.close()


def test_argument_errors(case):
    """the argument errors of bi_grid_reduce, under the new entry point's name"""
    c = case
    ctx = toy_cases.upload(c['model'], c['counts'])
    try:
        nodes = c['nodes']
        call = lambda **kw: ctx.grid_reduce(kw.pop('kind', KIND), kw.pop('index', INDEX), c['z0'][:1], c['scale0'][:1], c['unit'][:1],
                                            kw.pop('dataset', None), kw.pop('n_keep', 1), kw.pop('nodes', nodes), **kw)
        bad = lambda j, v: [np.array(v, dtype=float) if i == j else n for i, n in enumerate(nodes)]
        one = [np.zeros(1)]
        for kwargs, match in [(dict(kind=KIND[:0], index=INDEX[:0], nodes=[]), '1 <= F <= 16'),
                              (dict(kind=np.ones(17, dtype=np.int32), index=np.zeros(17, dtype=np.int32), nodes=one * 17), '1 <= F <= 16'),
                              (dict(n_keep=-1), 'n_keep'), (dict(n_keep=4), 'n_keep'),
                              (dict(nodes=bad(1, [])), 'at least 1'),
                              (dict(nodes=bad(2, [0.0, np.inf])), 'not finite'), (dict(nodes=bad(0, [np.nan])), 'not finite'),
                              (dict(term=bad(0, [0.0, np.inf])), 'finite or -inf'),
                              (dict(logw=bad(0, [0.0, np.nan])), 'finite or -inf'),
                              (dict(kind=KIND[:2], index=INDEX[:2], n_keep=2, nodes=[np.zeros(4097), np.zeros(4097)]), '2\\^24 cells'),
                              (dict(chunk=-1), 'chunk'), (dict(chunk=2 ** 26 + 1), 'chunk'),
                              (dict(kind=np.array([1, 0, 2], dtype=np.int32)), 'neither a shape parameter nor a rate multiplier'),
                              (dict(index=np.array([0, 5, 1], dtype=np.int32)), 'neither a shape parameter nor a rate multiplier'),
                              (dict(index=np.array([0, 0, 3], dtype=np.int32)), 'neither a shape parameter nor a rate multiplier'),
                              (dict(kind=np.array([1, 0, 1], dtype=np.int32), index=np.array([0, 0, 0], dtype=np.int32)), 'same parameter'),
                              (dict(dataset=[3]), 'dataset 3 of entry 0'),
                              (dict(route=2), 'route'), (dict(route=-2), 'route')]:
            with pytest.raises(ValueError, match='bi_grid_reduce_sourcewise.*' + match):
                call(**kwargs)
        lm, prof, arg, counters = call()                            # the context still works
        assert counters[1] == 40 and counters[4] == 0 and np.all(np.isfinite(lm))
    finally:
        ctx.close()
