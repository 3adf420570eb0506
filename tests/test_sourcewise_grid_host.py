"""Gridded likelihoods of source-wise models without a GPU: the library cross-compiles with the scan planner's translation unit, the
header, the ctypes binding and the bound methods agree, blueice_amd.grid.grid_scan reaches the context's grid_reduce with the
variable map, nodes, terms and route it should (over a recording context in SourceWiseContext's place), the host engine gives the
same GridResult, and the bound lf.grid_scan stays refused."""
import inspect
import os
import re

import numpy as np
import pytest

from test_sourcewise_sampler_host import RecordingSamplerContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bi_eval_sourcewise_scan', 'bi_grid_reduce_sourcewise')


def test_header_binding_and_methods_agree():
    import ctypes as C
    from blueice_amd import _capi, build
    from blueice_amd.device import DeviceContext
    from blueice_amd.source_wise import SourceWiseBinnedLogLikelihood, SourceWiseContext
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert 'tu_sourcewise_scan' in build.UNITS and os.path.exists(os.path.join(build.CSRC, 'tu_sourcewise_scan.hip'))
    for header in ('bi_k_sourcewise_scan.h', 'bi_sourcewise_scan.h'):
        assert os.path.exists(os.path.join(build.CSRC, header))
    build.build()                                             # cross-compiles for gfx950 with the new unit
    lib = _capi.load()
    for s in NEW:
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text)
        assert proto, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.group(1).split(',') if a.strip()]), s
    # bi_eval_sourcewise_planned's arguments and the counters; bi_grid_reduce's arguments with `route` behind `chunk`
    planned, grid = _capi.SIGNATURES['bi_eval_sourcewise_planned'], _capi.SIGNATURES['bi_grid_reduce']
    assert _capi.SIGNATURES['bi_eval_sourcewise_scan'] == (planned[0], planned[1] + [C.c_void_p])
    assert _capi.SIGNATURES['bi_grid_reduce_sourcewise'] == (grid[0], grid[1][:15] + [C.c_int] + grid[1][15:])
    one, i32 = np.ones(8), np.zeros(8, dtype=np.int32)
    p = _capi.ptr
    assert lib.bi_eval_sourcewise_scan(None, 1, p(one), None, None, p(one.copy()), None, None) == _capi.ERR_INVALID
    assert lib.bi_grid_reduce_sourcewise(None, 1, None, 1, 0, p(i32), p(i32), p(one), p(one), p(one), p(np.ones(1, dtype=np.int32)), p(one), None,
                                         None, 0, -1, p(one.copy()), p(one.copy()), p(np.zeros(8, dtype=np.int64)), None) == _capi.ERR_INVALID
    want = list(inspect.signature(DeviceContext.grid_reduce).parameters)
    assert list(inspect.signature(SourceWiseContext.grid_reduce).parameters) == want + ['route']
    assert list(inspect.signature(SourceWiseContext.eval_scan).parameters) == list(inspect.signature(SourceWiseContext.eval).parameters)
    assert list(inspect.signature(SourceWiseBinnedLogLikelihood.eval_points_scan).parameters) == \
        list(inspect.signature(SourceWiseBinnedLogLikelihood.eval_points).parameters)
    assert 'eval_points_scan' not in SourceWiseBinnedLogLikelihood._REFUSED and 'grid_scan' in SourceWiseBinnedLogLikelihood._REFUSED


def fake_ll(z, rs):
    return -np.sum((z - 0.2) ** 2, axis=1) - 3.0 * np.sum((rs - 1.1) ** 2, axis=1)


class RecordingGridContext(RecordingSamplerContext):
    """... with an `eval` and an `eval_scan` that answer with a smooth function of the point (-inf below z_0 = -1.5, as a point
    outside the box), and a `grid_reduce` that records its arguments and reduces that function over the grid in NumPy"""

    def eval(self, z, rate_scale=None, dataset=None):
        self.calls.append(('eval', len(rate_scale)))
        ll = fake_ll(np.asarray(z), np.asarray(rate_scale)) + (0.0 if dataset is None else 0.5 * np.asarray(dataset))
        st = (np.asarray(z)[:, 0] < -1.5).astype(np.int32)
        return np.where(st != 0, -np.inf, ll), st

    def eval_scan(self, z, rate_scale=None, dataset=None):
        ll, st = self.eval(z, rate_scale, dataset)
        self.calls[-1] = ('eval_scan', len(rate_scale))
        return ll, st

    def grid_reduce(self, kind, index, z0, scale0, unit, dataset, n_keep, nodes, term=None, logw=None, chunk=0, route=-1):
        from blueice_amd.grid import reduce_cells
        self.calls.append(('grid_reduce', dict(kind=kind, index=index, z0=z0, scale0=scale0, unit=unit, dataset=dataset, n_keep=n_keep,
                                               nodes=nodes, term=term, logw=logw, chunk=chunk, route=route)))
        shape = tuple(len(v) for v in nodes)
        E = 1 if dataset is None else len(dataset)
        GK, R = int(np.prod(shape)), int(np.prod(shape[n_keep:]))
        t, q = np.empty((E, GK)), np.zeros(GK)
        at = np.unravel_index(np.arange(GK), shape)
        for e in range(E):
            z, rs = np.tile(np.asarray(z0)[e % len(z0)], (GK, 1)), np.tile(np.asarray(scale0)[e % len(scale0)], (GK, 1))
            p = np.zeros(GK)
            for j, i in enumerate(at):
                if kind[j] == 0:
                    z[:, index[j]] = nodes[j][i]
                else:
                    rs[:, index[j]] = nodes[j][i] * np.asarray(unit)[e % len(unit)][index[j]]
                if term is not None:
                    p = p + term[j][i]
            ll = fake_ll(z, rs) + (0.0 if dataset is None else 0.5 * dataset[e])
            t[e] = np.where(z[:, 0] < -1.5, -np.inf, ll + p)
        for j, i in enumerate(at):
            if logw is not None and j >= n_keep:
                q = q + logw[j][i]
        lm, prof, arg, excluded = reduce_cells(t.reshape(-1, R), np.tile(q, E).reshape(-1, R))
        return lm.reshape(E, -1), prof.reshape(E, -1), arg.reshape(E, -1), np.array([1, E * GK, excluded, 1, max(route, 0)])


@pytest.fixture
def recorded(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd.priors import GaussianPrior
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingGridContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.25) if s == 2 else None)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.) if n in (names[0], names[1]) else None)
    lf.prepare()
    lf.set_binned_data(np.ones((3, 6, 5)))
    return lf, names


def axes_of(names):
    return dict(keep=[('s0_rate_multiplier', np.linspace(0.0, 2.0, 5))],
                reduce=[(names[0], np.linspace(-1.8, 1.8, 7)), ('s2_rate_multiplier', np.linspace(0.5, 1.5, 4))], datasets=[2, 0])


def test_grid_scan_reaches_the_context(recorded):
    from blueice_amd import grid
    from blueice_amd.profile import BatchObjective
    lf, names = recorded
    fixed = {names[1]: 0.5, 's3_rate_multiplier': 1.5}
    axes = axes_of(names)
    res = grid.grid_scan(lf, engine='native', chunk=50, **axes, **fixed)
    assert res.engine == 'native' and res.profile.shape == res.log_marginal.shape == res.argmax.shape == (2, 5)
    (what, got), = lf.ctx.calls
    assert what == 'grid_reduce' and got['route'] == grid.SOURCEWISE_AUTO_ROUTE and got['chunk'] == 50 and got['n_keep'] == 1
    assert list(got['kind']) == [1, 0, 1] and list(got['index']) == [0, 0, 2] and list(got['dataset']) == [2, 0]
    native = BatchObjective(lf, ['s0_rate_multiplier', names[0], 's2_rate_multiplier'], {}, fixed, None, np.array([2, 0])).native()
    for key in ('z0', 'scale0', 'unit'):
        assert np.array_equal(np.broadcast_to(got[key], native[key].shape), native[key]), key
    for v, (_, w) in zip(got['nodes'], axes['keep'] + axes['reduce']):
        assert np.array_equal(v, w)
    # the priors at the nodes: none on s0, the Gaussians of names[0] and s2; the fixed names[1]'s prior is the constant
    t0, t1, t2 = got['term']
    assert not t0.any() and np.array_equal(t1, lf.shape_parameters[names[0]][1](axes['reduce'][0][1]))
    assert np.array_equal(t2, lf.rate_parameters['s2'](axes['reduce'][1][1]))
    w0, w1, w2 = got['logw']
    assert not w0.any() and np.array_equal(w1, np.log(grid.trapezoid_weights(axes['reduce'][0][1])))
    const = float(lf.shape_parameters[names[1]][1](np.array([0.5]))[0])
    lf.ctx.calls.clear()

    # the host engine: the same GridResult from eval_points in chunks and reduce_cells
    host = grid.grid_scan(lf, engine='host', chunk=50, **axes, **fixed)
    assert host.engine == 'host' and all(c[0] == 'eval' for c in lf.ctx.calls) and len(lf.ctx.calls) == -(-2 * 5 * 7 * 4 // 50)
    assert np.allclose(res.profile, host.profile, rtol=1e-13, atol=0) and np.allclose(res.log_marginal, host.log_marginal, rtol=1e-13, atol=0)
    assert np.array_equal(res.argmax, host.argmax) and res.excluded == host.excluded == 2 * 5 * 4
    assert all(np.array_equal(res.best[k], host.best[k]) for k in host.best) and set(host.best) == {names[0], 's2_rate_multiplier'}
    assert abs(const) > 0 and np.allclose(res.credible_upper_limit(0.9), host.credible_upper_limit(0.9), rtol=1e-12)
    lf.ctx.calls.clear()

    # no engine named: native
    assert grid.grid_scan(lf, **axes).engine == 'native' and lf.ctx.calls[0][0] == 'grid_reduce'


def test_the_config_key_names_the_route(recorded):
    from blueice_amd import grid
    lf, names = recorded
    axes = axes_of(names)
    for setting, route in (('points', 0), ('scan', 1), ('auto', grid.SOURCEWISE_AUTO_ROUTE)):
        lf.config['sourcewise_grid_route'] = setting
        lf.ctx.calls.clear()
        assert grid.grid_scan(lf, engine='native', **axes).engine == 'native'
        assert lf.ctx.calls[0][1]['route'] == route
    assert grid.SOURCEWISE_AUTO_ROUTE in (-1, 0)
    for bad in ('fast', 1, None):
        lf.config['sourcewise_grid_route'] = bad
        with pytest.raises(ValueError, match="sourcewise_grid_route.*'auto', 'points' or 'scan'"):
            grid.grid_scan(lf, **axes)
    lf.config['sourcewise_grid_route'] = 'auto'
    # what keeps a likelihood off the native engine keeps this one off it too
    lf.config['unphysical_behaviour'] = 'error'
    assert grid.grid_scan(lf, **axes).engine == 'host'
    with pytest.raises(ValueError, match="engine='host'"):
        grid.grid_scan(lf, engine='native', **axes)


def test_the_bound_name_stays_refused_and_eval_points_scan_is_bound(recorded):
    import blueice_amd.source_wise as sw
    lf, names = recorded
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.grid_scan()
    assert 'the ensemble sampler' in str(e.value) and 'gridded likelihoods' in str(e.value)
    assert 'blueice_amd.grid.grid_scan(lf, ...)' in str(e.value)
    assert not lf.ctx.calls
    assert 'bi_grid_reduce_sourcewise' in sw.__doc__ and 'bi_eval_sourcewise_scan' in sw.__doc__ and 'grids (grid_scan)' not in sw.__doc__
    out = lf.eval_points_scan({names[0]: np.array([-1.8, 0.0, 0.7]), 's1_rate_multiplier': 1.2}, dataset=np.array([0, 1, 2]))
    assert lf.ctx.calls == [('eval_scan', 3)] and out.shape == (3,) and np.all(np.isfinite(out[1:]))
    ref = lf.eval_points({names[0]: np.array([-1.8, 0.0, 0.7]), 's1_rate_multiplier': 1.2}, dataset=np.array([0, 1, 2]))
    assert np.array_equal(out, ref) and ref[0] == -np.inf
