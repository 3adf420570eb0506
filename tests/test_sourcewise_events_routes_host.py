"""The planner, the sampler and the gridded likelihood on the event store of a source-wise model, without a GPU: the library
cross-compiles, the header, the ctypes binding and the context methods agree on the three new symbols (signatures equal to their
binned siblings'), a NULL context is an error code, blueice_amd.sampler.sample_posterior, blueice_amd.inference.bestfit_emcee and
blueice_amd.grid.grid_scan reach `sample_stretch_events` and `grid_reduce_events` of a recording context with what
BatchObjective.native() and grid._native_plan give, and the bound names stay refused and name the function spellings."""
import inspect
import os
import re

import numpy as np
import pytest

from test_sourcewise_events_host import RecordingContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLINGS = {'bi_eval_sourcewise_events_planned': 'bi_eval_sourcewise_planned',
            'bi_sample_stretch_sourcewise_events': 'bi_sample_stretch_sourcewise',
            'bi_grid_reduce_sourcewise_events': 'bi_grid_reduce_sourcewise'}
METHODS = {'eval_events_planned': 'eval_planned', 'sample_stretch_events': 'sample_stretch', 'grid_reduce_events': 'grid_reduce'}


def test_header_binding_and_methods_agree():
    from blueice_amd import _capi, build
    from blueice_amd.source_wise import SourceWiseContext
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    build.build()                                             # cross-compiles for gfx950 with the planner's event variant
    lib = _capi.load()
    for s, sibling in SIBLINGS.items():
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text)
        assert proto, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.group(1).split(',') if a.strip()]), s
        assert _capi.SIGNATURES[s] == _capi.SIGNATURES[sibling], s
        # the same argument types in the header too, name for name
        strip = lambda args: [re.sub(r'\s+', ' ', a).strip() for a in args.split(',')]
        assert strip(proto.group(1)) == strip(re.search(r'\b%s\s*\(([^)]*)\)' % sibling, text).group(1)), s
    for new, sibling in METHODS.items():
        assert inspect.signature(getattr(SourceWiseContext, new)) == inspect.signature(getattr(SourceWiseContext, sibling)), new
    plan = open(os.path.join(build.CSRC, 'bi_k_sourcewise_plan.h')).read()
    assert 'bool EV' in plan and 'launch_sourcewise_plan_events' in open(os.path.join(build.CSRC, 'tu_sourcewise_plan.hip')).read()


def test_a_null_context_is_an_error_code():
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    one, i32, p = np.ones(8), np.zeros(8, dtype=np.int32), _capi.ptr
    assert lib.bi_eval_sourcewise_events_planned(None, 1, p(one), None, None, p(one.copy()), None) == _capi.ERR_INVALID
    assert lib.bi_sample_stretch_sourcewise_events(None, 1, 2, 1, p(i32), p(i32), p(one), p(one), p(one), None, p(one), p(one), p(one), 1, 2.0, 0,
                                                   0, None, None, None, p(one.copy()), p(one.copy()), p(np.zeros(8, dtype=np.int64)),
                                                   None) == _capi.ERR_INVALID
    assert lib.bi_grid_reduce_sourcewise_events(None, 1, None, 1, 0, p(i32), p(i32), p(one), p(one), p(one), p(np.ones(1, dtype=np.int32)), p(one),
                                                None, None, 0, -1, p(one.copy()), p(one.copy()), p(np.zeros(8, dtype=np.int64)),
                                                None) == _capi.ERR_INVALID


class RecordingRoutesContext(RecordingContext):
    """... with what BatchObjective.native() asks for (a fit_batched), an eval for the host engines, and the two calls recorded.
    It has NO sample_stretch and NO grid_reduce: whatever reaches for the binned spellings fails."""

    def __init__(self, device=None):
        super().__init__(device)
        self.calls = []

    def fit_batched(self, *args, **kwargs):
        raise AssertionError('no fit is run here')

    def eval(self, z, rate_scale=None, dataset=None):
        P = len(rate_scale)
        self.calls.append(('eval', P))
        return np.zeros(P), np.zeros(P, dtype=np.int32)

    def sample_stretch_events(self, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a=2.0, seed=0, first_ensemble=0, priors=None):
        self.calls.append(('sample_stretch_events', dict(W=W, kind=kind, index=index, z0=z0, scale0=scale0, unit=unit, dataset=dataset,
                                                         x0=np.array(x0), lo=lo, hi=hi, n_steps=n_steps, a=a, seed=seed,
                                                         first_ensemble=first_ensemble, priors=priors)))
        E, _, F = x0.shape
        return np.zeros((n_steps, E, W, F)), np.zeros((n_steps, E, W)), np.zeros((E, W), dtype=np.int64), np.zeros(5, dtype=np.int64)

    def grid_reduce_events(self, kind, index, z0, scale0, unit, dataset, n_keep, nodes, term=None, logw=None, chunk=0, route=-1):
        self.calls.append(('grid_reduce_events', dict(kind=kind, index=index, z0=z0, scale0=scale0, unit=unit, dataset=dataset, n_keep=n_keep,
                                                      nodes=nodes, term=term, logw=logw, chunk=chunk, route=route)))
        E = 1 if dataset is None else len(dataset)
        K = int(np.prod([len(v) for v in nodes[:n_keep]], dtype=np.int64))
        return np.zeros((E, K)), np.zeros((E, K)), np.zeros((E, K), dtype=np.int64), np.zeros(5, dtype=np.int64)


@pytest.fixture
def recorded(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd import SourceWiseUnbinnedLogLikelihood
    from blueice_amd.priors import GaussianPrior
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingRoutesContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5), source_class=NuisanceHistogramSource)
    lf = SourceWiseUnbinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.25) if s == 2 else None)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.) if n == names[1] else None)
    lf.prepare()
    np.random.seed(11)
    lf.set_datasets([lf.base_model.simulate() for _ in range(3)])
    return lf, names


def test_sample_posterior_and_bestfit_emcee_reach_the_event_sampler(recorded):
    from blueice_amd import inference, sampler
    from blueice_amd.profile import BatchObjective
    lf, names = recorded
    assert not hasattr(lf.ctx, 'sample_stretch') and not hasattr(lf.ctx, 'grid_reduce')
    fixed = {names[7]: 0.5, 's3_rate_multiplier': 1.5}
    p0 = np.random.default_rng(0).uniform(0.9, 1.1, (8, 10)) * np.array([1.0] * 3 + [0.1] * 7)
    res = sampler.sample_posterior(lf, n_walkers=8, n_steps=4, seed=3, p0=p0, datasets=[2, 0], engine='native', first_ensemble=5, **fixed)
    assert res.engine == 'native' and res.chain.shape == (4, 2, 8, 10) and res.log_prob.shape == (4, 2, 8) and len(res.counters) == 5
    assert res.names == ['s0_rate_multiplier', 's1_rate_multiplier', 's2_rate_multiplier'] + names[:7]
    (what, got), = lf.ctx.calls
    assert what == 'sample_stretch_events'
    native = BatchObjective(lf, res.names, {}, fixed, None, np.array([2, 0])).native()
    for key in ('kind', 'index', 'z0', 'scale0', 'unit'):
        np.testing.assert_array_equal(got[key], native[key])
    assert list(got['kind']) == [1, 1, 1] + [0] * 7 and list(got['index']) == [0, 1, 2] + list(range(7))
    mean, sigma, const = got['priors']                          # GaussianPrior constraints go to the device
    np.testing.assert_array_equal(mean, native['prior_mean'])
    np.testing.assert_array_equal(sigma, native['prior_sigma'])
    np.testing.assert_array_equal(const, native['prior_const'])
    assert np.isfinite(sigma).tolist() == [False, False, True, False, True] + [False] * 5 and sigma[2] == 0.25 and mean[2] == 1.0
    assert list(got['dataset']) == [2, 0] and got['W'] == 8 and got['n_steps'] == 4 and got['seed'] == 3 and got['first_ensemble'] == 5 and got['a'] == 2.0
    assert got['x0'].shape == (2, 8, 10) and np.array_equal(got['x0'][0], p0) and np.array_equal(got['x0'][1], p0)
    lf.ctx.calls.clear()

    host = sampler.sample_posterior(lf, n_walkers=8, n_steps=4, seed=3, p0=p0, datasets=[2, 0], engine='host', first_ensemble=5, **fixed)
    assert host.engine == 'host' and host.names == res.names and host.chain.shape == res.chain.shape
    assert all(c[0] == 'eval' for c in lf.ctx.calls) and len(lf.ctx.calls) == 1 + 2 * 4
    lf.ctx.calls.clear()

    best, value = inference.bestfit_emcee(lf, quiet=True, n_walkers=8, n_steps=6, n_burn_in=2, seed=1, p0=p0, engine='native', **fixed)
    assert list(best) == res.names and lf.ctx.calls[0][0] == 'sample_stretch_events' and lf.ctx.calls[0][1]['dataset'] is None
    assert np.isfinite(value)


def test_grid_scan_reaches_the_event_grid(recorded):
    from blueice_amd import grid
    lf, names = recorded
    keep = [('s0_rate_multiplier', np.linspace(0.0, 3.0, 7))]
    reduce = [(names[0], np.linspace(-1.5, 1.5, 6)), ('s2_rate_multiplier', np.linspace(0.6, 1.4, 5))]
    fixed = {names[3]: 0.25}
    res = grid.grid_scan(lf, keep=keep, reduce=reduce, datasets=[1, 0], engine='native', chunk=50, **fixed)
    assert res.engine == 'native' and res.log_marginal.shape == (2, 7)
    (what, got), = lf.ctx.calls
    assert what == 'grid_reduce_events'
    plan = grid._native_plan(lf, grid._axes(keep, 'keep') + grid._axes(reduce, 'reduce'), fixed, None)
    for key in ('kind', 'index', 'z0', 'scale0', 'unit'):
        np.testing.assert_array_equal(got[key], plan[key])
    assert list(got['kind']) == [1, 0, 1] and list(got['index']) == [0, 0, 2] and got['n_keep'] == 1 and got['chunk'] == 50
    assert list(got['dataset']) == [1, 0] and [len(v) for v in got['nodes']] == [7, 6, 5]
    assert got['term'] is not None and not np.any(got['term'][0]) and not np.any(got['term'][1]) and np.any(got['term'][2])    # s2's GaussianPrior
    assert len(got['logw']) == 3 and not np.any(got['logw'][0])
    assert got['route'] == 0                                    # 'auto' on an event store is the per-point route
    lf.ctx.calls.clear()
    for setting, route in (('points', 0), ('scan', 1), ('auto', 0)):
        lf.config['sourcewise_grid_route'] = setting
        grid.grid_scan(lf, keep=keep, reduce=reduce, engine='native')
        assert lf.ctx.calls[-1][1]['route'] == route and lf.ctx.calls[-1][1]['dataset'] is None
    lf.config['sourcewise_grid_route'] = 'rows'
    with pytest.raises(ValueError, match="sourcewise_grid_route"):
        grid.grid_scan(lf, keep=keep, reduce=reduce, engine='native')
    lf.config['sourcewise_grid_route'] = 'auto'
    lf.ctx.calls.clear()
    host = grid.grid_scan(lf, keep=keep, reduce=reduce, datasets=[1, 0], engine='host', **fixed)
    assert host.engine == 'host' and all(c[0] == 'eval' for c in lf.ctx.calls) and sum(c[1] for c in lf.ctx.calls) == 2 * 7 * 6 * 5


def test_the_bound_names_stay_refused_and_name_the_functions(recorded):
    import blueice_amd.source_wise_unbinned as swu
    lf, names = recorded
    for name, spelling in (('sample_posterior', 'blueice_amd.sampler.sample_posterior(lf'),
                           ('bestfit_emcee', 'blueice_amd.inference.bestfit_emcee(lf'), ('grid_scan', 'blueice_amd.grid.grid_scan(lf')):
        with pytest.raises(NotImplementedError, match='unbinned source-wise model') as e:
            getattr(lf, name)()
        assert spelling in str(e.value), (name, str(e.value))
    assert 'not sampling' not in swu._SCOPE
    for word in ('bi_sample_stretch_sourcewise_events', 'bi_grid_reduce_sourcewise_events', 'sourcewise_grid_route'):
        assert word in swu.__doc__, word
    assert not lf.ctx.calls
