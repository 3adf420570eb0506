"""The ensemble sampler of source-wise models without a GPU: the library cross-compiles with the planner's translation unit, the
header, the ctypes binding and the bound methods agree, blueice_amd.sampler.sample_posterior reaches the context's sample_stretch
with what BatchObjective.native() gives (over test_factored_curvature_host's recording context), and the bound names stay refused
and name the spellings that work."""
import inspect
import os
import re

import numpy as np
import pytest

from test_factored_curvature_host import RecordingCurvatureContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('bi_eval_sourcewise_planned', 'bi_sample_stretch_sourcewise')


def test_header_binding_and_methods_agree():
    from blueice_amd import _capi, build
    from blueice_amd.device import DeviceContext
    from blueice_amd.source_wise import SourceWiseContext
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert 'tu_sourcewise_plan' in build.UNITS and os.path.exists(os.path.join(build.CSRC, 'tu_sourcewise_plan.hip'))
    build.build()                                             # cross-compiles for gfx950 with the new unit
    lib = _capi.load()
    for s in NEW:
        assert 'factored' not in s
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text)
        assert proto, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.group(1).split(',') if a.strip()]), s
    assert _capi.SIGNATURES['bi_sample_stretch_sourcewise'] == _capi.SIGNATURES['bi_sample_stretch_gauss']
    assert _capi.SIGNATURES['bi_eval_sourcewise_planned'][1] == _capi.SIGNATURES['bi_eval_factored'][1][:6] + _capi.SIGNATURES['bi_eval_factored'][1][7:]
    one, i32 = np.ones(8), np.zeros(8, dtype=np.int32)
    p = _capi.ptr
    assert lib.bi_eval_sourcewise_planned(None, 1, p(one), None, None, p(one.copy()), None) == _capi.ERR_INVALID
    assert lib.bi_sample_stretch_sourcewise(None, 1, 2, 1, p(i32), p(i32), p(one), p(one), p(one), None, p(one), p(one), p(one), 1, 2.0, 0, 0,
                                            None, None, None, p(one.copy()), p(one.copy()), p(np.zeros(8, dtype=np.int64)), None) == _capi.ERR_INVALID
    assert inspect.signature(SourceWiseContext.sample_stretch) == inspect.signature(DeviceContext.sample_stretch)
    assert list(inspect.signature(SourceWiseContext.eval_planned).parameters) == list(inspect.signature(SourceWiseContext.eval).parameters)
    header = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    assert 'counters [5]' in header and '[4] stream' in header


class RecordingSamplerContext(RecordingCurvatureContext):
    """... with what BatchObjective.native() asks for (a fit_batched), an eval for the host engine, and the sampler's call recorded"""

    def fit_batched(self, *args, **kwargs):
        raise AssertionError('no fit is run here')

    def eval(self, z, rate_scale=None, dataset=None):
        P = len(rate_scale)
        self.calls.append(('eval', P))
        return np.zeros(P), np.zeros(P, dtype=np.int32)

    def sample_stretch(self, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a=2.0, seed=0, first_ensemble=0, priors=None):
        self.calls.append(('sample_stretch', dict(W=W, kind=kind, index=index, z0=z0, scale0=scale0, unit=unit, dataset=dataset, x0=np.array(x0), lo=lo,
                                                  hi=hi, n_steps=n_steps, a=a, seed=seed, first_ensemble=first_ensemble, priors=priors)))
        E, _, F = x0.shape
        return np.zeros((n_steps, E, W, F)), np.zeros((n_steps, E, W)), np.zeros((E, W), dtype=np.int64), np.zeros(5, dtype=np.int64)


@pytest.fixture
def recorded(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd.priors import GaussianPrior
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingSamplerContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.25) if s == 2 else None)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.) if n == names[1] else None)
    lf.prepare()
    lf.set_binned_data(np.ones((3, 6, 5)))
    return lf, names


def test_sample_posterior_reaches_the_context(recorded):
    from blueice_amd import inference, sampler
    from blueice_amd.profile import BatchObjective
    lf, names = recorded
    fixed = {names[7]: 0.5, 's3_rate_multiplier': 1.5}
    p0 = np.random.default_rng(0).uniform(0.9, 1.1, (8, 10)) * np.array([1.0] * 3 + [0.1] * 7)
    res = sampler.sample_posterior(lf, n_walkers=8, n_steps=4, seed=3, p0=p0, datasets=[2, 0], engine='native', first_ensemble=5, **fixed)
    assert res.engine == 'native' and res.chain.shape == (4, 2, 8, 10) and res.log_prob.shape == (4, 2, 8) and len(res.counters) == 5
    assert res.names == ['s0_rate_multiplier', 's1_rate_multiplier', 's2_rate_multiplier'] + names[:7]
    (what, got), = lf.ctx.calls
    assert what == 'sample_stretch'
    native = BatchObjective(lf, res.names, {}, fixed, None, np.array([2, 0])).native()
    for key in ('kind', 'index', 'z0', 'scale0', 'unit'):
        np.testing.assert_array_equal(got[key], native[key])
    assert list(got['kind']) == [1, 1, 1] + [0] * 7 and list(got['index']) == [0, 1, 2] + list(range(7))
    assert got['z0'].shape == (2, 8) and np.all(got['z0'][:, 7] == 0.5) and np.all(got['scale0'][:, 3] == 1.5 * got['unit'][:, 3])
    mean, sigma, const = got['priors']
    np.testing.assert_array_equal(mean, native['prior_mean'])
    np.testing.assert_array_equal(sigma, native['prior_sigma'])
    np.testing.assert_array_equal(const, native['prior_const'])
    assert np.isfinite(sigma).tolist() == [False, False, True, False, True] + [False] * 5 and sigma[2] == 0.25 and mean[2] == 1.0
    assert list(got['dataset']) == [2, 0] and got['W'] == 8 and got['n_steps'] == 4 and got['seed'] == 3 and got['first_ensemble'] == 5 and got['a'] == 2.0
    assert got['x0'].shape == (2, 8, 10) and np.array_equal(got['x0'][0], p0) and np.array_equal(got['x0'][1], p0)
    lf.ctx.calls.clear()

    host = sampler.sample_posterior(lf, n_walkers=8, n_steps=4, seed=3, p0=p0, datasets=[2, 0], engine='host', first_ensemble=5, **fixed)
    assert host.engine == 'host' and host.names == res.names
    assert host.chain.shape == res.chain.shape and host.log_prob.shape == res.log_prob.shape and host.n_accepted.shape == res.n_accepted.shape
    assert all(c[0] == 'eval' for c in lf.ctx.calls) and len(lf.ctx.calls) == 1 + 2 * 4
    lf.ctx.calls.clear()

    # the reference's spelling, as a function: one dataset, the medians and the likelihood there
    lf.set_binned_data(np.ones((6, 5)))
    best, value = inference.bestfit_emcee(lf, quiet=True, n_walkers=8, n_steps=6, n_burn_in=2, seed=1, p0=p0, engine='native', **fixed)
    assert list(best) == res.names and lf.ctx.calls[0][0] == 'sample_stretch' and lf.ctx.calls[0][1]['dataset'] is None
    assert np.isfinite(value)


def test_the_bound_names_stay_refused_and_name_the_functions(recorded):
    import blueice_amd.source_wise as sw
    lf, names = recorded
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.sample_posterior()
    assert 'blueice_amd.sampler.sample_posterior(lf' in str(e.value)
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.bestfit_emcee(quiet=True)
    assert 'blueice_amd.inference.bestfit_emcee(lf' in str(e.value)
    with pytest.raises(NotImplementedError, match='source-wise') as e:
        lf.grid_scan()
    assert 'the ensemble sampler' in str(e.value)                 # the generic sentence lists what exists
    assert 'bi_sample_stretch_sourcewise' in sw.__doc__ and 'and the ensemble sampler.' not in sw.__doc__
    assert not lf.ctx.calls
