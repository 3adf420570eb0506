"""The real-valued layer of source-wise models without a GPU: the header / binding of its six C-ABI symbols, and the Python
layers -- the factories of blueice_amd.asimov and the three Asimov functions of blueice_amd.inference -- over a recording
context that stands where SourceWiseContext would."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('bi_sourcewise_set_real_counts', 'bi_sourcewise_set_asimov_counts', 'bi_sourcewise_real_count_sets',
           'bi_sourcewise_download_real_counts', 'bi_eval_sourcewise_real', 'bi_fit_batched_sourcewise_real')
STIFF = 50.0            # the recording context's half-deviance: STIFF (multiplier of source 0) ** 2


def test_header_and_binding_of_the_six_symbols():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    build.build()
    lib = _capi.load()
    for s in SYMBOLS:
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text)
        assert proto, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.group(1).split(',') if a.strip()]), s
    for ours, theirs in (('bi_sourcewise_set_real_counts', 'bi_set_real_counts'), ('bi_sourcewise_set_asimov_counts', 'bi_set_asimov_counts'),
                         ('bi_sourcewise_real_count_sets', 'bi_real_count_sets'), ('bi_sourcewise_download_real_counts', 'bi_download_real_counts'),
                         ('bi_eval_sourcewise_real', 'bi_eval_real'), ('bi_fit_batched_sourcewise_real', 'bi_fit_batched_real')):
        assert _capi.SIGNATURES[ours] == _capi.SIGNATURES[theirs], ours
    assert 'tu_sourcewise_real' in build.UNITS
    one = np.ones(64)
    p = _capi.ptr
    assert lib.bi_sourcewise_set_real_counts(None, 1, p(one)) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_set_asimov_counts(None, 1, p(one), None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_real_count_sets(None) == 0
    assert lib.bi_sourcewise_download_real_counts(None, 0, p(one.copy())) == _capi.ERR_INVALID
    assert lib.bi_eval_sourcewise_real(None, 1, p(one), None, None, p(one.copy()), None, None) == _capi.ERR_INVALID


# ---- the Python layers over a recording context -----------------------------------------------------------------------

class RecordingRealContext:
    """Stands where SourceWiseContext would: records what the Asimov layers ask of it.  Its half-deviance is
    STIFF * (multiplier of source 0) ** 2 whatever the data, and its fit returns the start with that value."""
    device = 0

    def __init__(self, device=None):
        self.calls = []
        self.T = 0
        self.sets = 0

    def begin_model(self, anchor_z, S, B, own_axes):
        self.d, self.S, self.B = len(anchor_z), S, B

    def set_anchor(self, s, local_index, ps_row, mu):
        pass

    def end_model(self):
        pass

    def set_counts(self, counts):
        self.T = np.asarray(counts).size // self.B
        self.calls.append(('set_counts', self.T))

    def get_param(self, name):
        return 0

    def set_param(self, name, value):
        pass

    def interpolate(self, which, z):
        return np.ones(self.S)

    def set_asimov_counts(self, z, rate_scale=None):
        z, rate_scale = np.array(z).reshape(-1, self.d), np.atleast_2d(np.array(rate_scale))
        self.calls.append(('set_asimov_counts', z, rate_scale))
        self.sets = len(z)
        return len(z)

    def set_real_counts(self, counts):
        c = np.asarray(counts, dtype=float)
        self.calls.append(('set_real_counts', c.shape))
        self.sets = c.size // self.B

    @property
    def real_count_sets(self):
        return self.sets

    def download_real_counts(self, t=0):
        return np.full(self.B, 1.5 + t)

    def eval_real(self, z, rate_scale=None, dataset=None, gradient=True):
        z, rs = np.atleast_2d(z), np.atleast_2d(rate_scale)
        P = len(rs)
        self.calls.append(('eval_real', z.shape, rs.shape, None if dataset is None else np.array(dataset), bool(gradient)))
        half = STIFF * rs[:, 0] ** 2
        st = np.zeros(P, dtype=np.int32)
        if not gradient:
            return half, None, None, st
        gs = np.zeros((P, self.S))
        gs[:, 0] = 2 * STIFF * rs[:, 0]
        return half, np.zeros((P, self.d)), gs, st

    def fit_batched_real(self, P, F, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks, gtol, max_iter, x, f, flags, counters,
                         priors=None):
        self.calls.append(('fit_batched_real', int(P), int(F), np.array(kind), np.array(index), np.shape(z0), np.shape(scale0),
                           None if dataset is None else np.array(dataset)))
        m0 = np.array(scale0[:, 0] / unit[:, 0])
        for j in range(F):
            if kind[j] == 1 and index[j] == 0:
                m0 = np.array(x0[:, j])
        x[:] = x0
        f[:] = STIFF * m0 ** 2
        flags[:] = 1
        counters[:] = [1, 1, 0, P]
        return 0


@pytest.fixture
def recorded(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingRealContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    lf.prepare()
    return lf, names


def test_the_factories_reach_the_context(recorded):
    from blueice_amd import asimov
    from blueice_amd.asimov import AsimovLikelihood
    from blueice_amd.exceptions import NotPreparedException
    lf, names = recorded
    calls = lf.ctx.calls
    d = len(names)

    view = asimov.asimov(lf, **{names[0]: 0.5, 's1_rate_multiplier': 1.5})
    kind, z, scale = calls.pop()
    assert kind == 'set_asimov_counts' and z.shape == (1, d) and scale.shape == (1, 4) and z[0, 0] == 0.5
    assert scale[0, 1] == 1.5 * scale[0, 2] and not calls
    assert isinstance(view, AsimovLikelihood) and view.n_sets == 1 and not view.supports_hessian and view.supports_gradient
    assert not lf.is_data_set and view.is_data_set and view.ctx.T == 1 and view.counts(0).shape == (6, 5)

    value = view(s0_rate_multiplier=0.5)
    kind, zs, rss, ds, grad = calls.pop()
    assert kind == 'eval_real' and rss == (1, 4) and not grad and ds == 0
    assert abs(value + STIFF * (0.5 * scale[0, 2]) ** 2) <= 1e-12
    ll = view.eval_points({'s0_rate_multiplier': np.array([0.0, 1.0, 2.0])}, dataset=np.zeros(3, dtype=np.int64))
    kind, zs, rss, ds, grad = calls.pop()
    assert (kind, zs, rss, grad) == ('eval_real', (3, d), (3, 4), False) and list(ds) == [0, 0, 0] and ll[0] == 0.0 and ll[2] < ll[1] < 0
    ll, grads = view.values_and_gradients({'s0_rate_multiplier': np.array([0.5, 1.0])})
    kind, zs, rss, ds, grad = calls.pop()
    assert (kind, zs, rss, grad) == ('eval_real', (2, d), (2, 4), True) and np.all(grads['s0_rate_multiplier'] < 0) and len(grads) == 4 + d
    one, g1 = view.value_and_gradient(s0_rate_multiplier=0.5)
    assert calls.pop()[0] == 'eval_real' and one == ll[0] and g1['s0_rate_multiplier'] == grads['s0_rate_multiplier'][0]

    best, top = view.bestfit_batched(**{n: 0.0 for n in names})
    kind, P, F, var_kind, var_index, zshape, sshape, ds = calls.pop()
    assert (kind, F, zshape[1], sshape[1]) == ('fit_batched_real', 4, d, 4) and list(var_kind) == [1, 1, 1, 1] and list(var_index) == [0, 1, 2, 3]

    many = asimov.asimov_points(lf, {names[1]: np.array([-0.5, 0.0, 0.5])})
    kind, z, scale = calls.pop()
    assert kind == 'set_asimov_counts' and z.shape == (3, d) and scale.shape == (3, 4) and list(z[:, 1]) == [-0.5, 0.0, 0.5]
    assert many.n_sets == 3 and many.ctx.T == 3
    with pytest.raises(NotPreparedException, match='stale'):
        view(s0_rate_multiplier=0.5)
    many.bestfit_batched(datasets=np.arange(3))
    fit = calls.pop()
    # (the engine may stack several starts per problem: the datasets then repeat with period 3)
    assert fit[0] == 'fit_batched_real' and fit[1] % 3 == 0 and fit[2] == 4 + d and list(fit[7]) == [0, 1, 2] * (fit[1] // 3)

    del calls[:]                                                # (the fit's evaluations of its starts)
    weighted = asimov.real_data(lf, np.full((2, 6, 5), 0.25))
    assert calls.pop() == ('set_real_counts', (2, 6, 5)) and weighted.n_sets == 2
    with pytest.raises(ValueError, match='real_data'):
        asimov.real_data(lf, np.ones((5, 6)))
    with pytest.raises(NotPreparedException, match='stale'):
        many.eval_points({names[1]: np.array([0.0])})
    assert not lf.is_data_set and not any(c[0] == 'set_counts' for c in calls)
    # the bound asimov_points is the module function
    bound = lf.asimov_points({names[1]: np.array([0.25])})
    assert calls.pop()[0] == 'set_asimov_counts' and isinstance(bound, AsimovLikelihood)


def test_the_asimov_functions_of_inference_reach_the_context(recorded):
    from blueice_amd import inference
    lf, names = recorded
    calls = lf.ctx.calls
    d = len(names)
    fixed = {n: 0.0 for n in names}
    unit = None

    hyps = np.array([0.5, 1.0, 2.0])
    q = inference.asimov_test_statistic(lf, 's0_rate_multiplier', hyps, **fixed)
    made = [c for c in calls if c[0] == 'set_asimov_counts']
    fits = [c for c in calls if c[0] == 'fit_batched_real']
    assert len(made) == 1 and made[0][2].shape == (1, 4) and made[0][2][0, 0] == 0.0          # the background-only truth
    unit = made[0][2][0, 1]
    # the free fit over the four multipliers, then the three hypotheses with s0 fixed (several starts per problem may be stacked)
    assert fits[0][2] == 4 and fits[-1][2] == 3 and fits[-1][1] % 3 == 0 and {c[2] for c in fits} == {3, 4}
    np.testing.assert_allclose(q, 2 * STIFF * (hyps * unit) ** 2, rtol=1e-12)
    assert np.array_equal(lf.asimov_test_statistic('s0_rate_multiplier', hyps, **fixed), q)

    del calls[:]
    zs = inference.expected_discovery_significance(lf, 's0_rate_multiplier', dict(s0_rate_multiplier=1.0), **fixed)
    made = [c for c in calls if c[0] == 'set_asimov_counts']
    assert len(made) == 1 and made[0][2][0, 0] == unit and any(c[0] == 'fit_batched_real' for c in calls)
    # (the recording context's deviance does not depend on its data: the free fit starts at the truth and stays there)
    assert zs == 0.0 and lf.expected_discovery_significance('s0_rate_multiplier', dict(s0_rate_multiplier=1.0), **fixed) == 0.0

    del calls[:]
    limits = inference.expected_upper_limit(lf, 's0_rate_multiplier', 5.0, n_sigma=(-2, 0, 1), **fixed)
    assert [c[0] for c in calls].count('set_asimov_counts') == 1 and any(c[0] == 'fit_batched_real' for c in calls)
    # (the search itself is held to the closed form on the device, test_sourcewise_real_gpu.py: the recording fit does not minimise)
    assert limits[-2] == 0.0 and all(0.0 < limits[n] <= 5.0 for n in (0, 1))
    assert {c[2] for c in calls if c[0] == 'fit_batched_real'} == {3, 4}          # the free fit, and the target held at hypotheses
    assert not lf.is_data_set and not any(c[0] == 'set_counts' for c in calls)


def test_pinned_bound_names_refuse_with_their_spellings(recorded):
    from blueice_amd import coarse, inference
    lf, names = recorded
    n_before = len(lf.ctx.calls)
    for name, spelling in (('asimov', 'blueice_amd.asimov.asimov(lf, **truth)'), ('real_data', 'blueice_amd.asimov.real_data(lf, counts)'),
                           ('expected_upper_limit', 'blueice_amd.inference.expected_upper_limit(lf, target, bound)')):
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            getattr(lf, name)()
        assert spelling in str(e.value), (name, str(e.value))
        assert name in type(lf)._REFUSED
    for name in ('asimov_points', 'asimov_test_statistic', 'expected_discovery_significance'):
        assert name not in type(lf)._REFUSED and callable(getattr(lf, name))
    for gate in (coarse._binned_for_gof, inference._binned_for_gof):
        with pytest.raises(NotImplementedError, match='BinnedLogLikelihood'):
            gate(lf, 'asimov')
    for name in ('grid_scan', 'expected_coarse', 'sample_posterior', 'eval_toys', 'eval_toys_points'):          # out of scope: as before
        with pytest.raises(NotImplementedError, match='source-wise'):
            getattr(lf, name)()
    assert len(lf.ctx.calls) == n_before


def test_the_factories_keep_refusing_what_has_no_real_valued_path(monkeypatch):
    import blueice_amd.source_wise as sw
    from blueice_amd import asimov, BinnedLogLikelihood, LogLikelihoodSum, UnbinnedLogLikelihood
    from blueice_amd.exceptions import NotPreparedException
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingRealContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    like = dict(device_histograms=False)
    # an unprepared source-wise model
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=like)
    lf.add_shape_parameter(names[0], (-1., 0., 1.))
    for call in (lambda: asimov.asimov(lf), lambda: asimov.asimov_points(lf, {names[0]: [0.0]}), lambda: asimov.real_data(lf, np.ones((6, 5)))):
        with pytest.raises(NotPreparedException, match='prepare'):
            call()
    # Beeston-Barlow: the class itself, and the grid model behind the factories
    with pytest.raises(NotImplementedError, match='Beeston-Barlow'):
        sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(like, model_statistical_uncertainty_handling='bb_single'))
    bb = BinnedLogLikelihood.__new__(BinnedLogLikelihood)
    bb.model_statistical_uncertainty_handling = 'bb_single'
    unbinned = UnbinnedLogLikelihood.__new__(UnbinnedLogLikelihood)
    total = LogLikelihoodSum.__new__(LogLikelihoodSum)
    for other, why in ((bb, 'Beeston-Barlow'), (unbinned, 'BinnedLogLikelihood'), (total, 'BinnedLogLikelihood')):
        for call in (lambda: asimov.asimov(other), lambda: asimov.asimov_points(other, {}), lambda: asimov.real_data(other, np.ones(3))):
            with pytest.raises(NotImplementedError, match=why):
                call()
