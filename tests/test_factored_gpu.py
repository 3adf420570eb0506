"""Source-wise (factored) models on the device: bi_eval_factored and bi_fit_batched_factored against the exact oracle.

Every comparison of a finite number is derivative_oracle.check_entries with C_POISSON = 256: |device - oracle| <= C 2^-52 cond,
the oracle being `derivatives(expand(model))` -- the same likelihood on the full tensor-product grid, the parent commit's
specification -- wherever that grid can be held, and `factored_oracle.factored_derivatives` with its own (smaller) cond where
it cannot.  Status words, -inf and nan are exact; "bitwise" means the same bits."""
import numpy as np
import pytest

import factored_oracle as fo
from derivative_oracle import C_POISSON, check_entries, derivatives

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
N_ANCHOR, OWN = (3, 2, 4), ((0,), (1, 2), ())


def upload(model, counts):
    from blueice_amd.source_wise import SourceWiseContext
    ctx = SourceWiseContext(0)
    B = fo.n_bins(model)
    ctx.begin_model(model['anchor_z'], len(model['own']), B, model['own'])
    for s, own in enumerate(model['own']):
        rows = np.asarray(model['ps'][s]).reshape(-1, B)
        mus = np.asarray(model['mus'][s]).reshape(-1)
        for k in np.random.default_rng(s).permutation(len(rows)):        # any order
            ctx.set_anchor(s, int(k), rows[k], mus[k])
    ctx.end_model()
    ctx.set_counts(counts)
    return ctx


def box_points(model, rng, n, on_anchor=True):
    """n points: inside cells, one exactly on interior anchors (where there are any), one on the upper edge of the box"""
    g = model['anchor_z']
    d, S = len(g), len(model['own'])
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    z = lo + (hi - lo) * rng.uniform(0.03, 0.97, (n, d))
    if on_anchor and n > 2:
        for i, a in enumerate(g):
            if len(a) > 2 and i % 2 == 0:
                z[n - 2, i] = a[1 + i % (len(a) - 2)]
        z[n - 1] = hi
    return z, rng.uniform(0.5, 1.6, (n, S))


def check_points(ctx, model, z, rs, counts, oracle, what, dataset=None):
    """value and gradient of every point against oracle(z, rs, counts) -> the worst ratio"""
    ll, gz, gs, st = ctx.eval_grad(z, rs, dataset)
    ll0, st0 = ctx.eval(z, rs, dataset)
    assert not st.any() and not st0.any()
    np.testing.assert_array_equal(ll0, ll)                      # grad == NULL: the same bits
    worst = 0.0
    for p in range(len(z)):
        n = counts if dataset is None else counts[dataset[p]]
        want = oracle(z[p], rs[p], n)
        worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (what, p)))
        worst = max(worst, check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='%s grad[%d]' % (what, p)))
    print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (what, worst, C_POISSON))
    return worst


def expanded_oracle(model):
    full = fo.expand(model)
    return lambda z, rs, n: derivatives(full, z, rs, n, hessian=False)


@pytest.fixture(scope='module')
def small():
    """the d = 3 models of the host test at B = 63 and 1001 (a quarter of source 1's bins zero), three datasets each"""
    out = {}
    for B in (63, 1001):
        rng = np.random.default_rng(500 + B)
        model = fo.random_model(rng, N_ANCHOR, OWN, B, zero_quarter=(1,))
        z, rs = box_points(model, rng, 3, on_anchor=False)
        counts = np.stack([rng.poisson(fo.expectation(model, z[t], rs[t])).astype(float) for t in range(3)])
        out[B] = (model, counts)
    return out


@pytest.mark.parametrize('B', [63, 1001])
def test_small_shapes_against_the_oracle_of_the_expansion(small, B):
    """B = 63: less than one tile; B = 1001: two tiles with a ragged tail"""
    model, counts = small[B]
    ctx = upload(model, counts[0])
    z, rs = box_points(model, np.random.default_rng(B), 6)
    check_points(ctx, model, z, rs, counts[0], expanded_oracle(model), 'd=3 B=%d' % B)
    # a point's bits do not depend on the batch it is evaluated in (two tiles: two blocks per item)
    ll, gz, gs, _ = ctx.eval_grad(z, rs)
    for p in range(len(z)):
        a = ctx.eval_grad(z[p], rs[p:p + 1])
        np.testing.assert_array_equal(a[0][0], ll[p])
        np.testing.assert_array_equal(a[1][0], gz[p])
        np.testing.assert_array_equal(a[2][0], gs[p])
    # no rate scales: ones
    np.testing.assert_array_equal(ctx.eval(z, None)[0], ctx.eval(z, np.ones_like(rs))[0])
    ctx.close()


@pytest.mark.parametrize('case', ['e3x8', 'mixed', 'mixed_padded', 's2_e1', 's2_e2', 's2_e3', 's4_e1', 's8_e1', 's8_e2'])
def test_largest_kernel_class_and_mixed_ownership(case):
    """S = 8, every source owning 3 of d = 4 axes (the kernel's largest class: 64 rows per point); e = (0, 1, 2, 3): every
    template value of e_s in one launch; and the same with a fifth source, so that padded empty source slots run.  The other
    cases launch the remaining (source slots, own axes) classes of the kernel: two sources with e <= 1, 2, 3, three with e <= 1,
    eight with e <= 1 and e <= 2 (the latter on the one-bin-in-flight path)"""
    triples = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    own = {'e3x8': [triples[s % 4] for s in range(8)], 'mixed': [(), (2,), (0, 3), (0, 1, 2)],
           'mixed_padded': [(), (2,), (0, 3), (0, 1, 2), (1, 3)],
           's2_e1': [(1,), ()], 's2_e2': [(0, 3), (2,)], 's2_e3': [(0, 1, 2), (3,)], 's4_e1': [(0,), (3,), ()],
           's8_e1': [(s % 4,) if s != 5 else () for s in range(8)],
           's8_e2': [[(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2,), ()][s] for s in range(8)]}[case]
    rng = np.random.default_rng(len(own) + sum(len(o) for o in own))
    model = fo.random_model(rng, (2, 2, 2, 2), own, 1027, zero_quarter=(1,))
    z, rs = box_points(model, rng, 4)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    ctx = upload(model, counts)
    check_points(ctx, model, z, rs, counts, expanded_oracle(model), case)
    ctx.close()


def test_many_axes():
    """d = 24, S = 8, three own axes each, 3 anchors per axis, B = 515: the grid model cannot hold this (3^24 anchors); the
    oracle is the factored specification with its own cond"""
    rng = np.random.default_rng(24)
    own = [(3 * s, 3 * s + 1, 3 * s + 2) for s in range(8)]
    model = fo.random_model(rng, (3,) * 24, own, 515)
    z, rs = box_points(model, rng, 4)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    ctx = upload(model, counts)
    check_points(ctx, model, z, rs, counts, lambda zp, rp, n: fo.factored_derivatives(model, zp, rp, n), 'd=24')
    ctx.close()


def test_status_and_edge_values():
    rng = np.random.default_rng(7)
    own = ((0,), (1,), ())                                  # nobody owns axis 2
    model = fo.random_model(rng, N_ANCHOR, own, 63)
    for s in range(3):
        model['ps'][s][..., 5] = 0.0                        # bin 5: every template is 0 at every anchor
    z, rs = box_points(model, rng, 8, on_anchor=False)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    hit = counts.copy()
    hit[5] = 2.0
    assert counts[5] == 0.0
    ctx = upload(model, np.stack([counts, hit]))
    g = model['anchor_z']
    z[1, 2] = g[2][-1] + 0.25                               # outside the box on the axis nobody owns
    z[2, 0] = np.nan
    rs[3, 1] = -0.5
    ds = np.zeros(8, dtype=np.int64)
    ds[4] = 2                                               # == T
    rs[5, 0] = 0.0                                          # a zero rate scale: finite, and the slope of that source is right
    ds[6] = 1                                               # n > 0 where mu = 0
    ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
    np.testing.assert_array_equal(st, [0, ST_OUT_OF_BOUNDS, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET, 0, 0, 0])
    for p in (1, 2, 3, 4, 6):
        assert ll[p] == -np.inf and np.isnan(gz[p]).all() and np.isnan(gs[p]).all(), p
    np.testing.assert_array_equal(ctx.eval(z, rs, ds)[0], ll)
    np.testing.assert_array_equal(ctx.eval(z, rs, ds)[1], st)
    oracle = expanded_oracle(model)
    for p in (0, 5, 7):                                     # bin 5 has n = 0, mu = 0 there: it contributes 0
        want = oracle(z[p], rs[p], counts)
        assert np.isfinite(ll[p])
        check_entries(ll[p], want['ll'], want['ll_cond'], what='ll[%d]' % p)
        check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='grad[%d]' % p)
    assert gs[5, 0] != 0.0 and gz[5, 0] == 0.0              # d ll / d rs_0 = M_0 sum f tau_0; the shape slope carries rs_0 = 0
    assert (gz[[0, 5, 7], 2] == 0.0).all()                  # an axis nobody owns has slope 0
    # the C ABI's refusals
    dev = ctx._dev
    with pytest.raises(Exception, match='was set before|bi_factored_begin first'):
        ctx.set_anchor(0, 0, model['ps'][0][0], 1.0)
    from blueice_amd.exceptions import NotPreparedException
    with pytest.raises(NotPreparedException, match='no model uploaded'):     # every existing entry point: its usual BI_ERR_STATE
        dev.d, dev.S = 3, 3
        dev.eval(z[:1], rs[:1])
    ctx.close()
    from blueice_amd.source_wise import SourceWiseContext
    c2 = SourceWiseContext(0)
    with pytest.raises(ValueError, match='outside \\[0,3\\]'):
        c2.begin_model(model['anchor_z'] + [np.array([0., 1.])], 1, 8, [(0, 1, 2, 3)])
    c2.begin_model(model['anchor_z'], 3, 63, own)
    c2.set_anchor(2, 0, model['ps'][2], 3.0)
    with pytest.raises(ValueError, match='was set before'):
        c2.set_anchor(2, 0, model['ps'][2], 3.0)
    with pytest.raises(ValueError, match='finite and >= 0'):
        c2.set_anchor(0, 0, -model['ps'][0][0] - 1.0, 3.0)
    with pytest.raises(NotPreparedException, match='never set'):
        c2.end_model()
    with pytest.raises(NotPreparedException, match='no source-wise model'):
        c2.eval(z[:1], rs[:1])
    c2.close()


def test_datasets_mixed_in_one_call(small):
    model, counts = small[1001]
    ctx = upload(model, counts)
    z, rs = box_points(model, np.random.default_rng(3), 9)
    ds = np.arange(9, dtype=np.int64) % 3
    ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
    assert not st.any()
    for t in range(3):
        single = upload(model, counts[t])
        a = single.eval_grad(z[ds == t], rs[ds == t])
        np.testing.assert_array_equal(a[0], ll[ds == t])
        np.testing.assert_array_equal(a[1], gz[ds == t])
        np.testing.assert_array_equal(a[2], gs[ds == t])
        single.close()
    check_points(ctx, model, z, rs, counts, expanded_oracle(model), 'T=3', dataset=ds)
    ctx.close()


def test_batches_across_the_chunk_boundary(small):
    """P = 65 536 + 5 at B = 63 crosses run_item_chunks' 65 535-item boundary: every point equals the same point in a batch of
    7 (all of them) and alone (a sample, the boundary's neighbours among it) bit for bit; repeated calls agree; values only
    gives the same ll bits"""
    model, counts = small[63]
    ctx = upload(model, counts[0])
    P = 65536 + 5
    z, rs = box_points(model, np.random.default_rng(65), P, on_anchor=False)
    z[17, 0] = model['anchor_z'][0][0] - 1.0               # a rejected point in the batch: the live points close ranks
    ll, gz, gs, st = ctx.eval_grad(z, rs)
    assert st[17] == ST_OUT_OF_BOUNDS and st.sum() == ST_OUT_OF_BOUNDS and np.isfinite(np.delete(ll, 17)).all()
    again = ctx.eval_grad(z, rs)
    for a, b in zip(again, (ll, gz, gs, st)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ctx.eval(z, rs)[0], ll)
    ll7, gz7, gs7 = np.empty_like(ll), np.empty_like(gz), np.empty_like(gs)
    for i in range(0, P, 7):
        ll7[i:i + 7], gz7[i:i + 7], gs7[i:i + 7], _ = ctx.eval_grad(z[i:i + 7], rs[i:i + 7])
    np.testing.assert_array_equal(ll7, ll)
    np.testing.assert_array_equal(gz7, gz)
    np.testing.assert_array_equal(gs7, gs)
    alone = np.unique(np.concatenate([np.arange(4), np.arange(65530, 65541), np.random.default_rng(1).integers(0, P, 48)]))
    for p in alone:
        a = ctx.eval_grad(z[p], rs[p:p + 1])
        np.testing.assert_array_equal(a[0][0], ll[p])
        np.testing.assert_array_equal(a[1][0], gz[p])
        np.testing.assert_array_equal(a[2][0], gs[p])
    oracle = expanded_oracle(model)
    for p in (0, 65534, 65535, 65536, P - 1):
        want = oracle(z[p], rs[p], counts[0])
        check_entries(ll[p], want['ll'], want['ll_cond'], what='ll[%d]' % p)
        check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='grad[%d]' % p)
    ctx.close()


# ---- the Python class ---------------------------------------------------------------------------------------------------

def tensor_likelihoods(model, counts, priors):
    """The source-wise likelihood of `model` and the plain BinnedLogLikelihood of the same sources on the full grid (the
    parent commit's route), built through the ordinary config -> Model -> prepare() route from one Source class."""
    from blueice_amd import BinnedLogLikelihood, GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.source import Source
    d, S, B = len(model['anchor_z']), len(model['own']), fo.n_bins(model)
    names = ['shape%d' % i for i in range(d)]

    class TensorSource(Source):
        def __init__(self, config, *args, **kwargs):
            m, s = config['tensor_model'], config['source_index']
            idx = tuple(int(np.flatnonzero(np.asarray(m['anchor_z'][i]) == float(config[names[i]]))[0]) for i in m['own'][s])
            self._row = np.asarray(m['ps'][s])[idx]
            super().__init__(dict(config, events_per_day=float(np.asarray(m['mus'][s])[idx]), livetime_days=1), *args, **kwargs)

        def get_pmf_grid(self):
            return self._row.copy(), np.full(self._row.shape, np.inf)

    out = []
    for cls in (SourceWiseBinnedLogLikelihood, BinnedLogLikelihood):
        conf = dict(analysis_space=[('x', np.arange(B + 1, dtype=float))], default_source_class=TensorSource, tensor_model=model,
                    sources=[dict(name='s%d' % s, source_index=s,
                                  extra_dont_hash_settings=[n for i, n in enumerate(names) if i not in model['own'][s]]) for s in range(S)],
                    **{n: float(g[len(g) // 2]) for n, g in zip(names, model['anchor_z'])})
        lf = cls(conf, likelihood_config=dict(device=0, device_histograms=False))
        for s in range(2):
            lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.2) if priors else None)
        for i, (n, g) in enumerate(zip(names, model['anchor_z'])):
            lf.add_shape_parameter(n, tuple(float(v) for v in g),
                                   log_prior=GaussianPrior(float(g[len(g) // 2]), 0.5) if priors and i == 0 else None)
        lf.prepare()
        lf.set_binned_data(counts)
        out.append(lf)
    return out


@pytest.mark.parametrize('priors', [False, True])
def test_native_fit_against_the_grid_model(small, priors):
    """64 problems (one dataset each) floating two shape parameters and two rate multipliers, with and without Gaussian
    constraints: bi_fit_batched_factored on the source-wise likelihood against bi_fit_batched[_gauss] on the plain likelihood
    of the expanded model.  Where both converge the maxima agree to 1e-6 in ll (README's tolerance of the profile engine), and
    neither is below the other's point re-evaluated by the oracle by more than that."""
    model, _ = small[1001]
    rng = np.random.default_rng(64)
    z, rs = box_points(model, rng, 64, on_anchor=False)
    z[:, 2] = 0.5 * (model['anchor_z'][2][1] + model['anchor_z'][2][2])
    rs[:, 2] = 1.0
    counts = np.stack([rng.poisson(fo.expectation(model, z[t], rs[t])).astype(float) for t in range(64)])
    sw, plain = tensor_likelihoods(model, counts, priors)
    assert type(sw.ctx).__name__ == 'SourceWiseContext' and plain.ctx.d == 3
    fixed = dict(shape2=float(z[0, 2]))
    results = []
    for lf in (sw, plain):
        best, ll, info = lf.bestfit_batched(datasets=np.arange(64), return_info=True, **fixed)
        assert list(best) == ['s0_rate_multiplier', 's1_rate_multiplier', 'shape0', 'shape1']
        results.append((best, ll, info))
        print('%s: %d of 64 converged, %d evaluations in %d calls' % (type(lf).__name__, int(info['converged'].sum()), info['evaluations'],
                                                                      info['calls']))
    assert results[0][2]['evaluations'] > 0                        # the native loop ran (counters[3])

    def oracle_ll(best, p):
        zp = np.array([best['shape0'][p], best['shape1'][p], fixed['shape2']])
        rp = np.array([best['s0_rate_multiplier'][p], best['s1_rate_multiplier'][p], 1.0])
        ll = fo.factored_derivatives(model, zp, rp, counts[p])['ll']
        if priors:
            ll += sum(sw.rate_parameters['s%d' % s](rp[s]) for s in range(2)) + sw.shape_parameters['shape0'][1](zp[0])
        return ll

    (b_sw, ll_sw, i_sw), (b_pl, ll_pl, i_pl) = results
    both = i_sw['converged'] & i_pl['converged']
    assert both.any()
    worst = 0.0
    for p in range(64):
        at_sw, at_pl = oracle_ll(b_sw, p), oracle_ll(b_pl, p)
        if np.isfinite(ll_sw[p]) and np.isfinite(ll_pl[p]):
            assert abs(ll_sw[p] - at_sw) <= 1e-6 and abs(ll_pl[p] - at_pl) <= 1e-6, p    # each run's value is its point's value
        if both[p]:
            worst = max(worst, abs(ll_sw[p] - ll_pl[p]))
            assert abs(ll_sw[p] - ll_pl[p]) <= 1e-6, (p, ll_sw[p], ll_pl[p])
        assert ll_sw[p] >= at_pl - 1e-6 or not both[p], (p, ll_sw[p], at_pl)
        assert ll_pl[p] >= at_sw - 1e-6 or not both[p], (p, ll_pl[p], at_sw)
    print('priors=%s: %d problems converged in both, worst |ll difference| %.3g' % (priors, int(both.sum()), worst))


def model_of(lf):
    """the factored_oracle model of a prepared SourceWiseBinnedLogLikelihood, from its sources"""
    names = list(lf.shape_parameters)
    anchor_z = [np.array(sorted(lf.shape_parameters[n][0])) for n in names]
    own, ps, mus = [], [], []
    for s, name in enumerate(lf.source_name_list):
        params = lf.source_shape_parameters.get(name, {})
        o = tuple(names.index(k) for k in params)
        shape = tuple(len(anchor_z[i]) for i in o)
        srcs = list(lf.anchor_sources[name].values()) if params else [lf.base_model.sources[s]]
        own.append(o)
        ps.append(np.array([x.get_pmf_grid()[0].ravel() for x in srcs]).reshape(shape + (-1,)))
        mus.append(np.array([x.expected_events for x in srcs]).reshape(shape))
    return dict(anchor_z=anchor_z, own=own, ps=ps, mus=mus)


def test_python_end_to_end():
    """The example's model (8 shape parameters x 5 anchors, 4 sources x 2 own parameters) at 20 x 20 bins"""
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(20, 20))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(5)
    d = lf.base_model.simulate()
    lf.set_data(d)
    counts = lf.data_events_per_bin.histogram
    assert counts.sum() == len(d) and lf.supports_gradient
    model = model_of(lf)
    rng = np.random.default_rng(9)
    P = 5
    pts = {n: rng.uniform(-1.9, 1.9, P) for n in names}
    pts.update({'s%d_rate_multiplier' % s: rng.uniform(0.6, 1.5, P) for s in range(4)})
    ll = lf.eval_points(pts)
    ll_g, grads = lf.values_and_gradients(pts)
    np.testing.assert_array_equal(ll_g, ll)
    for p in range(P):
        zp = np.array([pts[n][p] for n in names])
        rp = np.array([pts['s%d_rate_multiplier' % s][p] for s in range(4)])
        want = fo.factored_derivatives(model, zp, rp, counts)
        prior = float(sum(lf.shape_parameters[n][1](zp[i]) for i, n in enumerate(names)))
        check_entries(ll[p] - prior, want['ll'], want['ll_cond'] + abs(prior), what='eval_points[%d]' % p)
        one = lf(**{k: float(v[p]) for k, v in pts.items()})
        assert one == ll[p]
        got = np.array([grads[n][p] - lf.shape_parameters[n][1].slope(zp[i]) for i, n in enumerate(names)]
                       + [grads['s%d_rate_multiplier' % s][p] for s in range(4)])
        check_entries(got, want['grad'], want['grad_cond'] + np.concatenate([np.abs(zp), np.zeros(4)]), what='values_and_gradients[%d]' % p)
    assert lf(np0=2.5) == -np.inf
    limit = lf.one_parameter_interval('s3_rate_multiplier', 4.0, confidence_level=0.9, kind='upper')
    assert np.isfinite(limit) and 0.0 < limit < 4.0
    for name in ('hesse', 'simulate_toys', 'goodness_of_fit', 'asimov', 'fisher_information', 'grid_scan', 'sample_posterior', 'expected_coarse',
                 'bestfit_toys', 'expected_counts'):
        with pytest.raises(NotImplementedError, match='source-wise'):
            getattr(lf, name)()
    with pytest.raises(NotImplementedError, match='source-wise'):
        lf(compute_pdf=True)
