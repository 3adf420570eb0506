"""Second derivatives of source-wise (factored) models on the device: bi_eval_sourcewise_hess and bi_eval_sourcewise_fisher
against the exact oracles, and the Python layers over them.

The Hessian is held to derivative_oracle.check_entries with C_POISSON = 256, |device - oracle| <= C 2^-52 cond, the oracle being
`derivatives(expand(model), hessian=True)` -- the same likelihood on the full tensor-product grid -- wherever that grid can be
held, and the factored specification (factored_curvature_oracle) with its own cond where it cannot.  The expected information
is held to fisher_oracle.check (1e-10 max(1, cond) per entry), the total to the same relative figure, the unbounded counts to
equality.  ll, gradient and status are eval_grad's bits; "bitwise" means the same bits."""
import numpy as np
import pytest

import factored_curvature_oracle as fc
import factored_oracle as fo
import fisher_oracle
from derivative_oracle import C_POISSON, check_entries, derivatives
from test_factored_gpu import N_ANCHOR, OWN, box_points, model_of, tensor_likelihoods, upload

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
TOL = 1e-10


def oracles(model, expanded=True):
    """-> (hessian oracle(z, rs, n), information oracle(z, rs))"""
    if not expanded:
        return (lambda z, rs, n: fc.curvature(model, z, rs, n)), (lambda z, rs: fc.information(model, z, rs))
    full = fo.expand(model)
    return (lambda z, rs, n: derivatives(full, z, rs, n, hessian=True)), (lambda z, rs: fisher_oracle.information(full, z, rs))


def check_curvature(ctx, model, z, rs, counts, what, dataset=None, expanded=True):
    """every check of one batch of live points -> (worst Hessian ratio, worst information ratio)"""
    hess_oracle, info_oracle = oracles(model, expanded)
    ll, gz, gs, H, st = ctx.eval_hess(z, rs, dataset)
    ll_g, gz_g, gs_g, st_g = ctx.eval_grad(z, rs, dataset)
    assert not st.any()
    for a, b in ((ll, ll_g), (gz, gz_g), (gs, gs_g), (st, st_g)):
        np.testing.assert_array_equal(a, b)                          # eval_grad's bits
    assert np.array_equal(H, H.swapaxes(1, 2))
    info, total, unb, st_f = ctx.eval_fisher(z, rs)
    assert not st_f.any() and np.array_equal(info, info.swapaxes(1, 2))
    nobody = [i for i in range(len(model['anchor_z'])) if not any(i in o for o in model['own'])]
    worst_h = worst_i = 0.0
    for p in range(len(z)):
        n = counts if dataset is None else counts[dataset[p]]
        want = hess_oracle(z[p], rs[p], n)
        worst_h = max(worst_h, check_entries(H[p], want['hess'], want['hess_cond'], what='%s hess[%d]' % (what, p)))
        wi = info_oracle(z[p], rs[p])
        worst_i = max(worst_i, fisher_oracle.check(info[p], wi, what='%s info[%d]' % (what, p), tol=TOL))
        np.testing.assert_array_equal(unb[p], wi['unbounded'])
        assert abs(total[p] - wi['total']) <= TOL * max(1.0, wi['total'])
        assert np.linalg.eigvalsh(info[p]).min() >= -TOL * max(1.0, np.abs(wi['cond']).max())
        assert not H[p][nobody].any() and not H[p][:, nobody].any() and not info[p][nobody].any()
    print('%s: Hessian worst |err| / (2^-52 cond) = %.3g of C = %d; information worst |err| / max(1, cond) = %.3g of %g'
          % (what, worst_h, C_POISSON, worst_i, TOL))
    return worst_h, worst_i


def check_batch_independence(ctx, z, rs):
    """every point alone gives the bits it has in the batch; a repeated call gives the same bits"""
    first = ctx.eval_hess(z, rs)
    for a, b in zip(ctx.eval_hess(z, rs), first):
        np.testing.assert_array_equal(a, b)
    fish = ctx.eval_fisher(z, rs)
    for a, b in zip(ctx.eval_fisher(z, rs), fish):
        np.testing.assert_array_equal(a, b)
    for p in range(len(z)):
        for a, b in zip(ctx.eval_hess(z[p], rs[p:p + 1]), first):
            np.testing.assert_array_equal(a[0], b[p])
        for a, b in zip(ctx.eval_fisher(z[p], rs[p:p + 1]), fish):
            np.testing.assert_array_equal(a[0], b[p])


@pytest.fixture(scope='module')
def small():
    """the d = 3 models of test_factored_gpu at B = 63 and 1001 (a quarter of source 1's bins zero), three datasets each"""
    out = {}
    for B in (63, 1001):
        rng = np.random.default_rng(500 + B)
        model = fo.random_model(rng, N_ANCHOR, OWN, B, zero_quarter=(1,))
        z, rs = box_points(model, rng, 3, on_anchor=False)
        counts = np.stack([rng.poisson(fo.expectation(model, z[t], rs[t])).astype(float) for t in range(3)])
        out[B] = (model, counts)
    return out


@pytest.mark.parametrize('B', [63, 1001])
def test_small_shapes_against_the_oracles_of_the_expansion(small, B):
    """B = 63: less than one tile; B = 1001: two tiles with a ragged tail (two blocks per item)"""
    model, counts = small[B]
    ctx = upload(model, counts[0])
    z, rs = box_points(model, np.random.default_rng(B), 6)          # inside cells, on interior anchors, on the upper edge
    check_curvature(ctx, model, z, rs, counts[0], 'd=3 B=%d' % B)
    check_batch_independence(ctx, z, rs)
    for a, b in zip(ctx.eval_hess(z, None), ctx.eval_hess(z, np.ones_like(rs))):          # no rate scales: ones
        np.testing.assert_array_equal(a, b)
    for a, b in zip(ctx.eval_fisher(z, None), ctx.eval_fisher(z, np.ones_like(rs))):
        np.testing.assert_array_equal(a, b)
    ctx.close()


@pytest.mark.parametrize('case', ['e3x8', 'mixed', 'mixed_padded', 's2_e1', 's2_e2', 's2_e3', 's4_e1', 's8_e1', 's8_e2'])
def test_every_kernel_class(case):
    """The nine cases of test_factored_gpu.test_largest_kernel_class_and_mixed_ownership: every (source slots, own axes) class of
    the kernel, `e3x8` and `s8_e2` with their eight and four Gram panels, `mixed_padded` with padded source slots; axes shared
    between sources in most of them"""
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
    check_curvature(ctx, model, z, rs, counts, case)
    check_batch_independence(ctx, z, rs)
    ctx.close()


def test_many_axes():
    """d = 24, S = 8, three own axes each, 3 anchors per axis, B = 515: no expanded grid exists (3^24 anchors); the oracle is the
    factored specification with its own cond"""
    rng = np.random.default_rng(24)
    own = [(3 * s, 3 * s + 1, 3 * s + 2) for s in range(8)]
    model = fo.random_model(rng, (3,) * 24, own, 515)
    z, rs = box_points(model, rng, 3)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    ctx = upload(model, counts)
    check_curvature(ctx, model, z, rs, counts, 'd=24', expanded=False)
    ctx.close()


def test_status_and_edge_values():
    """test_factored_gpu.test_status_and_edge_values' model and points"""
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
    rs[5, 0] = 0.0
    ds[6] = 1                                               # n > 0 where mu = 0
    ll, gz, gs, H, st = ctx.eval_hess(z, rs, ds)
    ll_g, gz_g, gs_g, st_g = ctx.eval_grad(z, rs, ds)
    np.testing.assert_array_equal(st, [0, ST_OUT_OF_BOUNDS, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET, 0, 0, 0])
    for a, b in ((ll, ll_g), (gz, gz_g), (gs, gs_g), (st, st_g)):
        np.testing.assert_array_equal(a, b)
    for p in (1, 2, 3, 4, 6):                               # 6: mu = 0 and n > 0 in bin 5 -> ll = -inf, a nan Hessian
        assert ll[p] == -np.inf and np.isnan(H[p]).all(), p
    hess_oracle, info_oracle = oracles(model)
    for p in (0, 5, 7):                                     # bin 5 has n = 0 and mu = 0 there: it adds nothing
        want = hess_oracle(z[p], rs[p], counts)
        check_entries(H[p], want['hess'], want['hess_cond'], what='hess[%d]' % p)
        assert not H[p][2].any() and not H[p][:, 2].any() and np.array_equal(H[p], H[p].T)
    # the expected information of the same points: no dataset test, and the empty bin adds nothing and is not counted
    info, total, unb, st_f = ctx.eval_fisher(z, rs)
    np.testing.assert_array_equal(st_f, [0, ST_OUT_OF_BOUNDS, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, 0, 0, 0, 0])
    for p in (1, 2, 3):
        assert np.isnan(info[p]).all() and np.isnan(total[p]) and not unb[p].any(), p
    for p in (0, 4, 5, 6, 7):
        wi = info_oracle(z[p], rs[p])
        fisher_oracle.check(info[p], wi, what='info[%d]' % p, tol=TOL)
        np.testing.assert_array_equal(unb[p], wi['unbounded'])
        assert abs(total[p] - wi['total']) <= TOL * max(1.0, wi['total'])
    # P = 0
    e = ctx.eval_hess(np.zeros((0, 3)), np.zeros((0, 3)))
    assert e[0].shape == (0,) and e[3].shape == (0, 6, 6)
    assert ctx.eval_fisher(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0, 6, 6)
    ctx.close()


def test_unbounded_fixture_and_calls_without_counts():
    """Fisher needs no set_counts and gives exactly [7, 0, 0, 0, 0, 4] on the fixture; the observed call without counts is
    BI_ERR_STATE; every entry point of the grid model keeps refusing the context"""
    from blueice_amd.exceptions import NotPreparedException
    from blueice_amd.source_wise import SourceWiseContext
    model, z, rs, want = fc.unbounded_fixture()
    ctx = SourceWiseContext(0)
    B = fo.n_bins(model)
    ctx.begin_model(model['anchor_z'], 3, B, model['own'])
    for s in range(3):
        rows = np.asarray(model['ps'][s]).reshape(-1, B)
        for k in range(len(rows)):
            ctx.set_anchor(s, k, rows[k], np.asarray(model['mus'][s]).reshape(-1)[k])
    ctx.end_model()
    info, total, unb, st = ctx.eval_fisher(z[None], rs[None])
    assert not st.any()
    np.testing.assert_array_equal(unb[0], want)
    wi = fisher_oracle.information(fo.expand(model), z, rs)
    fisher_oracle.check(info[0], wi, what='unbounded fixture', tol=TOL)
    np.testing.assert_array_equal(wi['unbounded'], want)
    assert abs(total[0] - wi['total']) <= TOL * wi['total']
    with pytest.raises(NotPreparedException, match='no counts uploaded'):
        ctx.eval_hess(z[None], rs[None])
    dev = ctx._dev
    dev.d, dev.S = 3, 3
    for call in (lambda: dev.eval_hess(z[None], rs[None]), lambda: dev.eval_fisher(z[None], rs[None])):
        with pytest.raises(NotPreparedException):
            call()
    ctx.close()


def test_datasets_mixed_in_one_call(small):
    model, counts = small[1001]
    ctx = upload(model, counts)
    z, rs = box_points(model, np.random.default_rng(3), 6)
    ds = np.array([2, 0, 1, 1, 2, 0], dtype=np.int64)
    check_curvature(ctx, model, z, rs, counts, 'T=3', dataset=ds)
    H = ctx.eval_hess(z, rs, ds)[3]
    single = upload(model, counts[2])
    np.testing.assert_array_equal(single.eval_hess(z[ds == 2], rs[ds == 2])[3], H[ds == 2])
    single.close()
    ctx.close()


# ---- the Python class ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nuisances():
    """many_nuisances_config (8 shape parameters x 3 anchors, 4 sources x 2 own parameters) at 6 x 5 bins, with a GaussianPrior
    on every shape parameter but the first and on one rate multiplier"""
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s, log_prior=GaussianPrior(1.0, 0.3) if s == 3 else None)
    for i, n in enumerate(names):
        lf.add_shape_parameter(n, (-1., 0., 1.), log_prior=GaussianPrior(0., 0.8) if i else None)
    lf.prepare()
    model = model_of(lf)
    rng = np.random.default_rng(11)
    truth = dict([(n, float(v)) for n, v in zip(names, rng.uniform(-0.6, 0.6, len(names)))] +
                 [('s%d_rate_multiplier' % s, float(v)) for s, v in enumerate(rng.uniform(0.8, 1.3, 4))])
    zt = np.array([truth[n] for n in names])
    rt = np.array([truth['s%d_rate_multiplier' % s] for s in range(4)])
    expected = fo.expectation(model, zt, rt)
    lf.set_binned_data(rng.poisson(expected).astype(float).reshape(6, 5))
    return lf, names, model, truth, expected


def test_python_hessian_layers(nuisances):
    from blueice_amd import inference
    lf, names, model, truth, _ = nuisances
    assert lf.supports_hessian and lf.hessian_method == 'analytic'
    rng = np.random.default_rng(12)
    pts = {k: v + rng.uniform(-0.2, 0.2, 3) for k, v in truth.items()}
    ll, grads, order, H = lf.values_gradients_hessians(pts)
    assert lf.hessian_method == 'analytic' and order == ['s%d_rate_multiplier' % s for s in range(4)] + names
    ll_d, grads_d, order_d, want = lf._hessian_by_gradient_differences(pts, None, None)
    assert order_d == order
    np.testing.assert_array_equal(ll, ll_d)
    np.testing.assert_allclose(H, want, rtol=0, atol=1e-6 * np.abs(want).max())
    F = len(order)
    # a GaussianPrior's curvature -1 / sigma^2 on the diagonal: the difference to the likelihood without it is exactly that
    lp = {k: lf.shape_parameters[k][1] for k in names}
    sigma2 = np.array([0.3 ** 2 if k == 's3_rate_multiplier' else 0.8 ** 2 if lp.get(k) is not None else np.inf for k in order])
    ll0, gz, gs, Hth, st = lf.ctx.eval_hess(np.stack([pts[n] for n in names], axis=1), np.stack([pts[k] for k in order[:4]], axis=1))
    perm = [len(names) + s for s in range(4)] + list(range(len(names)))      # (z, rs) -> (multipliers, shapes): unit live time, no efficiencies
    data_part = Hth[:, perm][:, :, perm]
    np.testing.assert_allclose(H - data_part, np.tile(np.diag(-1.0 / sigma2), (3, 1, 1)), rtol=0, atol=1e-9 * np.abs(H).max())
    # hesse: inv(-H) of the floating block, the others held
    best = {k: float(v[0]) for k, v in pts.items()}
    floating = {k: best[k] for k in ('s0_rate_multiplier', 's3_rate_multiplier', names[0], names[5])}
    fixed = {k: v for k, v in best.items() if k not in floating}
    got_names, cov = inference.hesse(lf, floating, **fixed)
    idx = [order.index(k) for k in got_names]
    np.testing.assert_allclose(cov, np.linalg.inv(-H[0][np.ix_(idx, idx)]), rtol=1e-9)
    # ... and over an ensemble of datasets
    counts3 = np.stack([lf.ctx.download_counts(0)] * 2 + [np.random.default_rng(13).poisson(nuisances[4]).astype(float)])
    lf.set_binned_data(counts3.reshape(3, 6, 5))
    try:
        _, cov3 = inference.hesse(lf, {k: np.full(3, v) for k, v in floating.items()}, datasets=np.arange(3), **fixed)
        np.testing.assert_array_equal(cov3[0], cov3[1])
        np.testing.assert_allclose(cov3[0], cov, rtol=1e-12)
        assert not np.array_equal(cov3[2], cov3[0])
    finally:
        lf.set_binned_data(counts3[0].reshape(6, 5))


def test_python_bestfit_minuit_and_expected_errors(nuisances):
    from blueice_amd import inference
    lf, names, model, truth, expected = nuisances
    result, value = lf.bestfit_minuit()
    best = {k: v for k, v in result.items() if not k.endswith('_error')}
    assert sorted(best) == sorted(truth) and np.isfinite(value)
    got_names, cov = inference.hesse(lf, best)
    for k, var in zip(got_names, np.diag(cov)):
        assert result[k + '_error'] == np.sqrt(var) and np.isfinite(var), k
    # expected_covariance equals hesse(..., information='expected'); expected_errors are its diagonal
    n1, c1 = lf.expected_covariance(**truth)
    n2, c2 = inference.hesse(lf, truth, information='expected')
    assert n1 == n2
    np.testing.assert_array_equal(c1, c2)
    errors = lf.expected_errors(**truth)
    np.testing.assert_array_equal(np.array([errors[k] for k in n1]), np.sqrt(np.diag(c1)))
    # the two bound names stay refused
    with pytest.raises(NotImplementedError, match='source-wise'):
        lf.hesse()
    with pytest.raises(NotImplementedError, match='source-wise'):
        lf.fisher_information()


def test_python_information_is_minus_the_hessian_of_expected_data():
    """I at a truth = -H of data set to the expectation through set_binned_data(expected), within 1e-10 max(1, cond), through the
    Python layers on both sides.  Counts that are no whole numbers have ll = -inf (scipy's poisson.logpmf) and with it a nan
    Hessian, so the model is one whose expectation is a whole number in every bin, exactly (test_fisher_gpu's construction): rows
    of multiples of 4, unit rates, corner weights 1/2 and 1/4.  The weight n / mu - 1 of the second-order terms is then 0 or one
    rounding and -H is the same sum as I, from the other form of the kernel."""
    rng = np.random.default_rng(2)
    own = ((0,), (1,), (0, 1))
    g = [np.array([0.0, 1.0]), np.array([0.0, 1.0])]
    model = dict(anchor_z=g, own=list(own), ps=[4.0 * rng.integers(1, 32, size=(2,) * len(o) + (63,)).astype(float) for o in own],
                 mus=[np.ones((2,) * len(o)) for o in own])
    lf = None
    for z in (np.array([0.5, 0.5]), np.array([0.5, 1.0])):
        expected = fo.expectation(model, z, np.ones(3))
        assert np.all(expected == np.floor(expected)) and expected.min() >= 1
        if lf is None:
            lf, plain = tensor_likelihoods(model, expected, False)
            plain.ctx.close()
        lf.set_binned_data(expected)
        truth = dict(shape0=np.array([z[0]]), shape1=np.array([z[1]]), s0_rate_multiplier=np.ones(1), s1_rate_multiplier=np.ones(1))
        ll, grads, names, H = lf.values_gradients_hessians(truth)
        names_i, info, unb = lf.fisher_information_points(truth, priors=False)
        assert names == names_i == ['s0_rate_multiplier', 's1_rate_multiplier', 'shape0', 'shape1'] and np.isfinite(ll[0]) and not unb.any()
        wi = fc.information(model, z, np.ones(3))
        perm = [2, 3, 0, 1]                                 # (z_0, z_1, rs_0, rs_1, rs_2) -> the user's order; rs_2 has no parameter
        want = dict(info=wi['info'][np.ix_(perm, perm)], cond=wi['cond'][np.ix_(perm, perm)])
        fisher_oracle.check(info[0], want, what='information at %s' % z, tol=TOL)
        worst = fisher_oracle.check(-H[0], dict(info=info[0], cond=want['cond']), what='-H against I at %s' % z, tol=TOL)
        print('z = %s: -H against I, worst |err| / max(1, cond) = %.3g of %g' % (z, worst, TOL))
    lf.ctx.close()
