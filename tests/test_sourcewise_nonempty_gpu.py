"""The non-empty-bin form of source-wise models on the device (bi_sourcewise_build_nonempty; k_sourcewise_nonempty): bi_eval_factored,
bi_fit_batched_factored, bi_eval_sourcewise_planned and bi_sample_stretch_sourcewise over the listed bins only.

Every comparison of a finite number is derivative_oracle.check_entries with C_POISSON = 256 against `derivatives(expand(model))`,
the same likelihood on the full tensor-product grid, as in tests/test_factored_gpu.py; status words, -inf and nan are exact;
"bitwise" means the same bits.  The fits are held to the 1e-6 in ll that test_factored_gpu.test_native_fit_against_the_grid_model
applies between the source-wise and the grid model.  Every shape is the smallest at which the walk can go wrong: an empty list (one
tile of padding), a few entries, exactly one tile and one tile plus a bin, every bin, a list longer than the blocks of an item, a
chunked walk, and datasets with lists of different lengths in one launch."""
import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_nonempty_oracle as no
import sourcewise_toy_cases as toy_cases
import sourcewise_walk_cases as wc
from derivative_oracle import C_POISSON, check_entries, derivatives
from test_sourcewise_sampler_gpu import assert_planned_is_eval, bits, class_case, planner_points

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
FIT_BAR = 1e-6            # tests/test_factored_gpu.py::test_native_fit_against_the_grid_model
FIT_GTOL = 1e-3           # the gradient tolerance at which `converged` is the loop's to decide: test_native_fits_on_both_forms
CLASSES = list(wc.FAMILIES['load_forms']) + ['s4_e2']
# (bins, listed bins) of the class tests: one tile of padding; a few; exactly one tile, and one tile plus a bin; every bin
LISTS = [(63, 0), (63, 5), (1027, 512), (1027, 513), (1001, 1001)]


def expanded_oracle(model):
    full = fo.expand(model)
    return lambda z, rs, n: derivatives(full, z, rs, n, hessian=False)


def filled_counts(rng, model, z, rs):
    """every bin listed: a Poisson draw at the expectation scaled to 3 events per bin, plus one"""
    mu = fo.expectation(model, z, rs)
    return rng.poisson(mu * (3.0 * len(mu) / mu.sum())).astype(float) + 1.0


def built(ctx, want_nnz=None):
    nnz = ctx.build_nonempty()
    assert ctx.get_param('sourcewise_nonempty_ready') == 1 and ctx.get_param('sourcewise_nonempty_bytes') > 0
    if want_nnz is not None:
        np.testing.assert_array_equal(nnz, want_nnz)
    return nnz


def check_points(ctx, z, rs, counts, oracle, what, dataset=None):
    """value and gradient of every point on the non-empty-bin form against oracle(z, rs, counts) -> the worst ratio"""
    assert ctx.get_param('sourcewise_nonempty_ready') == 1 and ctx.get_param('sourcewise_form') == 1
    ll, gz, gs, st = ctx.eval_grad(z, rs, dataset)
    ll0, st0 = ctx.eval(z, rs, dataset)
    assert not st.any() and not st0.any()
    assert np.array_equal(bits(ll0), bits(ll))                  # values only: the bits of the call with the gradient
    worst = 0.0
    for p in range(len(z)):
        n = counts if dataset is None else counts[dataset[p]]
        want = oracle(z[p], rs[p], n)
        worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (what, p)))
        worst = max(worst, check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='%s grad[%d]' % (what, p)))
    print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (what, worst, C_POISSON))
    return worst


def class_model(name, B):
    """the class's own axes (test_factored_gpu / sourcewise_walk_cases; OWN_4_2 for <4, 2>) on four axes of two anchors at B bins"""
    own = class_case(name)[0]['own']
    rng = np.random.default_rng(sum(name.encode()) + B)
    model = fo.random_model(rng, (2, 2, 2, 2), own, B, zero_quarter=(1,))
    return model, rng


@pytest.mark.parametrize('name', CLASSES)
def test_every_class_at_every_list(name):
    """All nine (source slots, own axes) classes, value and gradient, at the five lists; with no entry ll = -sum_s lambda_s and
    the gradient comes from the row totals alone"""
    worst = 0.0
    for B, nnz in LISTS:
        model, rng = class_model(name, B)
        z, rs = toy_cases.box_points(model, rng, 2)
        counts = filled_counts(rng, model, z[0], rs[0]) if nnz == B else no.sparse_counts(rng, B, nnz)
        ctx = toy_cases.upload(model, counts)
        try:
            built(ctx, [nnz])
            assert ctx.get_param('sourcewise_nonempty_bytes') == 8 * (sum(np.asarray(m).size for m in model['mus']) + 1) * max(512, -(-nnz // 512) * 512)
            worst = max(worst, check_points(ctx, z, rs, counts, expanded_oracle(model), '%s B=%d nnz=%d' % (name, B, nnz)))
            assert ctx.get_param('last_morph_nbx') == max(1, -(-nnz // 512))
            if nnz == 0:
                ll, _ = ctx.eval(z, rs)
                for p in range(2):
                    total = fo.expectation(model, z[p], rs[p]).sum()
                    assert abs(ll[p] + total) <= 1e-12 * total
        finally:
            ctx.close()
    print('%s: worst over the lists %.3g of C = %d' % (name, worst, C_POISSON))


def two_single_axis_sources(B, seed, per_bin=wc.PER_BIN):
    """two sources of one own axis each (four rows), scaled to per_bin expected events per bin"""
    rng = np.random.default_rng(seed)
    model = fo.random_model(rng, (2, 2), [(0,), (1,)], B)
    centre = np.array([0.5 * (g[0] + g[-1]) for g in model['anchor_z']])
    scale = per_bin * B / fo.expectation(model, centre, np.ones(2)).sum()
    model['mus'] = [m * scale for m in model['mus']]
    return model, rng


def test_a_list_longer_than_the_blocks_of_an_item():
    """1026 tiles of listed bins on the 1024 blocks of an item: blocks 0 and 1 walk a second tile, k_finish adds 1024 partials"""
    B = 1026 * 512 - 100
    model, rng = two_single_axis_sources(B, 1026)
    z, rs = toy_cases.box_points(model, rng, 2)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float) + 1.0
    assert np.count_nonzero(counts) == B > 524288
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx, [B])
        check_points(ctx, z[:1], rs[:1], counts, expanded_oracle(model), '1026 tiles')
        assert ctx.get_param('last_morph_nbx') == 1024
        both = ctx.eval(z, rs)[0]
        assert bits(both)[0] == bits(ctx.eval(z[:1], rs[:1])[0])[0]
    finally:
        ctx.close()


def test_chunked_walk():
    """193 tiles of listed bins under tile_chunks = 3: three regions of 65 tiles, the last two tiles short"""
    B = wc.row_bins(wc.CHUNKED_TILES)
    model, rng = two_single_axis_sources(B, 193)
    z, rs = toy_cases.box_points(model, rng, 2)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    listed = np.count_nonzero(counts)
    counts[np.flatnonzero(counts == 0)[:B - listed - 37]] = 1.0      # all but 37 bins listed: still 193 tiles, the last one ragged
    assert -(-np.count_nonzero(counts) // 512) == wc.CHUNKED_TILES
    assert wc.walk(wc.CHUNKED_TILES, 3)[1] == 2
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx)
        oracle = expanded_oracle(model)
        for chunks in (3, 1):
            ctx.set_param('tile_chunks', chunks)
            check_points(ctx, z, rs, counts, oracle, '193 tiles, tile_chunks=%d' % chunks)
    finally:
        ctx.close()


@pytest.fixture(scope='module')
def mixed():
    """B = 2000, four datasets with lists of 0, 5, 513 and 1500 entries: one, one, two and three tiles"""
    B = 2000
    model, rng = class_model('mixed', B)
    counts = np.stack([no.sparse_counts(rng, B, k) for k in (0, 5, 513, 1500)])
    return model, counts


def test_lists_of_different_lengths_in_one_call(mixed):
    """A point has the same bits alone, in a batch of 7 and in a batch of 65 541 across the 65 535-item chunk boundary, with and
    without the gradient, whatever datasets are evaluated beside it"""
    model, counts = mixed
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx, [0, 5, 513, 1500])
        P = 65536 + 5
        rng = np.random.default_rng(65)
        z, rs = toy_cases.box_points(model, rng, P)
        ds = rng.integers(0, 4, P)
        ds[:8] = [0, 1, 2, 3, 3, 2, 1, 0]
        z[17, 0] = model['anchor_z'][0][0] - 1.0            # a rejected point in the batch: the live points close ranks
        ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
        assert ctx.get_param('last_morph_nbx') == 3 and ctx.get_param('last_point_pieces') == 2
        assert st[17] == ST_OUT_OF_BOUNDS and st.sum() == ST_OUT_OF_BOUNDS and np.isfinite(np.delete(ll, 17)).all()
        ll0, st0 = ctx.eval(z, rs, ds)
        assert np.array_equal(bits(ll0), bits(ll)) and np.array_equal(st0, st)
        again = ctx.eval_grad(z, rs, ds)
        for a, b in zip(again, (ll, gz, gs)):
            assert np.array_equal(bits(a), bits(b))
        sevens = np.unique(np.concatenate([np.arange(0, 70, 7), np.arange(65520, P - 7, 7), rng.integers(0, P - 7, 24)]))
        for i in sevens:
            a = ctx.eval_grad(z[i:i + 7], rs[i:i + 7], ds[i:i + 7])
            assert np.array_equal(bits(a[0]), bits(ll[i:i + 7])) and np.array_equal(bits(a[1]), bits(gz[i:i + 7]))
            assert np.array_equal(bits(a[2]), bits(gs[i:i + 7]))
            assert np.array_equal(bits(ctx.eval(z[i:i + 7], rs[i:i + 7], ds[i:i + 7])[0]), bits(ll[i:i + 7]))
        alone = np.unique(np.concatenate([np.arange(8), np.arange(65530, P), rng.integers(0, P, 32)]))
        for p in alone:
            a = ctx.eval_grad(z[p], rs[p:p + 1], ds[p:p + 1])
            assert bits(a[0])[0] == bits(ll)[p] and np.array_equal(bits(a[1][0]), bits(gz[p])) and np.array_equal(bits(a[2][0]), bits(gs[p]))
            assert bits(ctx.eval(z[p], rs[p:p + 1], ds[p:p + 1])[0])[0] == bits(ll)[p]
        assert set(ds[alone]) == {0, 1, 2, 3}
        oracle = expanded_oracle(model)
        sample = np.array([0, 1, 2, 3, 65534, 65535, 65536, P - 1])
        check_points(ctx, z[sample], rs[sample], counts, oracle, 'mixed lists', dataset=ds[sample])
        # ... and the planned route: bit for bit the host route, rejected points included
        zp, rp, dp, _ = planner_points(model, 4, 240, 5)
        llp, stp = assert_planned_is_eval(ctx, zp, rp, dp)
        assert set(np.unique(stp)) == {0, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET} and len(set(dp[stp == 0])) == 4
        assert_planned_is_eval(ctx, z, rs, ds)              # (65 541 points: across the planner's chunk boundary too)
        # the dense route of the same context: the same status words and defaults, values within the two bounds
        ctx.set_param('sourcewise_form', 0)
        lld, gzd, gsd, std = ctx.eval_grad(zp, rp, dp)
        ctx.set_param('sourcewise_form', 1)
        lln, gzn, gsn, stn = ctx.eval_grad(zp, rp, dp)
        assert np.array_equal(stn, std) and np.array_equal(stn, stp) and np.array_equal(bits(lln), bits(llp))
        dead = std != 0
        assert np.all(lln[dead] == -np.inf) and np.all(lld[dead] == -np.inf)
        assert np.isnan(gzn[dead]).all() and np.isnan(gsn[dead]).all() and np.isnan(gzd[dead]).all()
        assert np.allclose(lln[~dead], lld[~dead], rtol=1e-12, atol=0) and not np.array_equal(bits(lln[~dead]), bits(lld[~dead]))
    finally:
        ctx.close()


def test_non_finite_values():
    rng = np.random.default_rng(7)
    own = ((0,), (1,), ())
    model = fo.random_model(rng, (3, 2, 4), own, 63)
    for s in range(3):
        model['ps'][s][..., 5] = 0.0                        # bin 5: every template is 0 at every anchor
    z, rs = toy_cases.box_points(model, rng, 4)
    counts = no.sparse_counts(rng, 63, 6)
    counts[5] = 0.0
    hit, half = counts.copy(), counts.copy()
    hit[5] = 2.0                                            # a listed bin that expects nothing
    half[int(np.flatnonzero(counts)[0])] = 2.5              # a listed count that is no integer
    ctx = toy_cases.upload(model, np.stack([counts, hit, half]))
    try:
        built(ctx)
        ds = np.array([0, 1, 2, 0])
        ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
        assert not st.any()
        for p in (1, 2):
            assert ll[p] == -np.inf and np.isnan(gz[p]).all() and np.isnan(gs[p]).all()
        assert np.array_equal(ctx.eval(z, rs, ds)[0], ll)
        assert np.array_equal(ctx.eval_planned(z, rs, ds)[0], ll)
        oracle = expanded_oracle(model)
        for p in (0, 3):
            want = oracle(z[p], rs[p], counts)
            check_entries(ll[p], want['ll'], want['ll_cond'], what='ll[%d]' % p)
            check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='grad[%d]' % p)
        assert (gz[[0, 3], 2] == 0.0).all()                 # an axis nobody owns has slope 0
        # early exits: the dense route's status words and defaults
        z[0, 2] = model['anchor_z'][2][-1] + 0.25
        z[1, 0] = np.nan
        rs[2, 1] = -0.5
        ds = np.array([0, 0, 0, 3])
        got = ctx.eval_grad(z, rs, ds)
        ctx.set_param('sourcewise_form', 0)
        dense = ctx.eval_grad(z, rs, ds)
        np.testing.assert_array_equal(got[3], [ST_OUT_OF_BOUNDS, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET])
        for a, b in zip(got, dense):
            np.testing.assert_array_equal(a, b)
    finally:
        ctx.close()


def test_what_replaces_the_counts_releases_the_form(mixed):
    model, counts = mixed
    rng = np.random.default_rng(3)
    z, rs = toy_cases.box_points(model, rng, 5)
    ds = np.array([0, 1, 2, 3, 2])
    ctx = toy_cases.upload(model, counts)
    fresh = toy_cases.upload(model, counts)                 # never builds: the dense route's bits
    try:
        dense = fresh.eval_grad(z, rs, ds)
        assert fresh.get_param('sourcewise_nonempty_ready') == 0 and fresh.get_param('sourcewise_nonempty_bytes') == 0
        assert fresh.get_param('sourcewise_form') == 1

        def is_dense(c, want=dense):
            for a, b in zip(c.eval_grad(z, rs, ds), want):
                assert np.array_equal(bits(a), bits(b))
            assert np.array_equal(bits(c.eval_planned(z, rs, ds)[0]), bits(want[0]))

        built(ctx)
        listed = ctx.eval_grad(z, rs, ds)
        assert not np.array_equal(bits(listed[0]), bits(dense[0]))
        ctx.set_param('sourcewise_form', 0)                 # built, but not chosen
        assert ctx.get_param('sourcewise_nonempty_ready') == 1
        is_dense(ctx)
        ctx.set_param('sourcewise_form', 1)
        assert np.array_equal(bits(ctx.eval_grad(z, rs, ds)[0]), bits(listed[0]))
        ctx.set_counts(counts)                              # new counts
        assert ctx.get_param('sourcewise_nonempty_ready') == 0 and ctx.get_param('sourcewise_nonempty_bytes') == 0
        is_dense(ctx)
        built(ctx)
        ctx.drop_nonempty()
        assert ctx.get_param('sourcewise_nonempty_ready') == 0
        is_dense(ctx)
        # a budget below the need: an explicit answer, and the context evaluates densely
        budget = ctx.get_param('compact_budget')
        ctx.set_param('compact_budget', 1000)
        with pytest.raises(ValueError, match='compact_budget'):
            ctx.build_nonempty()
        assert ctx.get_param('sourcewise_nonempty_ready') == 0
        is_dense(ctx)
        ctx.set_param('compact_budget', budget)
        # toys
        built(ctx)
        ctx.generate_toys_points(z[:1], rs[:1], 4, seed=9)
        fresh.generate_toys_points(z[:1], rs[:1], 4, seed=9)
        assert ctx.get_param('sourcewise_nonempty_ready') == 0
        is_dense(ctx, fresh.eval_grad(z, rs, ds))
        nnz = built(ctx)
        assert np.array_equal(nnz, [np.count_nonzero(ctx.download_counts(t)) for t in range(4)])
        # a new model
        B = fo.n_bins(model)
        ctx.begin_model(model['anchor_z'], len(model['own']), B, model['own'])
        assert ctx.get_param('sourcewise_nonempty_ready') == 0
    finally:
        ctx.close()
        fresh.close()


# ---- the Python class -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('priors', [False, True])
def test_native_fits_on_both_forms(priors):
    """64 problems floating two shape parameters and two rate multipliers, with and without Gaussian constraints, on the
    non-empty-bin form and on the dense form of the same context: the maxima agree to FIT_BAR in every one of the 64 problems,
    and all converge in both.

    The gradient tolerance of the fits that must converge is FIT_GTOL, for this reason.  The native loop (bi_fit.h) reports
    `converged` when the projected gradient is below gtol and `stalled` when eight iterations gain less than slow_tol max(1, |f|)
    = 1e-11 x 1e3 = 1e-8 here (or no step lowers f).  A fit whose gradient is g has at most g^2 / (2 lambda) left to gain,
    lambda being the curvature along g -- up to the expected events of a source, a few hundred here, for a rate multiplier.
    Below g = sqrt(2 x 1e-8 x lambda) ~ 1e-3 no run of iterations can gain 1e-8 any more, so a gtol below that asks the loop to
    go on where it must call its steps a stall: whether a problem then ends `converged` (two flat steps) or `stalled` (eight
    crawling ones) is decided by rounding, on either form.  With the default gtol = 1e-6 that is what happens (measured on one
    MI355X: 60 to 64 of 64 converged on either form over ten data recipes, the unchanged dense route included, with no
    preference for a form; this data: 64 and 63 without constraints, 63 and 64 with); those fits are run too and held to FIT_BAR
    alone.  With FIT_GTOL all 64 converge on both forms at every one of the ten recipes, and end within 4e-8 of the maxima of
    the default tolerance."""
    from test_factored_gpu import box_points, tensor_likelihoods
    B = 1001
    rng = np.random.default_rng(500 + B)
    model = fo.random_model(rng, (3, 2, 4), ((0,), (1, 2), ()), B, zero_quarter=(1,))
    rng = np.random.default_rng(64)
    z, rs = box_points(model, rng, 64, on_anchor=False)
    z[:, 2] = 0.5 * (model['anchor_z'][2][1] + model['anchor_z'][2][2])
    rs[:, 2] = 1.0
    counts = np.stack([rng.poisson(0.25 * fo.expectation(model, z[t], rs[t])).astype(float) for t in range(64)])
    sw, plain = tensor_likelihoods(model, counts, priors)
    plain.ctx.close()
    nnz = built(sw.ctx)
    assert nnz.max() < B // 2 and nnz.min() > 0
    fixed = dict(shape2=float(z[0, 2]))
    worst = {}
    for gtol in (1e-6, FIT_GTOL):                            # bestfit_batched's default, then the tolerance reasoned above
        results = {}
        for form in (1, 0):
            sw.ctx.set_param('sourcewise_form', form)
            best, ll, info = sw.bestfit_batched(datasets=np.arange(64), return_info=True, gtol=gtol, **fixed)
            assert info['evaluations'] > 0
            results[form] = (best, ll, info)
        (b1, ll1, i1), (b0, ll0, i0) = results[1], results[0]
        worst[gtol] = float(np.abs(ll1 - ll0).max())
        print('priors=%s gtol=%.0e: worst |ll difference| between the forms %.3g; converged %d (non-empty) and %d (dense) of 64, failed %d and %d'
              % (priors, gtol, worst[gtol], int(i1['converged'].sum()), int(i0['converged'].sum()), int(i1['failed'].sum()),
                 int(i0['failed'].sum())))
        assert not i1['failed'].any() and not i0['failed'].any()
        assert worst[gtol] <= FIT_BAR
    sw.ctx.close()
    assert i1['converged'].all() and i0['converged'].all()   # (at FIT_GTOL)


def nuisance_lf(**likelihood_config):
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(20, 20))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0, **likelihood_config))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    return lf, names


def test_python_end_to_end():
    """nonempty_bins=True against the default on the example's model at 20 x 20 bins: values within the sum of the two oracle
    bounds, fits at FIT_BAR"""
    from blueice_amd import inference
    from test_factored_gpu import model_of
    lf1, names = nuisance_lf(nonempty_bins=True)
    lf0, _ = nuisance_lf()
    np.random.seed(5)
    d = lf1.base_model.simulate()
    d = d[:len(d) // 8]                                     # mostly empty bins
    for lf in (lf1, lf0):
        lf.set_data(d)
    assert lf1.ctx.get_param('sourcewise_nonempty_ready') == 1 and lf0.ctx.get_param('sourcewise_nonempty_ready') == 0
    counts = lf1.data_events_per_bin.histogram
    assert 0 < np.count_nonzero(counts) < counts.size // 2
    model = model_of(lf1)
    rng = np.random.default_rng(9)
    P = 5
    pts = {n: rng.uniform(-1.9, 1.9, P) for n in names}
    pts.update({'s%d_rate_multiplier' % s: rng.uniform(0.6, 1.5, P) for s in range(4)})
    ll1, ll0 = lf1.eval_points(pts), lf0.eval_points(pts)
    (llg1, g1), (llg0, g0) = lf1.values_and_gradients(pts), lf0.values_and_gradients(pts)
    np.testing.assert_array_equal(llg1, ll1)
    for p in range(P):
        zp = np.array([pts[n][p] for n in names])
        rp = np.array([pts['s%d_rate_multiplier' % s][p] for s in range(4)])
        want = fo.factored_derivatives(model, zp, rp, counts)
        prior = abs(float(sum(lf1.shape_parameters[n][1](zp[i]) for i, n in enumerate(names))))
        bound = 2 * C_POISSON * 2.0 ** -52 * (want['ll_cond'] + prior)
        assert abs(ll1[p] - ll0[p]) <= bound, (p, ll1[p], ll0[p], bound)
        assert lf1(**{k: float(v[p]) for k, v in pts.items()}) == ll1[p]
        got1 = np.array([g1[n][p] for n in names] + [g1['s%d_rate_multiplier' % s][p] for s in range(4)])
        got0 = np.array([g0[n][p] for n in names] + [g0['s%d_rate_multiplier' % s][p] for s in range(4)])
        gbound = 2 * C_POISSON * 2.0 ** -52 * (want['grad_cond'] + np.concatenate([np.abs(zp), np.zeros(4)]))
        assert np.all(np.abs(got1 - got0) <= gbound), (p, got1, got0, gbound)
    fits = []
    for lf in (lf1, lf0):
        best, ll = lf.bestfit_device()
        scan = lf.likelihood_ratio_scan(('s3_rate_multiplier', np.array([0.5, 1.0, 1.5, 2.0])))
        fits.append((ll, np.asarray(scan, dtype=float)))
    assert abs(fits[0][0] - fits[1][0]) <= FIT_BAR
    assert fits[0][1].shape == (4,) and np.all(np.abs(fits[0][1] - fits[1][1]) <= 2 * FIT_BAR), fits      # (a difference of two maxima)
    toys = []
    for lf in (lf1, lf0):
        lf.simulate_toys_points({names[0]: np.array([0.3])}, 8, seed=21)
        toys.append(np.asarray(inference.bestfit_toys(lf)[1], dtype=float))
    assert lf1.ctx.get_param('sourcewise_nonempty_ready') == 1 and lf0.ctx.get_param('sourcewise_nonempty_ready') == 0
    assert toys[0].shape == (8,) and np.all(np.abs(toys[0] - toys[1]) <= FIT_BAR), toys
    for lf in (lf1, lf0):
        lf.ctx.close()


def test_sampler_on_the_form_equals_the_host_engine():
    """bi_sample_stretch_sourcewise and the host engine (one bi_eval_factored call per half-step) on the non-empty-bin form: the
    same chain bit for bit, no stream wait in the loop"""
    from blueice_amd.sampler import sample_posterior
    from test_sourcewise_sampler_gpu import nuisance_start
    lf, names = nuisance_lf(nonempty_bins=True, device_histograms=False)
    lf.simulate_toys_points({names[0]: np.array([0.5]), 's0_rate_multiplier': np.array([0.1])}, 3, seed=12)
    assert lf.ctx.get_param('sourcewise_nonempty_ready') == 1
    kw = dict(n_walkers=8, n_steps=20, p0=nuisance_start(lf, 8, 1), seed=6, datasets=[0, 1, 2])
    native = sample_posterior(lf, **kw)
    host = sample_posterior(lf, engine='host', **kw)
    assert native.engine == 'native' and host.engine == 'host' and native.counters[4] == 0
    assert np.array_equal(bits(native.chain), bits(host.chain))
    # (log_prob = ll + the constraint terms, which the host engine adds in NumPy and the device in its own order: to rounding)
    assert np.allclose(native.log_prob, host.log_prob, rtol=1e-13, atol=0)
    lf.ctx.set_param('sourcewise_form', 0)
    dense = sample_posterior(lf, **kw)
    assert not np.array_equal(bits(dense.log_prob), bits(native.log_prob))      # (the form was in use above)
    assert np.allclose(dense.log_prob[0], native.log_prob[0], rtol=1e-10, atol=0)
    lf.ctx.close()
