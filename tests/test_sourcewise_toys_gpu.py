"""Source-wise models on the device: the expectation per bin, the goodness-of-fit sums and the toy generator against their exact
oracles, and the inference layers (toy fits, goodness of fit, Neyman thresholds) on a SourceWiseBinnedLogLikelihood.

Expected counts: every entry against the long-double sum of factored_columns' coefficients times the rows, by
derivative_oracle.check_entries with cond = mu_b (all terms are non-negative) and C = C_POISSON.  Goodness of fit: the long-double
statistics of the expanded grid, 1e-10 max(1, |want|) (test_gof_gpu.py's bar).  Toys: every draw replayed by toy_oracle.per_bin_toys
on the plain NumPy expectation (never the device's); the undecided share of these inputs is held to the cap on the CPU
(test_sourcewise_toys_host.py).  Status words, +inf and "bitwise" are exact."""
import numpy as np
import pytest

import factored_oracle as fo
import gof_oracle
import sourcewise_toy_cases as cases
import toy_oracle as orc
from derivative_oracle import C_POISSON, check_entries

pytestmark = pytest.mark.gpu

TOL = 1e-10
ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16


@pytest.fixture(scope='module')
def inputs():
    return {name: cases.make_case(name) for name in cases.ALL_CASES}


# ---- expected counts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_expected_counts_against_the_exact_sum(inputs, name):
    model, _, _ = inputs[name]
    S, B = len(model['own']), fo.n_bins(model)
    ctx = cases.upload(model)                                   # no counts: none are needed
    z, rs = cases.box_points(model, np.random.default_rng(B + S), 6)
    mu = ctx.expected_counts(z, rs)
    per = ctx.expected_counts(z, rs, per_source=True)
    assert mu.shape == (6, B) and per.shape == (6, S, B)
    worst = 0.0
    for p in range(6):
        want_mu, want_per = cases.exact_expectation(model, z[p], rs[p])
        worst = max(worst, check_entries(mu[p], want_mu, want_mu, what='%s mu[%d]' % (name, p)))
        worst = max(worst, check_entries(per[p], want_per, want_per, what='%s per source[%d]' % (name, p)))
        np.testing.assert_allclose(per[p].sum(axis=0), mu[p], rtol=1e-13, atol=0)
        # a point alone and in the batch of six: the same bits
        np.testing.assert_array_equal(ctx.expected_counts(z[p], rs[p:p + 1])[0], mu[p])
        np.testing.assert_array_equal(ctx.expected_counts(z[p], rs[p:p + 1], per_source=True)[0], per[p])
    print('%s: worst |err| / (2^-52 mu) = %.3g of C = %d' % (name, worst, C_POISSON))
    np.testing.assert_array_equal(ctx.expected_counts(z, rs), mu)                     # repeatable
    np.testing.assert_array_equal(ctx.expected_counts(z, None), ctx.expected_counts(z, np.ones_like(rs)))
    if name == 'zero_both_sides':
        assert (mu[:, cases.ZERO_BINS] == 0.0).all() and (per[:, :, cases.ZERO_BINS] == 0.0).all()
    ctx.close()


def test_expected_counts_rejected_points_and_empty_calls(inputs):
    model, _, _ = inputs['B1001']
    ctx = cases.upload(model)
    z, rs = cases.box_points(model, np.random.default_rng(3), 5)
    good = ctx.expected_counts(z, rs)
    z[1, 2] = model['anchor_z'][2][-1] + 0.25                   # outside the box on an axis
    z[2, 0] = np.nan
    rs[3, 1] = -0.5                                             # an unphysical rate
    mu = ctx.expected_counts(z, rs)
    per = ctx.expected_counts(z, rs, per_source=True)
    for p in (1, 2, 3):
        assert np.isnan(mu[p]).all() and np.isnan(per[p]).all(), p
    for p in (0, 4):                                            # the live points close ranks: the same bits as before
        np.testing.assert_array_equal(mu[p], good[p])
        assert np.isfinite(per[p]).all()
    dev = ctx._dev
    assert dev._lib.bi_sourcewise_expected_counts(dev._h, 0, None, None, 0, None) == 0
    assert dev._lib.bi_sourcewise_generate_toys(dev._h, 0, None, None, None, 0) == 0
    from blueice_amd._capi import ERR_STATE
    from blueice_amd.exceptions import NotPreparedException
    assert dev._lib.bi_eval_sourcewise_gof(dev._h, 0, None, None, None, None, None, None) == ERR_STATE     # it needs counts, whatever P
    with pytest.raises(NotPreparedException, match='no counts'):
        ctx.eval_gof(z, rs)
    with pytest.raises(NotPreparedException, match='no counts'):
        ctx.download_counts(0)
    ctx.close()


# ---- goodness of fit ------------------------------------------------------------------------------------------------------

def _gof_want(full, counts, z, rs):
    w = gof_oracle.statistics(full, counts, z, rs, dtype=np.longdouble)
    return float(w['half_deviance']), float(w['pearson'])


@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_gof_against_the_long_double_statistics_of_the_expansion(inputs, name):
    model, zt, rst = inputs[name]
    full = fo.expand(model)
    rng = np.random.default_rng(len(name) + fo.n_bins(model))
    counts = np.stack([rng.poisson(fo.expectation(model, zt[t], rst[t])).astype(float) for t in range(3)])
    ctx = cases.upload(model, counts)
    z, rs = cases.box_points(model, rng, 6)
    ds = np.arange(6, dtype=np.int64) % 3                       # three datasets addressed through `dataset`
    half, pearson, st = ctx.eval_gof(z, rs, ds)
    assert not st.any()
    for p in range(6):
        want = _gof_want(full, counts[ds[p]], z[p], rs[p])
        for got, w, what in ((half[p], want[0], 'half-deviance'), (pearson[p], want[1], 'pearson')):
            print('%s point %d %s: %r, want %r' % (name, p, what, got, w))
            assert abs(got - w) <= TOL * max(1.0, abs(w)), '%s point %d %s: %r, want %r' % (name, p, what, got, w)
        a = ctx.eval_gof(z[p], rs[p:p + 1], ds[p:p + 1])        # alone: the same bits
        assert a[0][0] == half[p] and a[1][0] == pearson[p] and a[2][0] == 0
    again = ctx.eval_gof(z, rs, ds)
    np.testing.assert_array_equal(again[0], half)
    np.testing.assert_array_equal(again[1], pearson)
    assert ctx._dev._lib.bi_eval_sourcewise_gof(ctx._dev._h, 0, None, None, None, None, None, None) == 0      # P = 0
    h0, p0, _ = ctx.eval_gof(z, rs)                             # dataset NULL: dataset 0
    h00, p00, _ = ctx.eval_gof(z, rs, np.zeros(6, dtype=np.int64))
    np.testing.assert_array_equal(h0, h00)
    np.testing.assert_array_equal(p0, p00)
    ctx.close()


def test_gof_status_and_infinite_values(inputs):
    model, zt, rst = inputs['zero_both_sides']
    rng = np.random.default_rng(12)
    counts = rng.poisson(fo.expectation(model, zt[0], rst[0])).astype(float)
    dead = int(cases.ZERO_BINS[3])
    assert counts[dead] == 0.0
    hit, frac = counts.copy(), counts.copy()
    hit[dead] = 2.0                                             # an event where mu_b = 0
    live = int(np.flatnonzero(counts > 0)[0])
    frac[live] += 0.5                                           # a count that is no integer
    ctx = cases.upload(model, np.stack([counts, hit, frac]))
    z, rs = cases.box_points(model, rng, 8)
    ds = np.zeros(8, dtype=np.int64)
    z[1, 2] = model['anchor_z'][2][-1] + 0.25
    z[2, 0] = np.nan
    rs[3, 1] = -0.5
    ds[4] = 3                                                   # == T
    ds[5] = 1
    ds[6] = 2
    ds[7] = -1
    half, pearson, st = ctx.eval_gof(z, rs, ds)
    np.testing.assert_array_equal(st, [0, ST_OUT_OF_BOUNDS, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET, 0, 0, ST_BAD_DATASET])
    for p in range(1, 8):
        assert half[p] == np.inf and pearson[p] == np.inf, p
    want = _gof_want(fo.expand(model), counts, z[0], rs[0])
    assert abs(half[0] - want[0]) <= TOL * max(1.0, want[0]) and abs(pearson[0] - want[1]) <= TOL * max(1.0, want[1])
    ll, _ = ctx.eval(z, rs, ds)                                 # +inf exactly where the likelihood is -inf
    np.testing.assert_array_equal(np.isinf(ll), np.isinf(half))
    ctx.close()


# ---- toys -----------------------------------------------------------------------------------------------------------------

def _download(ctx, T):
    return np.stack([ctx.download_counts(t) for t in range(T)])


@pytest.mark.parametrize('offset', cases.TOY_OFFSETS)
@pytest.mark.parametrize('name', cases.ALL_CASES)
def test_toys_replayed_draw_for_draw(inputs, name, offset):
    """H = 3 with n_toys = (3, 0, 5) and the same truths one by one (H = 1): every toy replayed against the oracle on the NumPy
    expectation, the grouping invariance bitwise, no event where mu_b = 0, B counts per dataset however the rows are padded"""
    model, z, rs = inputs[name]
    B = fo.n_bins(model)
    ctx = cases.upload(model)                                   # toys need no counts
    ctx.set_param('toy_offset', offset)
    methods = ctx.generate_toys_points(z, rs, cases.N_TOYS, cases.SEED)
    np.testing.assert_array_equal(methods, [0, -1, 0])
    T = sum(cases.N_TOYS)
    assert ctx.T == T
    dev = _download(ctx, T)
    assert dev.shape == (T, B)
    h_of = cases.truth_of_toy(cases.N_TOYS)
    draws = undecided = 0
    for h in range(3):
        mine = np.flatnonzero(h_of == h)
        if not len(mine):
            continue
        mu = fo.expectation(model, z[h], rs[h])
        rep = orc.per_bin_toys(mu, cases.SEED, (offset + mine).astype(np.uint64))
        d, u, _ = orc.compare_toys(dev[mine], rep, what='%s offset %d truth %d' % (name, offset, h))
        draws, undecided = draws + d, undecided + u
        assert (dev[mine][:, mu == 0.0] == 0.0).all()
        # the same toys from an H = 1 call with toy_offset advanced by the toys before it: the same bits
        ctx.set_param('toy_offset', offset + int(mine[0]))
        ctx.generate_toys_points(z[h:h + 1], rs[h:h + 1], [len(mine)], cases.SEED)
        assert ctx.T == len(mine)
        np.testing.assert_array_equal(_download(ctx, len(mine)), dev[mine])
    print('%s offset %d: %d draws replayed, %d undecided' % (name, offset, draws, undecided))
    with pytest.raises(ValueError, match='outside'):
        ctx.download_counts(ctx.T)
    ctx.set_param('toy_offset', 0)
    ctx.close()


def test_toy_lgamma_sums_and_evaluation_of_the_resident_toys(inputs):
    """bi_eval_factored on toy t equals bi_eval_factored after bi_factored_set_counts of the downloaded counts, bitwise"""
    for name in ('B63', 'zero_both_sides', 'B1027'):
        model, z, rs = inputs[name]
        ctx = cases.upload(model)
        ctx.generate_toys_points(z, rs, cases.N_TOYS, cases.SEED)
        T = sum(cases.N_TOYS)
        toys = _download(ctx, T)
        zp, rp = cases.box_points(model, np.random.default_rng(5), T)
        ds = np.arange(T, dtype=np.int64)
        on_toys = ctx.eval_grad(zp, rp, ds)
        gof_toys = ctx.eval_gof(zp, rp, ds)
        assert np.isfinite(on_toys[0]).all()
        other = cases.upload(model, toys)
        uploaded = other.eval_grad(zp, rp, ds)
        for a, b in zip(on_toys, uploaded):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(gof_toys, other.eval_gof(zp, rp, ds)):
            np.testing.assert_array_equal(a, b)
        other.close()
        ctx.close()


def test_refused_truth_leaves_the_old_counts(inputs):
    model, z, rs = inputs['B1001']
    rng = np.random.default_rng(8)
    counts = rng.poisson(fo.expectation(model, z[0], rs[0])).astype(float)
    ctx = cases.upload(model, counts)
    before = ctx.eval_grad(z, rs)
    bad_z = z.copy()
    bad_z[1, 0] = model['anchor_z'][0][0] - 1.0
    with pytest.raises(ValueError, match=r'truth 1\).*outside the anchor box'):
        ctx.generate_toys_points(bad_z, rs, cases.N_TOYS, cases.SEED)
    bad_rs = rs.copy()
    bad_rs[2, 0] = -1.0
    with pytest.raises(ValueError, match=r'truth 2\)'):
        ctx.generate_toys_points(z, bad_rs, cases.N_TOYS, cases.SEED)
    with pytest.raises(ValueError, match='T >= 1'):
        ctx.generate_toys_points(z, rs, [0, 0, 0], cases.SEED)
    with pytest.raises(ValueError, match='negative'):
        ctx.generate_toys_points(z, rs, [1, -1, 0], cases.SEED)
    assert ctx.T == 1
    np.testing.assert_array_equal(ctx.download_counts(0), counts)
    dev = ctx._dev
    out = np.empty(fo.n_bins(model))
    from blueice_amd._capi import ptr
    assert dev._lib.bi_sourcewise_download_counts(dev._h, 0, ptr(out)) == 0      # ... and from the device
    np.testing.assert_array_equal(out, counts)
    for a, b in zip(ctx.eval_grad(z, rs), before):
        np.testing.assert_array_equal(a, b)
    ctx.close()


def test_more_toys_than_one_launch_takes(inputs):
    """32 768 toys per launch: 32 770 toys of the B = 1 model cross the boundary; the first and last toys replayed"""
    model, z, rs = inputs['B1']
    ctx = cases.upload(model)
    ctx.generate_toys_points(z[:1], rs[:1], [cases.LAUNCH_TOYS], cases.SEED)
    assert ctx.T == cases.LAUNCH_TOYS
    mu = fo.expectation(model, z[0], rs[0])
    pick = np.array(cases.LAUNCH_BOUNDARY_TOYS)
    rep = orc.per_bin_toys(mu, cases.SEED, pick.astype(np.uint64))
    orc.compare_toys(np.stack([ctx.download_counts(int(t)) for t in pick]), rep, what='launch boundary')
    ll, st = ctx.eval(np.tile(z[0], (6, 1)), np.tile(rs[0], (6, 1)), pick)
    assert np.isfinite(ll).all() and not st.any()
    ctx.close()


# ---- the Python layers ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nuisance_lf():
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(4, 4))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(5)
    lf.set_data(lf.base_model.simulate())
    return lf, names


def test_toy_mc_fits_do_not_depend_on_the_chunk(nuisance_lf):
    from blueice_amd import inference
    lf, names = nuisance_lf
    own = lf.ctx.download_counts(0)
    a, ll_a = inference.toy_mc_fits(lf, 8, chunk=3, seed=21)
    b, ll_b = inference.toy_mc_fits(lf, 8, chunk=8, seed=21)
    assert len(ll_a) == 8 and np.isfinite(ll_a).all()
    np.testing.assert_allclose(ll_a, ll_b, rtol=1e-9, atol=1e-9)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-9, atol=1e-9)
    fits, ll = inference.bestfit_toys(lf)                       # the toys of the last chunk are the likelihood's data
    assert len(ll) == 8
    np.testing.assert_allclose(ll, ll_b, rtol=1e-9, atol=1e-9)
    lf.set_binned_data(own.reshape(lf.bin_shape))


def test_goodness_of_fit_with_toys(nuisance_lf):
    from blueice_amd import inference
    lf, names = nuisance_lf
    own = lf.ctx.download_counts(0)
    res = inference.goodness_of_fit(lf, n_toys=8, chunk=3, seed=2)
    assert len(res.toys) == 8 and np.isfinite(res.toys).all() and np.isfinite(res.observed)
    assert 0 < res.p_value <= 1
    assert res.ndof == 16 - (4 + len(names))
    assert lf.ctx.T == 1
    np.testing.assert_array_equal(lf.ctx.download_counts(0), own)          # the likelihood's own data, bit for bit
    same = inference.goodness_of_fit(lf, n_toys=8, chunk=8, seed=2)
    np.testing.assert_allclose(res.toys, same.toys, rtol=1e-9, atol=1e-9)
    # the observed statistic is the statistic of the data at the fit, and the expectation there sums to about the data
    stats_ = inference.gof_statistics(lf, **res.best)
    assert stats_['deviance'][0] == res.observed and stats_['n_events'][0] == own.sum()
    mu = inference.expected_counts_points(lf, {k: np.array([v]) for k, v in res.best.items()}, per_source=True)
    assert mu.shape == (1, 4) + tuple(lf.bin_shape)
    assert abs(mu.sum() - own.sum()) < 5 * np.sqrt(own.sum()) + 5
    with pytest.raises(NotImplementedError, match='binning'):
        inference.goodness_of_fit(lf, n_toys=2, binning=object())


def test_toy_test_statistics_and_neyman_thresholds(nuisance_lf):
    from blueice_amd import inference
    lf, names = nuisance_lf
    own = lf.ctx.download_counts(0)
    target = 's3_rate_multiplier'
    st = lf.toy_test_statistics(target, [0.8, 1.4], 4, seed=9, kind='upper')
    assert st.t.shape == (2, 4) and np.isfinite(st.t).all() and (st.t >= -1e-9).all()
    np.testing.assert_array_equal(lf.ctx.download_counts(0), own)
    chunked = lf.toy_test_statistics(target, [0.8, 1.4], 4, seed=9, kind='upper', chunk=3)     # chunks across the hypotheses
    np.testing.assert_allclose(chunked.t, st.t, rtol=1e-9, atol=1e-9)
    table = inference.ToyThresholds.from_statistics(st)
    assert np.isfinite(table(1.0, 0.7))
    limit = lf.one_parameter_interval(target, 6.0, confidence_level=0.7, kind='upper', t_ppf=table)
    assert np.isfinite(limit) and 0.0 < limit < 6.0
    table2 = lf.neyman_thresholds(target, [0.8, 1.4], 4, seed=9, kind='upper')
    np.testing.assert_allclose(table2.t, table.t, rtol=1e-9, atol=1e-9)
