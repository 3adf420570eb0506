"""The expected (Fisher) information on the device (bi_eval_fisher, k_morph_fisher) and what is built on it, against the numpy
oracle (tests/fisher_oracle.py): every kernel variant, the tile edges and both tile orders, unbounded information, the screen,
repeatability and batching, the identity with the observed Hessian of data that equal the expectation, the likelihoods'
fisher_information / expected_covariance, and hesse(information='expected').

The bar is the project's per-entry one, the one tests/test_real_counts_gpu.py holds gradient entries to:
|device - oracle| <= 1e-10 max(1, cond_qr), cond_qr = sum_b |d_q mu_b d_r mu_b| / mu_b from the oracle; the counts of unbounded
bins, the status words, nan and the zeros of single-anchor axes are exact."""
import ctypes as C
import warnings
from collections import OrderedDict

import numpy as np
import pytest

import fisher_oracle as fo
import gof_oracle
import hessian_oracle as ho
import model_zoo
import real_counts_oracle as rco
from fisher_fixtures import FIXTURES, fixture_model, fixture_points, synthetic_model, synthetic_points

pytestmark = pytest.mark.gpu
TOL = 1e-10
VARIANTS = {(4, 4), (8, 4), (8, 8), (16, 8), (16, 16)}
reached = set()                      # the (G, DM) variants the oracle tests of this module went through


@pytest.fixture(scope='module')
def ns():
    return model_zoo.namespace_of('blueice_amd')


def context_of(model, allow_negative=None, **params):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])
    if allow_negative is not None:
        ctx.set_allow_negative([1 if a else 0 for a in allow_negative])
    for k, v in params.items():
        ctx.set_param(k, v)
    return ctx


def variant_of(model):
    """the kernel variant bi_eval_fisher takes for this model (bi_fisher_variant)"""
    from blueice_amd import _capi
    D = sum(len(g) > 1 for g in model['anchor_z']) + model['mus'].shape[-1]
    G, DM = C.c_int(0), C.c_int(0)
    assert _capi.load().bi_fisher_variant(D, C.byref(G), C.byref(DM)) == 0
    return G.value, DM.value


def check_points(got, model, zs, rs, what, allow_negative=None):
    """every point of a call against the oracle -> the worst |err| / max(1, cond)"""
    info, total, unb, st = got
    d = len(model['anchor_z'])
    single = [i for i, g in enumerate(model['anchor_z']) if len(g) < 2]
    worst = 0.0
    for p in range(len(rs)):
        want_st = rco.screen(model, zs[p], rs[p], allow_negative)
        assert st[p] == want_st, '%s point %d: status %d, want %d' % (what, p, st[p], want_st)
        if want_st:
            assert np.isnan(info[p]).all() and np.isnan(total[p]) and not unb[p].any(), '%s point %d' % (what, p)
            continue
        want = fo.information(model, zs[p], rs[p])
        assert np.array_equal(unb[p], want['unbounded']), '%s point %d: unbounded %r, want %r' % (what, p, unb[p], want['unbounded'])
        if want['negative']:
            assert np.isnan(info[p]).all() and np.isnan(total[p]), '%s point %d: a negative expectation' % (what, p)
            continue
        assert np.array_equal(info[p], info[p].T), '%s point %d: not exactly symmetric' % (what, p)
        worst = max(worst, fo.check(info[p], want, '%s point %d' % (what, p), TOL))
        assert abs(total[p] - want['total']) <= TOL * max(1.0, want['total'])
        for i in single:
            assert np.all(info[p][i] == 0.0) and np.all(info[p][:, i] == 0.0) and unb[p][i] == 0
        assert np.all(np.diag(info[p]) >= 0.0)
    assert d == zs.shape[1]
    return worst


@pytest.mark.parametrize('name', FIXTURES)
def test_golden_fixtures_against_the_oracle(name):
    """d = 0 .. 3, non-uniform anchors, a single-anchor axis; points inside cells, on anchors, on both edges of the box, a rate
    scale of 0; nontemporal loads both ways"""
    model = fixture_model(name)
    zs, rs = fixture_points(name)
    reached.add(variant_of(model))
    for nt in (0, 1):
        ctx = context_of(model, nt_loads=nt)
        try:
            got = ctx.eval_fisher(zs if zs.shape[1] else None, rs)
            worst = check_points(got, model, zs, rs, '%s nt_loads %d' % (name, nt))
            assert not got[3].any()
            print('%s, nt_loads %d, variant %s: worst |err| / max(1, cond) = %.3g' % (name, nt, variant_of(model), worst))
        finally:
            ctx.close()


@pytest.mark.parametrize('d,S', [(0, 1), (0, 3), (1, 3), (0, 7), (0, 8), (1, 7), (0, 15), (2, 13), (3, 12)])
def test_every_variant_against_the_oracle(d, S):
    """S from 1 up to the limit 1 + d_eff + S = 16; B = 37 (one partly filled half tile)"""
    rng = np.random.default_rng(1000 + 16 * d + S)
    model = synthetic_model(rng, d, S, 37, anchors=(-1.0, 0.25, 1.0) if d < 3 else (-1.0, 1.0))
    zs, rs = synthetic_points(rng, model, 5)
    reached.add(variant_of(model))
    ctx = context_of(model)
    try:
        worst = check_points(ctx.eval_fisher(zs if d else None, rs), model, zs, rs, 'd %d S %d' % (d, S))
        print('d %d, S %d, variant %s: worst |err| / max(1, cond) = %.3g' % (d, S, variant_of(model), worst))
    finally:
        ctx.close()


def test_every_variant_was_reached():
    """(runs after the two oracle tests above: with them deselected it fails, as it should)"""
    assert reached == VARIANTS, 'variants not reached: %s' % sorted(VARIANTS - reached)


def test_too_many_columns_are_refused_by_name():
    model = synthetic_model(np.random.default_rng(5), 1, 15, 9)          # 1 + 1 + 15 = 17
    ctx = context_of(model)
    try:
        with pytest.raises(ValueError, match='17'):
            ctx.eval_fisher([[0.0]], np.ones((1, 15)))
    finally:
        ctx.close()


@pytest.mark.parametrize('B', [1, 255, 256, 257, 511, 512, 513, 1025])
def test_tile_edges(B):
    """the two 256-bin passes of a 512-bin tile and the tile edges; d = 1, S = 3 (the (8, 4) variant), one and many points"""
    rng = np.random.default_rng(B)
    model = synthetic_model(rng, 1, 3, B)
    zs, rs = synthetic_points(rng, model, 4)
    ctx = context_of(model)
    try:
        worst = check_points(ctx.eval_fisher(zs, rs), model, zs, rs, 'B %d' % B)
        one = ctx.eval_fisher(zs[:1], rs[:1])
        check_points(one, model, zs[:1], rs[:1], 'B %d, one point' % B)
        print('B %d: worst |err| / max(1, cond) = %.3g' % (B, worst))
    finally:
        ctx.close()


def test_tile_chunks_on_a_long_row():
    """193 tiles, tile_chunks 3: 65 tiles per chunk, the last chunk two tiles short; against tile_chunks 1 and the oracle"""
    B = 193 * 512 - 100
    rng = np.random.default_rng(193)
    model = synthetic_model(rng, 1, 2, B, anchors=(-1.0, 1.0))
    zs = np.array([[0.3], [1.0]])
    rs = rng.uniform(0.4, 1.6, size=(2, 2))
    for chunks in (1, 3):
        for nt in (0, 1):
            ctx = context_of(model, tile_chunks=chunks, nt_loads=nt)
            try:
                worst = check_points(ctx.eval_fisher(zs, rs), model, zs, rs, 'tile_chunks %d' % chunks)
                check_points(ctx.eval_fisher(zs[:1], rs[:1]), model, zs[:1], rs[:1], 'tile_chunks %d, one point' % chunks)
                print('tile_chunks %d, nt_loads %d: worst |err| / max(1, cond) = %.3g' % (chunks, nt, worst))
            finally:
                ctx.close()


# ---- the identity with the observed Hessian ---------------------------------------------------------------------------

def whole_number_model(rng, B=700):
    """d = 2, S = 2: rows of whole numbers that are multiples of 4 in [4, 124], unit mus: at corner weights 1/2 and 1/4 and rate
    scales 1 every mu_b is a whole number <= 248, exactly"""
    ps = 4.0 * rng.integers(1, 32, size=(2, 2, 2, B)).astype(float)
    return dict(anchor_z=[np.array([0.0, 1.0]), np.array([0.0, 1.0])], ps=ps, mus=np.ones((2, 2, 2)), n_model=None)


WHOLE_POINTS = np.array([[0.5, 0.5], [0.5, 0.0], [0.0, 0.5], [0.5, 1.0]])


def test_minus_the_hessian_of_data_that_equal_the_expectation():
    """n_b = mu_b as ordinary integer data, bit for bit: the weight n / mu - 1 of bi_eval_hess's second-order terms is 0 (the
    kernel forms n (1 / mu) - 1: 0 or one rounding, 2^-53, far below the bar) and -H is the same sum as I, from another kernel"""
    model = whole_number_model(np.random.default_rng(2))
    rs = np.ones((1, 2))
    from blueice_amd.device import DeviceContext
    for p, z in enumerate(WHOLE_POINTS):
        n = ho._mu_derivatives(model, z, rs[0])[0]
        assert np.all(n == np.floor(n)) and n.max() <= 255 and n.min() >= 1
        ctx = DeviceContext(0)
        try:
            ctx.set_param('sparse', 0)
            ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])
            ctx.upload_counts(n)
            ll, gz, gs, H, st = ctx.eval_hess(z[None], rs)
            info, total, unb, st2 = ctx.eval_fisher(z[None], rs)
        finally:
            ctx.close()
        assert not st.any() and not st2.any() and not unb.any() and np.isfinite(ll[0])
        assert total[0] == n.sum()
        want = fo.information(model, z, rs[0])
        fo.check(info[0], want, 'point %d, information' % p, TOL)
        worst = fo.check(-H[0], dict(info=info[0], cond=want['cond']), 'point %d, -H against I' % p, TOL)
        print('point %s: -H against I, worst |err| / max(1, cond) = %.3g' % (z, worst))


# ---- unbounded information, negative expectations, the screen -----------------------------------------------------------

def test_unbounded_information_is_counted_and_left_out():
    """B = 600 (424 padding bins).  Bin 7: only source 1 fills it; bin 9: only the anchor at 1 fills it; bin 11: nothing does."""
    rng = np.random.default_rng(8)
    B = 600
    ps = rng.uniform(0.1, 1.0, size=(2, 2, B))
    ps[:, 0, 7] = 0.0
    ps[0, :, 9] = 0.0
    ps[:, :, 11] = 0.0
    model = dict(anchor_z=[np.array([0.0, 1.0])], ps=ps, mus=rng.uniform(20.0, 60.0, size=(2, 2)), n_model=None)
    zs = np.array([[0.4], [0.4], [0.0], [1.0], [0.0]])
    rs = np.array([[1.0, 1.0], [1.3, 0.0], [0.7, 1.1], [0.7, 1.1], [0.0, 0.0]])
    ctx = context_of(model)
    try:
        info, total, unb, st = ctx.eval_fisher(zs, rs)
        check_points((info, total, unb, st), model, zs, rs, 'unbounded')
    finally:
        ctx.close()
    assert unb.tolist() == [[0, 0, 0],          # inside the cell, both rates on: every bin but 11 is filled
                            [0, 0, 1],          # source 1 off: bin 7 would fill with it -- for its rate and for nothing else
                            [1, 0, 0],          # on the anchor at 0: bin 9 would fill with z
                            [0, 0, 0],          # on the anchor at 1 (the upper edge, the same cell): bin 9 is filled
                            [0, B - 3, B - 2]]  # nothing expected anywhere: every bin a source fills at this anchor (not 9, 11; 7: source 1 alone)
    assert np.isfinite(info).all() and np.all(info[4] == 0.0) and total[4] == 0.0
    assert info[1][2, 2] > 0          # the bins both sources fill still inform on the rate that is off


def test_a_negative_expectation_gives_a_nan_matrix():
    model = dict(anchor_z=[], ps=np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5]]), mus=np.array([10.0, 5.0]), n_model=None)
    rs = np.array([[1.0, 0.5], [1.0, -1.0], [1.0, 1.0]])          # the second point: mu = (10, -5, 2.5)
    ctx = context_of(model, [False, True])
    try:
        info, total, unb, st = ctx.eval_fisher(None, rs)
        check_points((info, total, unb, st), model, np.zeros((3, 0)), rs, 'allow-negative', [False, True])
    finally:
        ctx.close()
    assert not st.any() and np.isnan(info[1]).all() and np.isnan(total[1]) and np.isfinite(info[[0, 2]]).all()


def test_status_in_a_mixed_batch():
    from blueice_amd import _capi
    model = fixture_model('d2_nonuniform')
    zs, rs = fixture_points('d2_nonuniform')
    zs, rs = np.tile(zs, (2, 1)), np.tile(rs, (2, 1))
    zs[1, 0] = model['anchor_z'][0][-1] + 0.5          # outside the box
    zs[4, 1] = np.nan
    rs[6, 2] = -0.5                                     # an unphysical rate
    rs[9, 0] = np.inf
    ctx = context_of(model)
    try:
        got = ctx.eval_fisher(zs, rs)
        check_points(got, model, zs, rs, 'mixed batch')
        alone = ctx.eval_fisher(np.delete(zs, [1, 4, 6, 9], axis=0), np.delete(rs, [1, 4, 6, 9], axis=0))
    finally:
        ctx.close()
    info, total, unb, st = got
    want = np.zeros(len(zs), dtype=np.int32)
    want[[1, 4]] = _capi.ST_OUT_OF_BOUNDS
    want[[6, 9]] = _capi.ST_UNPHYSICAL
    assert np.array_equal(st, want)
    live = st == 0
    assert np.isnan(info[~live]).all() and np.isfinite(info[live]).all()
    # the neighbours are what they are without the screened points in the call
    assert np.array_equal(info[live], alone[0]) and np.array_equal(total[live], alone[1]) and np.array_equal(unb[live], alone[2])


# ---- repeatability and batching -----------------------------------------------------------------------------------------

def test_repeatable_and_independent_of_the_batch():
    model = fixture_model('d3_small')
    rng = np.random.default_rng(4)
    zs = rng.uniform(-1.0, 1.0, size=(257, 3))
    rs = rng.uniform(0.4, 1.6, size=(257, 4))
    ctx = context_of(model)
    try:
        a = ctx.eval_fisher(zs, rs)
        b = ctx.eval_fisher(zs, rs)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        for p in (0, 100, 256):
            one = ctx.eval_fisher(zs[p:p + 1], rs[p:p + 1])
            for x, y in zip(a, one):
                assert np.array_equal(x[p], y[0]), 'point %d alone and in the batch' % p
    finally:
        ctx.close()


def test_across_the_launch_chunk_seam():
    """65 537 one-bin points: two launches of 65 535 and 2 items.  d = 0, S = 2, B = 1: I = u u^T / (rs . u), u_s = mus_s ps_s --
    the oracle at the seam and at a sample, its closed form everywhere"""
    model = dict(anchor_z=[], ps=np.array([[0.75], [0.5]]), mus=np.array([12.0, 30.0]), n_model=None)
    P = 65537
    rng = np.random.default_rng(6)
    rs = rng.uniform(0.4, 1.6, size=(P, 2))
    ctx = context_of(model)
    try:
        info, total, unb, st = ctx.eval_fisher(None, rs)
    finally:
        ctx.close()
    assert not st.any() and not unb.any()
    u = np.array([12.0 * 0.75, 30.0 * 0.5])
    mu = rs @ u
    want = u[None, :, None] * u[None, None, :] / mu[:, None, None]
    assert np.all(np.abs(info - want) <= TOL * np.maximum(1.0, want)) and np.all(np.abs(total - mu) <= TOL * mu)
    sample = np.concatenate([[0, 65533, 65534, 65535, 65536], rng.choice(P, size=20, replace=False)])
    check_points((info[sample], total[sample], unb[sample], st[sample]), model, np.zeros((len(sample), 0)), rs[sample], 'seam')


# ---- the likelihood classes ---------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def morph(ns):
    """d = 1 (shift), S = 3, a base live time of 2 days; prepared, NO data set"""
    rng = np.random.default_rng(101)
    space = [['x', np.linspace(-4, 4, 31)], ['y', np.linspace(0, 5, 21)]]
    strengths = [1.0, -0.6, 0.45]
    conf = dict(sources=[dict(name='s%d' % s, events_per_day=40. * (s + 1), data=model_zoo.sample(rng, 20000, space), strength=strengths[s])
                         for s in range(3)],
                default_source_class=model_zoo.morphed_source_class(ns), analysis_space=space, force_recalculation=True,
                never_save_to_cache=True, shift=0., stretch=0., tilt=0., livetime_days=2.0)
    lf = ns.BinnedLogLikelihood(conf)
    for s in range(3):
        lf.add_rate_parameter('s%d' % s)
    lf.add_shape_parameter('shift', (-1., 0., 1.))
    lf.prepare()
    return lf, space


def test_no_data_are_needed_and_nothing_resident_is_touched(morph):
    from blueice_amd.coarse import CoarseBinning
    lf, space = morph
    assert not lf.is_data_set
    truth = dict(shift=0.37, s0_rate_multiplier=1.3)
    names, info, unb = lf.fisher_information(**truth)
    assert names == ['s0_rate_multiplier', 's1_rate_multiplier', 's2_rate_multiplier', 'shift'] and np.isfinite(info).all()
    # with a dataset, a real-valued store and a coarse binning resident: all three are what they were
    lf.set_data(model_zoo.sample(np.random.default_rng(3), 150, space))
    p = dict(shift=0.2, s0_rate_multiplier=1.1, s1_rate_multiplier=0.9)
    view = lf.asimov(shift=0.3)
    binning = CoarseBinning(lf, keep=['x'], rebin=dict(x=5))
    coarse = lf.expected_coarse(binning, **p)
    before = (lf(**p), view(**p), lf.ctx.download_counts(0), view.counts(0))
    names2, info2, unb2 = lf.fisher_information(**truth)
    lf.fisher_information_points(dict(shift=np.linspace(-1, 1, 9)))
    after = (lf(**p), view(**p), lf.ctx.download_counts(0), view.counts(0))
    assert np.array_equal(info2, info) and np.array_equal(unb2, unb)          # and the data change nothing in it
    assert before[0] == after[0] and before[1] == after[1] and np.isfinite(before[0]) and np.isfinite(before[1])
    assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
    assert np.array_equal(lf.expected_coarse(binning, **p), coarse)


def oracle_user_information(lf, model, points, livetime_days=None):
    """the oracle's information over (z, rate_scale) carried to the user's parameters by the chain rule tested on the host
    (tests/test_fisher_host.py) -> (I [P, F, F], cond [P, F, F], unbounded [P, F] bool)"""
    from blueice_amd import hessian
    z, scale, _ = lf._batch_terms(points, livetime_days)
    P = len(z)
    mult, L, eff, eff_axis, rate_sources = lf._chain_rule_terms(points, P, livetime_days)
    theta = [fo.information(model, z[p], scale[p]) for p in range(P)]
    info = hessian.chain_rule_information(np.stack([t['info'] for t in theta]), mult, L, eff, eff_axis, rate_sources)
    J = hessian.user_jacobian(P, z.shape[1], scale.shape[1], mult, L, eff, eff_axis, rate_sources)
    cond = np.einsum('pfk,pkl,pgl->pfg', np.abs(J), np.stack([t['cond'] for t in theta]), np.abs(J))
    unb = hessian.chain_rule_unbounded(np.stack([t['unbounded'] for t in theta]), mult, L, eff, eff_axis, rate_sources)
    return info, cond, unb


def test_fisher_information_points_against_the_oracle(ns, morph):
    """a live-time factor (morph), and efficiencies of which one is a shape parameter (efficiency_param)"""
    lf, _ = morph
    rng = np.random.default_rng(12)
    pts = dict(shift=rng.uniform(-1, 1, 6), s0_rate_multiplier=rng.uniform(0.5, 2, 6), s2_rate_multiplier=rng.uniform(0.5, 2, 6))
    pts['shift'][1] = 0.0
    pts['s0_rate_multiplier'][2] = 0.0
    cases = [(lf, pts, 5.0), (lf, pts, None)]
    lf2, _, _ = model_zoo.efficiency_param(ns)
    cases.append((lf2, dict(eff=rng.uniform(0.5, 1.5, 6), shift=rng.uniform(-1, 1, 6), a_rate_multiplier=rng.uniform(0.5, 2, 6),
                            c_rate_multiplier=rng.uniform(0.5, 2, 6)), None))
    for lf_, points, lt in cases:
        model = gof_oracle.tensors_of(lf_)
        names, info, unb = lf_.fisher_information_points(points, livetime_days=lt, priors=False)
        want, cond, want_unb = oracle_user_information(lf_, model, points, lt)
        assert names == lf_._parameter_names() and info.shape == (6, len(names), len(names))
        assert np.array_equal(unb, want_unb)
        assert np.array_equal(info, np.swapaxes(info, 1, 2))                      # symmetry is exact
        err = np.abs(info - want) / np.maximum(1.0, cond)
        print('%s, livetime %s: worst |err| / max(1, cond) = %.3g' % (names, lt, err.max()))
        assert np.all(err <= TOL)
        for p in range(6):
            assert np.linalg.eigvalsh(info[p]).min() >= -1e-10 * np.trace(info[p])
        one = lf_.fisher_information(livetime_days=lt, priors=False, **{k: v[3] for k, v in points.items()})
        assert one[0] == names and np.array_equal(one[1], info[3]) and np.array_equal(one[2], unb[3])


def test_priors_add_their_curvature(morph):
    from blueice_amd.priors import GaussianPrior
    lf, _ = morph
    truth = dict(shift=0.37, s1_rate_multiplier=1.2)
    names, bare, _ = lf.fisher_information(**truth)
    old = lf.rate_parameters['s1'], lf.shape_parameters['shift']
    try:
        lf.rate_parameters['s1'] = GaussianPrior(1.0, 0.25)
        lf.shape_parameters['shift'] = (old[1][0], lambda x: -0.5 * (np.asarray(x) / 0.5) ** 2, old[1][2])
        _, with_priors, _ = lf.fisher_information(**truth)
        _, without, _ = lf.fisher_information(priors=False, **truth)
    finally:
        lf.rate_parameters['s1'], lf.shape_parameters['shift'] = old
    assert np.array_equal(without, bare)
    add = with_priors - bare
    j, k = names.index('s1_rate_multiplier'), names.index('shift')
    assert with_priors[j, j] == bare[j, j] + 1.0 / 0.25 ** 2                      # a GaussianPrior adds exactly 1 / sigma^2
    assert abs(add[k, k] - 4.0) <= 1e-5                                            # a callable: by second differences
    add[j, j] = add[k, k] = 0.0
    assert np.all(add == 0.0)


def test_expected_covariance_and_errors(morph):
    lf, _ = morph
    model = gof_oracle.tensors_of(lf)
    truth = dict(shift=0.37, s0_rate_multiplier=1.3, s1_rate_multiplier=0.8)
    names = lf._parameter_names()
    want, cond, _ = oracle_user_information(lf, model, {k: np.array([v]) for k, v in truth.items()}, 4.0)
    for floating in (None, ['s0_rate_multiplier'], ['shift', 's0_rate_multiplier'], ['s1_rate_multiplier', 's2_rate_multiplier', 'shift']):
        got_names, cov = lf.expected_covariance(floating=floating, livetime_days=4.0, **truth)
        idx = [j for j, n in enumerate(names) if floating is None or n in floating]
        assert got_names == [names[j] for j in idx]
        inv = np.linalg.inv(want[0][np.ix_(idx, idx)])
        # first order: cov' - cov = -cov dI cov with |dI| <= 1e-10 max(1, cond) per entry (twice that for the higher orders)
        bound = 2 * TOL * (np.abs(inv) @ np.maximum(1.0, cond[0][np.ix_(idx, idx)]) @ np.abs(inv))
        assert np.all(np.abs(cov - inv) <= bound), (floating, cov, inv)
        assert np.array_equal(cov, cov.T) and np.all(np.linalg.eigvalsh(cov) > 0)
        errors = lf.expected_errors(floating=floating, livetime_days=4.0, **truth)
        assert list(errors) == got_names and np.array_equal(np.array(list(errors.values())), np.sqrt(np.diag(cov)))
    # errors shrink with live time as 1 / sqrt(t) (no priors here: the information is linear in it)
    e1 = lf.expected_errors(livetime_days=4.0, **truth)['s0_rate_multiplier']
    e4 = lf.expected_errors(livetime_days=16.0, **truth)['s0_rate_multiplier']
    assert abs(e4 / e1 - 0.5) <= 1e-9
    # log10 rates: sigma(log10 m) = sigma(m) / (m ln 10) for a lone parameter
    lone = lf.expected_errors(floating=['s0_rate_multiplier'], livetime_days=4.0, **truth)['s0_rate_multiplier']
    log = lf.expected_errors(floating=['s0_rate_multiplier'], livetime_days=4.0, rates_in_log_space=True, **truth)['s0_rate_multiplier']
    assert abs(log - lone / (1.3 * np.log(10.0))) <= 1e-12 * log
    with pytest.raises(ValueError, match='nonsense'):
        lf.expected_covariance(floating=['nonsense'], **truth)


def test_unbounded_parameters_get_variance_zero_and_one_warning(ns):
    """a signal that alone fills some bins, at multiplier 0: its information is unbounded"""
    data, _ = ns.make_data([dict(n_events=8, x=0.5)])
    space = [['x', np.linspace(0, 1, 5)]]
    rng = np.random.default_rng(9)
    sig = np.zeros(100, dtype=[('source', int), ('x', float)])
    sig['x'] = rng.uniform(0.0, 1.0, 100)
    bkg = sig.copy()
    bkg['x'] = rng.uniform(0.0, 0.49, 100)                   # the background leaves the upper two bins empty
    conf = dict(sources=[dict(name='sig', events_per_day=10., data=sig), dict(name='bkg', events_per_day=50., data=bkg)],
                default_source_class=model_zoo.morphed_source_class(ns), analysis_space=space, force_recalculation=True,
                never_save_to_cache=True)
    lf = ns.BinnedLogLikelihood(conf)
    lf.add_rate_parameter('sig')
    lf.add_rate_parameter('bkg')
    lf.prepare()
    names, info, unb = lf.fisher_information(sig_rate_multiplier=0.0)
    assert unb.tolist() == [True, False] and np.isfinite(info).all()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        _, cov = lf.expected_covariance(sig_rate_multiplier=0.0)
    assert len(rec) == 1 and 'sig_rate_multiplier' in str(rec[0].message)
    assert np.all(cov[0] == 0.0) and np.all(cov[:, 0] == 0.0) and abs(cov[1, 1] - 1.0 / info[1, 1]) <= 1e-15 * cov[1, 1]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        _, cov = lf.expected_covariance(sig_rate_multiplier=1.0)
    assert not rec and np.all(np.linalg.eigvalsh(cov) > 0)


# ---- hesse(information='expected') ---------------------------------------------------------------------------------------

def test_hesse_expected_where_the_observed_route_fails(morph):
    """an all-empty dataset: -H of the rates is 0 (ll is linear in them), the observed route returns nan; the expected one is
    finite and positive definite there"""
    from blueice_amd.inference import hesse
    lf, space = morph
    lf.set_data(model_zoo.sample(np.random.default_rng(3), 0, space))
    values = dict(s0_rate_multiplier=1.0, s1_rate_multiplier=1.0, shift=0.3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        names, cov = hesse(lf, values)
    assert np.isnan(cov).all() and len(rec) == 1
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        names2, cov2 = hesse(lf, values, information='expected')
        many = hesse(lf, {k: np.array([v, v]) for k, v in values.items()}, information='expected')[1]
    assert names2 == names and not rec and np.isfinite(cov2).all() and np.all(np.linalg.eigvalsh(cov2) > 0)
    assert many.shape == (2, 3, 3) and np.array_equal(many[0], cov2) and np.array_equal(many[1], cov2)
    want = lf.expected_covariance(floating=list(values), **values)[1]
    assert np.array_equal(cov2, want)
    with pytest.raises(ValueError, match='bogus'):
        hesse(lf, values, information='bogus')


def test_hesse_expected_and_observed_agree_on_data_that_equal_the_expectation(ns):
    """The whole-number model above under a likelihood (its device tensors replaced by the whole numbers, the data by
    n_b = mu_b): -H == I under the bar, so the two covariances agree to first order in it,
    |cov_e - cov_o| <= 2 x 1e-10 |cov| max(1, cond) |cov| (twice: the bar of either kernel's sum)"""
    from blueice_amd.inference import hesse
    rng = np.random.default_rng(2)
    space = [['x', np.linspace(-4, 4, 701)]]
    lf = model_zoo.morph_lf(ns, rng, 2, space, OrderedDict(shift=(0., 1.), stretch=(0., 1.)), 2000, 50)
    model = whole_number_model(np.random.default_rng(2))
    lf.ctx.set_param('sparse', 0)
    lf.ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])
    for z in WHOLE_POINTS[[0, 1]]:
        n = ho._mu_derivatives(model, z, np.ones(2))[0]
        lf.ctx.upload_counts(n)
        values = dict(s0_rate_multiplier=1.0, s1_rate_multiplier=1.0, shift=z[0], stretch=z[1])
        names, observed = hesse(lf, values)
        names2, expected = hesse(lf, values, information='expected')
        assert names == names2 and np.isfinite(observed).all() and np.isfinite(expected).all()
        want = fo.information(model, z, np.ones(2))
        order = [2, 3, 0, 1]                                 # the user's order: the rates, then the shape parameters
        cond = want['cond'][np.ix_(order, order)]
        bound = 2 * 2 * TOL * (np.abs(expected) @ np.maximum(1.0, cond) @ np.abs(expected))
        err = np.abs(expected - observed)
        print('z %s: expected against observed covariance, worst err / bound = %.3g' % (z, (err / bound).max()))
        assert np.all(err <= bound)
