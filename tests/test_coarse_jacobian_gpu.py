"""Derivatives of coarse views on the device: bi_expected_coarse_jacobian against the per-bin derivatives of the numpy oracle
(tests/hessian_oracle._mu_derivatives, what tests/fisher_oracle.py uses) summed in long double over `CoarseBinning.bin_map()`,
at the shapes of tests/test_coarse_gpu.py that reach every path of the kernel and one more for its 16-column variant, for every
kind of coarsening; the refusals of the C ABI; and the likelihood classes' expected_coarse_jacobian(_points),
expected_coarse_band and coarse_information end to end.

The bar is tests/fisher_oracle.check's: |got - want| <= TOL max(1, cond) per entry, TOL = 1e-10 (tests/test_gof_gpu.py).  cond
is the sum over the cell's fine bins and the point's corner rows of |coefficient x template entry|: derivatives along z are
differences of corner rows that cancel inside a cell, so |want| alone is the wrong scale for them.  The coefficients are formed
from the oracle's own interpolation -- the weight of every anchor at z is the interpolation of an identity tensor, its slope the
face difference of tests/hessian_oracle._derivatives -- by the product rule d(w r) = dw r + w dr."""
from collections import OrderedDict

import numpy as np
import pytest

import fisher_oracle as fo
import gof_oracle
import hessian_oracle as ho
import model_zoo
from blueice_amd import coarse, hessian
from blueice_amd.coarse import CoarseBinning
from golden_util import load_case
from test_coarse_gpu import SHAPES, binnings_of, bits, ns, reduce_wide, set_binning, zoo  # noqa: F401  (ns, zoo: fixtures)
from test_gof_gpu import TOL, case_of, context_of

pytestmark = pytest.mark.gpu

# The shapes of tests/test_coarse_gpu.py and what they reach in k_morph_coarse_jac: G = 4 columns and one masked x-tile (B = 63,
# d = 0), G = 8 and four sub-rows of 64 lanes (30 x 20 with three sources, 9 x 7 with two shape parameters), odd L and unaligned
# rows (5 x 4 x 7), two shares (33 x 9 with four sub-rows, 9 x 130 with one), the finish by a block per cell (B = 600).  Two more:
# 9 x 7 with two shape parameters and SIX sources, 1 + 2 + 6 = 9 columns: G = 16; and the 9 x 7 model cut down to ONE anchor on
# its second axis (d = 2, d_eff = 1: the row of that axis must be exactly 0).
S6 = 'k2_9x7_d2_S6'
SINGLE = 'k2_9x7_d2_single_anchor'
NAMES = ['k1_B63_d0', 'k2_30x20_d1_S3', 'k2_9x7_d2', 'k3_5x4x7_d1', 'k2_33x9_d0', 'k2_9x130_d1', 'k1_B600_d1', S6, SINGLE]
COLUMNS = {'k1_B63_d0': 4, 'k2_30x20_d1_S3': 8, 'k2_9x7_d2': 8, 'k3_5x4x7_d1': 4, 'k2_33x9_d0': 4, 'k2_9x130_d1': 4, 'k1_B600_d1': 4,
           S6: 16, SINGLE: 4}


@pytest.fixture(scope='module')
def models(zoo, ns):  # noqa: F811
    """name -> (likelihood whose analysis space the binnings are made for, anchor tensors, analysis space)"""
    out = OrderedDict((name, (zoo[name][0], zoo[name][1], SHAPES[name]['space'])) for name in NAMES if name in SHAPES)
    s = SHAPES['k2_9x7_d2']
    lf = model_zoo.morph_lf(ns, np.random.default_rng(377), 6, s['space'], s['anchors'], 20000, 150)
    out[S6] = (lf, gof_oracle.tensors_of(lf), s['space'])
    lf, model, _ = zoo['k2_9x7_d2']
    az = [np.asarray(g, dtype=float) for g in model['anchor_z']]
    out[SINGLE] = (lf, dict(model, anchor_z=[az[0], az[1][1:2]], ps=np.asarray(model['ps'])[:, 1:2], mus=np.asarray(model['mus'])[:, 1:2]),
                   s['space'])
    return out


def points_of(name, model, seed):
    """`case_of`'s tensors (a floor under every template, one bin without expectation) and its five points -- on an anchor, inside a
    cell, on the edge of the box, outside it, with a negative rate --, one copy of each"""
    model, counts, zs, rs, _, _ = case_of(model, seed=seed)
    T = len(counts)
    zs, rs = zs[::T].copy(), rs[::T].copy()
    if name == SINGLE:
        zs[:, 1] = model['anchor_z'][1][0]                # (the box of a single-anchor axis is its anchor)
    return model, counts, zs, rs


def derivatives(model, z, rs):
    """-> (mu [B], dmu [d + S, B]) of the oracle, and cond [1 + d + S, B]: per fine bin the sum over the corner rows of
    |coefficient x template entry| of the value (row 0) and of every derivative"""
    anchor_z = [np.asarray(g, dtype=float) for g in model['anchor_z']]
    d, S = len(anchor_z), len(rs)
    z, rs = np.asarray(z, dtype=float), np.asarray(rs, dtype=float)
    mu, dmu = ho._mu_derivatives(model, z, rs)[:2]
    shape = tuple(len(g) for g in anchor_z)
    A = int(np.prod(shape, dtype=np.int64))
    w, dw, _ = ho._derivatives(anchor_z, np.eye(A).reshape(shape + (A,)), z)           # the weight of every anchor at z, and its slopes
    u, du, _ = ho._derivatives(anchor_z, model['mus'], z)                             # the interpolated rates [S]
    T = np.abs(np.asarray(model['ps'], dtype=float)).reshape(A, S, -1)
    coef = np.zeros((1 + d + S, A, S))
    coef[0] = w[:, None] * (rs * u)[None, :]
    for i in range(d):
        coef[1 + i] = dw[i][:, None] * (rs * u)[None, :] + w[:, None] * (rs * du[i])[None, :]
    for s in range(S):
        coef[1 + d + s, :, s] = w * u[s]
    return mu, dmu, np.einsum('gas,asb->gb', np.abs(coef), T)


def check(got, want, cond, what):
    """fisher_oracle.check's bound on arrays of cells -> the largest |err| / (TOL max(1, cond))"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - want)
    bound = TOL * np.maximum(1.0, cond)
    assert np.all(err <= bound), '%s: off by %.3g of TOL max(1, cond)' % (what, float(np.max(err / bound)))
    return float(np.max(err / bound)) if err.size else 0.0


@pytest.mark.parametrize('name', NAMES)
def test_bi_expected_coarse_jacobian_against_the_oracle(models, name):
    """Every binning of the shape at the points of `case_of`: mu and every row of jac against the oracle's per-bin values summed
    in long double; the status words and the BITS of mu are bi_expected_coarse's (the same fma chain in the same order), a dead
    point is nan throughout, rows of single-anchor axes are exactly 0, a repeated call is bitwise equal and a point alone has the
    bits it has in the batch."""
    lf, tensors, space = models[name]
    model, counts, zs, rs = points_of(name, tensors, seed=41)
    P, d, S = len(zs), zs.shape[1], rs.shape[1]
    F = d + S
    d_eff = sum(1 for g in model['anchor_z'] if len(g) > 1)
    assert COLUMNS[name] == (4 if 1 + d_eff + S <= 4 else 8 if 1 + d_eff + S <= 8 else 16)
    live = np.array([True, True, True, d == 0, False])
    fine = {p: derivatives(model, zs[p], rs[p]) for p in np.flatnonzero(live)}
    ctx = context_of(model, counts, 0)
    worst = 0.0
    try:
        for label, b in binnings_of(lf, space).items():
            what = '%s, %s' % (name, label)
            set_binning(ctx, lf, b)
            total, status = ctx.expected_coarse(b.n_cells, zs if d else None, rs)
            mu, jac, st = ctx.expected_coarse_jacobian(b.n_cells, zs if d else None, rs)
            assert mu.shape == (P, b.n_cells) and jac.shape == (P, F, b.n_cells) and st.dtype == np.int32
            assert np.array_equal(st, status) and np.array_equal(status == 0, live), what
            assert np.isnan(mu[~live]).all() and np.isnan(jac[~live]).all(), what
            assert np.all(np.isfinite(mu[live])) and np.all(np.isfinite(jac[live])), what
            assert np.array_equal(bits(mu[live]), bits(total[live])), what + ': mu is not bi_expected_coarse bit for bit'
            for p in np.flatnonzero(live):
                mu_b, dmu_b, cond_b = fine[p]
                cond = np.asarray(reduce_wide(b, cond_b), dtype=float)
                worst = max(worst, check(mu[p], reduce_wide(b, mu_b), cond[0], what + ', mu of point %d' % p),
                            check(jac[p], reduce_wide(b, dmu_b), cond[1:], what + ', jac of point %d' % p))
            for i, g in enumerate(model['anchor_z']):
                if len(g) == 1:
                    assert np.all(jac[live][:, i] == 0.0), what + ': the row of a single-anchor axis'
            again = ctx.expected_coarse_jacobian(b.n_cells, zs if d else None, rs)
            assert np.array_equal(bits(again[0]), bits(mu)) and np.array_equal(bits(again[1]), bits(jac)), what
            alone = ctx.expected_coarse_jacobian(b.n_cells, zs[1:2] if d else None, rs[1:2])
            assert np.array_equal(bits(alone[0][0]), bits(mu[1])) and np.array_equal(bits(alone[1][0]), bits(jac[1])), what
    finally:
        ctx.close()
    print('%s (G = %d): the worst entry is at %.3g of TOL max(1, cond)' % (name, COLUMNS[name], worst))


def test_the_c_abi_refusals(models):
    """No binning set (and a binning that a new model released), more than 16 coefficient columns refused by name -- 16 are taken --,
    Beeston-Barlow and unbinned contexts."""
    from blueice_amd.device import DeviceContext
    from blueice_amd.exceptions import NotPreparedException
    lf, tensors, _ = models['k2_9x7_d2']
    model, counts, zs, rs = points_of('k2_9x7_d2', tensors, seed=43)
    ctx = context_of(model, counts, 0)
    try:
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse_jacobian(1, zs, rs)
        assert ctx.set_coarse_binning([9, 7], [[0, 4, 9], [1, 2, 7]]) == 4
        mu, jac, st = ctx.expected_coarse_jacobian(4, zs[:1], rs[:1])
        assert st[0] == 0 and np.all(np.isfinite(mu)) and np.all(np.isfinite(jac))
        ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])          # a new model releases the binning
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse_jacobian(4, zs, rs)
    finally:
        ctx.close()
    rng = np.random.default_rng(44)
    B = 12
    for S in (15, 16):                                                          # d = 0: 1 + S columns
        ps = rng.uniform(0.0, 1.0, size=(S, B))
        wide = dict(anchor_z=[], ps=ps / ps.sum(axis=1, keepdims=True), mus=rng.uniform(5.0, 50.0, size=S), n_model=None)
        ctx = context_of(wide, np.zeros((1, B)), 0)
        try:
            assert ctx.set_coarse_binning([B], [[0, 5, B]]) == 2
            r = rng.uniform(0.6, 1.5, size=(1, S))
            if S == 16:
                with pytest.raises(ValueError, match='17 exceeds 16 coefficient columns'):
                    ctx.expected_coarse_jacobian(2, None, r)
                total, _ = ctx.expected_coarse(2, None, r)                      # (the value alone has no such limit)
                assert np.all(np.isfinite(total))
            else:
                mu, jac, st = ctx.expected_coarse_jacobian(2, None, r)
                want = wide['mus'][:, None] * np.stack([wide['ps'][:, :5].sum(axis=1), wide['ps'][:, 5:].sum(axis=1)], axis=1)
                assert st[0] == 0 and np.all(np.abs(jac[0] - want) <= TOL * np.maximum(1.0, want))
                assert np.all(np.abs(mu[0] - r[0] @ want) <= TOL * np.maximum(1.0, r[0] @ want))
        finally:
            ctx.close()
    c = load_case('ref_bb_multi_bin')
    ctx = DeviceContext(0)
    try:
        ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'], n_model=c['model']['n_model'], bb_source=c['bb_source'])
        ctx.upload_counts(c['counts'])
        with pytest.raises(ValueError, match='Beeston-Barlow'):
            ctx.expected_coarse_jacobian(1, None, np.ones((1, c['S'])))
    finally:
        ctx.close()
    c = load_case('unb_d0_three_sources')
    ctx = DeviceContext(0)
    try:
        n_ev = c['bins'][0]
        ctx.begin_model(c['model']['anchor_z'], c['S'], n_ev)
        ctx.set_anchor(0, np.asarray(c['model']['ps']).reshape(c['S'], n_ev), np.asarray(c['model']['mus']).reshape(c['S']))
        ctx.end_model()
        ctx.set_unbinned(c['outlier'])
        with pytest.raises(ValueError, match='unbinned'):
            ctx.expected_coarse_jacobian(1, None, np.ones((1, c['S'])))
    finally:
        ctx.close()


# ---- the likelihood classes, on the 30 x 20 model (three sources, one shape parameter, base live time 2.0) ----

LIVETIME = 5.0                  # of a base live time of 2.0: the chain rule to the user's parameters is not the identity


@pytest.fixture(scope='module')
def end_to_end(zoo):  # noqa: F811
    lf, model, _ = zoo['k2_30x20_d1_S3']
    factor = LIVETIME / SHAPES['k2_30x20_d1_S3']['livetime']
    rng = np.random.default_rng(51)
    P = 3
    points = OrderedDict(('s%d_rate_multiplier' % s, rng.uniform(0.6, 1.5, P)) for s in range(3))
    points['shift'] = np.array([0.37, -0.45, 0.81])                # strictly inside a cell of the anchors (-1, 0, 1)
    return lf, model, factor, points, binnings_of(lf, SHAPES['k2_30x20_d1_S3']['space'])


def user_cond(model, b, factor, point):
    """cond [F, C] in the user's parameters (three rate multipliers, then shift): sum_k |d theta_k / d parameter| cond_k"""
    mult = np.array([point['s%d_rate_multiplier' % s] for s in range(3)])
    _, _, cond_b = derivatives(model, [point['shift']], mult * factor)
    cond = np.asarray(reduce_wide(b, cond_b[1:]), dtype=float)                       # [d + S, C], theta = (z, rate_scale)
    U = hessian.user_jacobian(1, 1, 3, mult[None, :], factor, np.ones((1, 3)), [-1, -1, -1], [0, 1, 2])[0]     # [F, d + S]
    return np.abs(U) @ cond


def test_jacobian_points_against_central_differences(end_to_end):
    """expected_coarse_jacobian_points against central differences of expected_coarse_points at points strictly inside a cell,
    step h = 1e-3 of the cell's width for the shape parameter and of the multiplier for a rate multiplier.  mu_C is a polynomial
    of degree <= 2 in each parameter there (the rates and the templates are both linear in z), so a central difference is exact
    up to the rounding of its two values: 8 2^-52 max|mu_C| / h, on top of the device's own TOL max(1, cond)."""
    lf, model, factor, points, binnings = end_to_end
    names = list(points)
    P = len(points['shift'])
    worst = 0.0
    for label, b in binnings.items():
        got_names, mu, J = lf.expected_coarse_jacobian_points(b, points, livetime_days=LIVETIME)
        assert got_names == names == lf._parameter_names()
        assert mu.shape == (P,) + b.shape and J.shape == (P, len(names)) + b.shape
        assert np.array_equal(bits(mu), bits(lf.expected_coarse_points(b, points, livetime_days=LIVETIME))), label
        one = lf.expected_coarse_jacobian(b, livetime_days=LIVETIME, **{k: v[1] for k, v in points.items()})
        assert one[0] == names and np.array_equal(bits(one[1]), bits(mu[1])) and np.array_equal(bits(one[2]), bits(J[1])), label
        h = {k: 1e-3 * (1.0 if k == 'shift' else points[k]) for k in names}
        stencil = {k: np.concatenate([np.concatenate([v + (h[f] if f == k else 0.0), v - (h[f] if f == k else 0.0)]) for f in names])
                   for k, v in points.items()}
        at = lf.expected_coarse_points(b, stencil, livetime_days=LIVETIME).reshape((len(names), 2, P) + b.shape)
        for p in range(P):
            cond = user_cond(model, b, factor, {k: v[p] for k, v in points.items()}).reshape((len(names),) + b.shape)
            for f, k in enumerate(names):
                step = np.broadcast_to(h[k], (P,))[p]
                x = stencil[k].reshape(len(names), 2, P)[f, :, p]
                diff = (at[f, 0, p] - at[f, 1, p]) / (x[0] - x[1])                    # (the step the two points really are apart)
                bound = 8 * 2.0 ** -52 * np.max(np.abs(at[f, :, p])) / step + TOL * np.maximum(1.0, cond[f])
                err = np.abs(J[p, f] - diff)
                assert np.all(err <= bound), '%s, point %d, %s: off by %.3g of the bound' % (label, p, k, float(np.max(err / bound)))
                worst = max(worst, float(np.max(err / bound)))
    print('central differences: the worst entry is at %.3g of its bound' % worst)
    dead = dict(points, shift=np.array([0.37, 1.5, 0.81]))                # outside the anchor box: nan throughout
    _, mu, J = lf.expected_coarse_jacobian_points(binnings['keep_x'], dead, livetime_days=LIVETIME)
    assert np.isnan(mu[1]).all() and np.isnan(J[1]).all() and np.all(np.isfinite(mu[[0, 2]])) and np.all(np.isfinite(J[[0, 2]]))


def test_band_from_the_covariance_of_hesse(end_to_end):
    """expected_coarse_band with hesse's covariance -- some parameters floating, one held -- is the numpy propagation of
    expected_coarse_jacobian's J; an unknown name is a ValueError, a nan covariance a nan band."""
    lf, _, _, _, binnings = end_to_end
    own_data = lf.ctx.download_counts(0).reshape(lf.bin_shape)
    fixed = dict(s2_rate_multiplier=1.0)
    try:
        truth = dict(shift=0.2, s0_rate_multiplier=1.1)
        lf.set_binned_data(np.random.default_rng(61).poisson(lf.expected_counts(livetime_days=LIVETIME, **truth)).astype(float))
        best, _ = lf.bestfit_device(livetime_days=LIVETIME, **fixed)
        names, cov = lf.hesse(best, livetime_days=LIVETIME, **fixed)
    finally:
        lf.set_binned_data(own_data)
    assert names == ['s0_rate_multiplier', 's1_rate_multiplier', 'shift'] and np.all(np.isfinite(cov))
    at = dict(best, **fixed)
    for label in ('keep_x', 'box', 'rebin3', 'identity'):
        b = binnings[label]
        mu, sigma, impacts = lf.expected_coarse_band(b, names, cov, livetime_days=LIVETIME, **at)
        all_names, mu2, J = lf.expected_coarse_jacobian(b, livetime_days=LIVETIME, **at)
        assert mu.shape == sigma.shape == b.shape and list(impacts) == names
        assert np.array_equal(bits(mu), bits(mu2)) and np.array_equal(bits(mu), bits(lf.expected_coarse(b, livetime_days=LIVETIME, **at)))
        Jk = J[[all_names.index(k) for k in names]]
        want = np.sqrt(np.einsum('k...,kl,l...->...', Jk, cov, Jk))
        assert np.all(sigma >= 0) and sigma.max() > 0 and np.all(np.abs(sigma - want) <= 1e-12 * want), label
        for i, k in enumerate(names):
            assert np.array_equal(impacts[k], Jk[i] * np.sqrt(cov[i, i])), (label, k)
        s2, i2 = coarse.propagate_covariance(all_names, J, names, cov)
        assert np.array_equal(bits(s2), bits(sigma)) and all(np.array_equal(i2[k], impacts[k]) for k in names)
    b = binnings['box']
    with pytest.raises(ValueError, match='bogus'):
        lf.expected_coarse_band(b, ['s0_rate_multiplier', 'bogus'], np.eye(2), livetime_days=LIVETIME, **at)
    mu, sigma, impacts = lf.expected_coarse_band(b, names, np.full((3, 3), np.nan), livetime_days=LIVETIME, **at)
    assert np.all(np.isfinite(mu)) and np.isnan(sigma).all() and all(np.isnan(v).all() for v in impacts.values())


def test_coarse_information_against_the_fisher_information(end_to_end):
    """With the identity binning the cells' information adds up to fisher_information(priors=False), to TOL max(1, cond) with
    the oracle's cond carried to the user's parameters; with any other binning I_fine - sum_C I_C has no eigenvalue below
    -TOL ||I_fine||: rebinning cannot add information."""
    lf, model, factor, _, binnings = end_to_end
    truth = dict(s0_rate_multiplier=1.1, s1_rate_multiplier=0.8, s2_rate_multiplier=1.3, shift=0.2)
    names, I_fine, unb_fine = lf.fisher_information(livetime_days=LIVETIME, priors=False, **truth)
    mult = np.array([truth['s%d_rate_multiplier' % s] for s in range(3)])
    cond_theta = fo.information(model, [truth['shift']], mult * factor)['cond']                       # [d + S, d + S]
    U = hessian.user_jacobian(1, 1, 3, mult[None, :], factor, np.ones((1, 3)), [-1, -1, -1], [0, 1, 2])[0]
    cond = np.abs(U) @ cond_theta @ np.abs(U).T
    norm = np.linalg.norm(I_fine, 2)
    for label, b in binnings.items():
        got_names, info, unbounded = lf.coarse_information(b, livetime_days=LIVETIME, **truth)
        assert got_names == names and info.shape == (4, 4) + b.shape and unbounded.shape == (4,) + b.shape and unbounded.dtype == bool
        total = info.reshape(4, 4, -1).sum(axis=2)
        if label == 'identity':
            assert np.array_equal(unbounded.reshape(4, -1).any(axis=1), unb_fine)
            err = np.abs(total - I_fine)
            assert np.all(err <= TOL * np.maximum(1.0, cond)), 'off by %.3g of TOL max(1, cond)' % float(np.max(err / np.maximum(1.0, cond)) / TOL)
            print('identity binning against fisher_information: the worst entry is at %.3g of TOL max(1, cond)'
                  % float(np.max(err / np.maximum(1.0, cond)) / TOL))
        lowest = np.linalg.eigvalsh(I_fine - total).min()
        assert lowest >= -TOL * norm, '%s: an eigenvalue of I_fine - sum_C I_C at %.3g ||I_fine||' % (label, lowest / norm)
        if label == 'all_summed':
            _, mu, J = lf.expected_coarse_jacobian(b, livetime_days=LIVETIME, **truth)
            assert info.shape == (4, 4) and np.array_equal(info, np.outer(J, J) / mu)
