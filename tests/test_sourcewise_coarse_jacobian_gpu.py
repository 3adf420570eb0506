"""Derivatives of the coarse views of a source-wise model on the device: bi_sourcewise_expected_coarse_jacobian against the per-bin
products of factored_curvature_oracle.curvature_columns(second=False) -- X = coef.v . rows in long double, cond = |coef.v| . |rows|,
both reduced with np.add.at over the cell map of the binning -- at the fine shapes of test_sourcewise_coarse_gpu.py (every path of
the kernel's geometry and of the finish kernels, every kind of coarsening) and the nine (source slots, own axes) classes, total and
per source; an axis nobody owns; a host sub-batch seam; the refusals of the C ABI; and the four `sourcewise_coarse_*` functions of
blueice_amd.coarse on a SourceWiseBinnedLogLikelihood end to end.

The bar is test_coarse_jacobian_gpu.check's, restated: |got - want| <= TOL max(1, cond) per entry, TOL = 1e-10
(tests/test_gof_gpu.py).  Derivatives along z are differences of rows that cancel inside a cell, so |want| alone is the wrong
scale for them.  The per-source form is held to the same products restricted to the rows of source s.  nan, status words, zeros
and "bitwise" are exact."""
from collections import OrderedDict

import numpy as np
import pytest

import batch_seam_cases as bsc
import factored_curvature_oracle as fco
import factored_oracle as fo
import sourcewise_toy_cases as cases
from test_gof_gpu import TOL
from test_sourcewise_coarse_gpu import CLASS_SHAPE, SHAPES, binnings_of, bits, cell_map, five_points, reduce_wide

pytestmark = pytest.mark.gpu


def check(got, want, cond, what):
    """test_coarse_jacobian_gpu.check: -> the largest |err| / (TOL max(1, cond))"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - want)
    bound = TOL * np.maximum(1.0, cond)
    assert np.all(err <= bound), '%s: off by %.3g of TOL max(1, cond)' % (what, float(np.max(err / bound)))
    return float(np.max(err / bound)) if err.size else 0.0


def fine_products(model, z, rs):
    """-> (X [1 + S, 1 + F, B] long double, cond [1 + S, 1 + F, B]): block 0 every row of the point, block 1 + s the rows of source
    s alone; row 0 of a block mu, rows 1 .. F the derivatives over theta = (z, then rate scales)"""
    S, B = len(model['own']), fo.n_bins(model)
    coef, rows = fco.curvature_columns(model, z, rs, second=False)
    v = np.asarray(coef.v, dtype=np.longdouble)                     # [1 + F, NR]
    t = fco._block(model, rows, 0, B).astype(np.longdouble)         # [NR, B]
    src = np.array([s for s, _ in rows])
    X, cond = [v @ t], [np.abs(v) @ np.abs(t)]
    for s in range(S):
        X.append(v[:, src == s] @ t[src == s])
        cond.append(np.abs(v[:, src == s]) @ np.abs(t[src == s]))
    return np.stack(X), np.stack(cond).astype(float)


def summed_over_sources(per):
    """[..., S, F, C] -> [..., F, C]: added over s in ascending order in long double from 0, rounded once (the header's wording)"""
    acc = np.zeros(per.shape[:-3] + per.shape[-2:], dtype=np.longdouble)
    for s in range(per.shape[-3]):
        acc = acc + per[..., s, :, :].astype(np.longdouble)
    return acc.astype(np.float64)


def structure_zero(model):
    """bool [S, F]: the entries of source s's block that the structure makes exactly 0.0 -- another source's scale, an axis s
    does not own"""
    d, S = len(model['anchor_z']), len(model['own'])
    zero = np.ones((S, d + S), dtype=bool)
    for s, own in enumerate(model['own']):
        zero[s, list(own)] = False
        zero[s, d + s] = False
    return zero


def check_point(model, z, rs, m, cells, mu, jac, mu_s, jac_s, what):
    """one live point's four arrays against the oracle -> the worst ratio"""
    X, cond = fine_products(model, z, rs)
    want = reduce_wide(m, cells, X)                                 # [1 + S, 1 + F, C]
    c = np.asarray(reduce_wide(m, cells, cond), dtype=float)
    return max(check(mu, want[0, 0], c[0, 0], what + ', mu'), check(jac, want[0, 1:], c[0, 1:], what + ', jac'),
               check(mu_s, want[1:, 0], c[1:, 0], what + ', mu per source'), check(jac_s, want[1:, 1:], c[1:, 1:], what + ', jac per source'))


def check_jacobian(name, model, shape, few):
    d, S, B = len(model['anchor_z']), len(model['own']), fo.n_bins(model)
    F = d + S
    assert B == int(np.prod(shape))
    z, rs, status = five_points(model, B + S)
    live = np.flatnonzero(status == 0)
    zero = structure_zero(model)
    unowned = [i for i in range(d) if not any(i in own for own in model['own'])]
    ctx = cases.upload(model)                                       # no counts: none are needed
    worst = 0.0
    try:
        for label, groups in binnings_of(shape, few).items():
            what = '%s, %s' % (name, label)
            m, cells = cell_map(shape, groups)
            assert ctx.set_coarse_binning(shape, groups) == cells, what
            total, st0 = ctx.expected_coarse(cells, z, rs)
            mu, jac, st = ctx.expected_coarse_jacobian(cells, z, rs)
            mu_s, jac_s, st_s = ctx.expected_coarse_jacobian(cells, z, rs, per_source=True)
            assert mu.shape == (5, cells) and jac.shape == (5, F, cells) and mu_s.shape == (5, S, cells) and jac_s.shape == (5, S, F, cells), what
            assert all(a.dtype == np.float64 for a in (mu, jac, mu_s, jac_s)) and st.dtype == np.int32 == st_s.dtype, what
            assert np.array_equal(st, st0) and np.array_equal(st_s, st0) and np.array_equal(st0, status), what
            for a in (mu, jac, mu_s, jac_s):
                assert np.isnan(a[3:]).all() and np.isfinite(a[live]).all(), what
            assert np.array_equal(bits(mu[live]), bits(total[live])), what + ': mu is not bi_sourcewise_expected_coarse bit for bit'
            assert np.array_equal(bits(summed_over_sources(jac_s[live])), bits(jac[live])), what + ': the per-source rows do not add up to the total rows bit for bit'
            assert np.all(jac_s[live][:, zero] == 0.0) and not np.signbit(jac_s[live][:, zero]).any(), what + ': structural zeros'
            assert np.all(jac[live][:, unowned] == 0.0), what + ': the row of an axis nobody owns'
            for p in live:
                worst = max(worst, check_point(model, z[p], rs[p], m, cells, mu[p], jac[p], mu_s[p], jac_s[p], what + ', point %d' % p))
            # the same calls again, and the second point alone: the same bits
            for per_source, first in ((False, (mu, jac)), (True, (mu_s, jac_s))):
                again = ctx.expected_coarse_jacobian(cells, z, rs, per_source=per_source)
                assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(bits(again[1]), bits(first[1])), what
                alone = ctx.expected_coarse_jacobian(cells, z[1:2], rs[1:2], per_source=per_source)
                assert np.array_equal(bits(alone[0][0]), bits(first[0][1])) and np.array_equal(bits(alone[1][0]), bits(first[1][1])), what
        assert ctx.set_coarse_binning() == 0
    finally:
        ctx.close()
    print('%s: the worst entry is at %.3g of TOL max(1, cond)' % (name, worst))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(n) for n in s))
def test_jacobian_against_the_oracle(shape):
    """Every binning of the shape at three truths (one on the upper edge of the box), a point outside the box and one with a
    negative rate scale, total and per source: shapes, dtypes, the status of bi_sourcewise_expected_coarse, nan throughout the dead
    points, the total mu with the bits of bi_sourcewise_expected_coarse, the per-source rows adding up to the total rows bit for
    bit, exact zeros where the structure says so, the oracle's cells, a repeated call bitwise equal and a point alone with the bits
    it has in the batch."""
    B = int(np.prod(shape))
    model = fo.random_model(np.random.default_rng(5100 + B), cases.N_ANCHOR, cases.OWN, B, zero_quarter=(1,))
    check_jacobian('x'.join(str(n) for n in shape), model, shape, few=False)


@pytest.mark.parametrize('name', cases.CLASS_CASES)
def test_jacobian_of_every_kernel_class(name):
    """The nine (source slots, own axes) classes at 13 x 79 bins: every instantiation of k_sourcewise_coarse_jac, at 128 lanes and
    two sub-rows (the passes through LDS: one for up to 16 slots, two for 17 and 25, three for the 33 of <8, 3>)"""
    model, _, _ = cases.make_case(name)
    check_jacobian(name, model, CLASS_SHAPE, few=True)


def test_an_axis_nobody_owns():
    """factored_curvature_oracle.unbounded_fixture's model (B = 63 as 9 x 7; nobody owns axis 2): row 2 is exactly 0.0 at every
    binning, in both forms, and the rest is held to the oracle."""
    model, z, rs, _ = fco.unbounded_fixture()
    shape = (9, 7)
    z, rs = z[None, :], rs[None, :]
    ctx = cases.upload(model)
    worst = 0.0
    try:
        for label, groups in binnings_of(shape).items():
            m, cells = cell_map(shape, groups)
            assert ctx.set_coarse_binning(shape, groups) == cells
            mu, jac, st = ctx.expected_coarse_jacobian(cells, z, rs)
            mu_s, jac_s, _ = ctx.expected_coarse_jacobian(cells, z, rs, per_source=True)
            assert not st.any() and np.isfinite(jac).all()
            assert np.all(jac[0, 2] == 0.0) and np.all(jac_s[0, :, 2] == 0.0), label
            assert np.any(jac[0, 0] != 0.0) and np.any(jac[0, 1] != 0.0), label
            worst = max(worst, check_point(model, z[0], rs[0], m, cells, mu[0], jac[0], mu_s[0], jac_s[0], label))
    finally:
        ctx.close()
    print('an axis nobody owns: the worst entry is at %.3g of TOL max(1, cond)' % worst)


def test_the_host_sub_batch_seam():
    """One axis of 63 bins in 9 cells, P = chunk + 8 points with two dead ones ahead of the seam: two pieces, and the probes on both
    sides of the seam are the oracle's and have the bits of the same points evaluated alone."""
    model = bsc.model_of('tile')
    S = len(model['own'])
    K = 1 + S + sum(len(o) for o in model['own'])
    dead = (bsc.OUTSIDE, bsc.UNPHYSICAL)
    cap = bsc.IN_FLIGHT // (K * 63)
    P = cap + 8
    n_live = P - len(dead)
    chunk = bsc.coarse_chunk_one_row(n_live, K, 63, 9)
    assert chunk == cap < n_live <= 2 * chunk
    rng = np.random.default_rng(bsc.SEED + 0x1AC)
    g = model['anchor_z']
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    z = lo + (hi - lo) * rng.uniform(0.03, 0.97, (P, len(g)))
    rs = rng.uniform(0.5, 1.6, (P, S))
    z[bsc.OUTSIDE, 0] = lo[0] - 1.0
    rs[bsc.UNPHYSICAL, 0] = -1.0
    status = np.zeros(P, dtype=np.int32)
    status[bsc.OUTSIDE], status[bsc.UNPHYSICAL] = bsc.ST_OUT_OF_BOUNDS, bsc.ST_UNPHYSICAL
    probes = bsc.probes_of(P, dead, [chunk])
    groups = [np.asarray(bsc.REBIN7, dtype=np.int32)]
    m, cells = cell_map((63,), groups)
    ctx = cases.upload(model)
    worst = 0.0
    try:
        assert ctx.set_coarse_binning((63,), groups) == cells == 9
        for per_source in (False, True):
            mu, jac, st = ctx.expected_coarse_jacobian(cells, z, rs, per_source=per_source)
            assert ctx.get_param('last_point_pieces') == 2
            assert np.array_equal(st, status)
            assert np.isnan(mu[list(dead)]).all() and np.isnan(jac[list(dead)]).all()
            assert np.isfinite(np.delete(mu, dead, axis=0)).all() and np.isfinite(np.delete(jac, dead, axis=0)).all()
            alone = ctx.expected_coarse_jacobian(cells, z[probes], rs[probes], per_source=per_source)
            assert ctx.get_param('last_point_pieces') == 1
            assert np.array_equal(bits(alone[0]), bits(mu[probes])) and np.array_equal(bits(alone[1]), bits(jac[probes]))
            for p in probes:
                X, cond = fine_products(model, z[p], rs[p])
                want, c = reduce_wide(m, cells, X), np.asarray(reduce_wide(m, cells, cond), dtype=float)
                if per_source:
                    worst = max(worst, check(mu[p], want[1:, 0], c[1:, 0], 'point %d, mu per source' % p),
                                check(jac[p], want[1:, 1:], c[1:, 1:], 'point %d, jac per source' % p))
                else:
                    worst = max(worst, check(mu[p], want[0, 0], c[0, 0], 'point %d, mu' % p), check(jac[p], want[0, 1:], c[0, 1:], 'point %d, jac' % p))
    finally:
        ctx.close()
    print('seam at live item %d of %d: the worst probe is at %.3g of TOL max(1, cond)' % (chunk, n_live, worst))


def test_abi_refusals():
    from blueice_amd._capi import ERR_INVALID, ERR_STATE, ptr
    OK = 0
    from blueice_amd.exceptions import NotPreparedException
    shape, groups = (9, 7), [[0, 4, 9], [0, 7]]
    rng = np.random.default_rng(78)
    model = fo.random_model(rng, cases.N_ANCHOR, cases.OWN, 63)
    d, S = len(model['anchor_z']), len(model['own'])
    z, rs = cases.box_points(model, rng, 2)
    ctx = cases.upload(model)
    dev = ctx._dev
    f = dev._lib.bi_sourcewise_expected_coarse_jacobian
    mu, jac = np.empty((2, 2)), np.empty((2, d + S, 2))
    try:
        # no binning yet
        assert f(dev._h, 2, ptr(z), ptr(rs), 0, ptr(mu), ptr(jac), None) == ERR_STATE
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse_jacobian(2, z, rs)
        # the grid model's binning on the same context does not stand in for the store's own
        dev.upload_model([], rng.uniform(0.5, 1.5, (1, 63)), np.array([30.0]))
        assert dev.set_coarse_binning(shape, groups) == 2
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse_jacobian(2, z, rs)
        assert ctx.set_coarse_binning(shape, groups) == 2
        assert dev.set_coarse_binning() == 0
        # bad pointers, P < 0, P = 0
        assert f(dev._h, 2, ptr(z), ptr(rs), 0, None, ptr(jac), None) == ERR_INVALID
        assert f(dev._h, 2, ptr(z), ptr(rs), 0, ptr(mu), None, None) == ERR_INVALID
        assert f(dev._h, 2, None, ptr(rs), 0, ptr(mu), ptr(jac), None) == ERR_INVALID
        assert f(dev._h, -1, ptr(z), ptr(rs), 0, ptr(mu), ptr(jac), None) == ERR_INVALID
        assert f(dev._h, 0, None, None, 0, None, None, None) == OK
        assert f(dev._h, 2, ptr(z), ptr(rs), 0, ptr(mu), ptr(jac), None) == OK          # status is nullable, rate_scale too
        first = mu.copy()
        assert np.isfinite(mu).all() and np.isfinite(jac).all()
        ones_mu, ones_jac = np.empty((2, 2)), np.empty((2, d + S, 2))
        assert f(dev._h, 2, ptr(z), None, 0, ptr(ones_mu), ptr(ones_jac), None) == OK
        got = ctx.expected_coarse_jacobian(2, z, np.ones((2, S)))
        assert np.array_equal(bits(got[0]), bits(ones_mu)) and np.array_equal(bits(got[1]), bits(ones_jac))
        # ... and released by a new model
        ctx.begin_model(model['anchor_z'], S, 63, model['own'])
        for s in range(S):
            rows = np.asarray(model['ps'][s]).reshape(-1, 63)
            for k in range(len(rows)):
                ctx.set_anchor(s, k, rows[k], float(np.asarray(model['mus'][s]).reshape(-1)[k]))
        ctx.end_model()
        assert f(dev._h, 2, ptr(z), ptr(rs), 0, ptr(mu), ptr(jac), None) == ERR_STATE
        with pytest.raises(NotPreparedException, match='no coarse binning'):
            ctx.expected_coarse_jacobian(2, z, rs)
        assert ctx.set_coarse_binning(shape, groups) == 2
        assert np.array_equal(bits(ctx.expected_coarse_jacobian(2, z, rs)[0]), bits(first))
    finally:
        ctx.close()


# ---- through the likelihood class -----------------------------------------------------------------------------------------

LIVETIME = 2.5                  # of a base live time of 1.0: the chain rule to the user's parameters is not the identity


@pytest.fixture(scope='module')
def nuisance_lf():
    """built as test_sourcewise_coarse_gpu.nuisance_lf"""
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device=0))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(5)
    lf.set_data(lf.base_model.simulate())
    return lf, names


def binnings_for(lf):
    from blueice_amd import coarse
    space = lf.base_model.config['analysis_space']
    first, last = str(space[0][0]), str(space[-1][0])
    return OrderedDict(identity=coarse.CoarseBinning(lf), keep_first=coarse.CoarseBinning(lf, keep=[first]),
                       rebin=coarse.CoarseBinning(lf, rebin={first: 2, last: 3}), all_summed=coarse.CoarseBinning(lf, keep=[]),
                       box=coarse.CoarseBinning(lf, keep=[last], ranges={first: (space[0][1][1], space[0][1][-2])}))


def interior_points(names, P, seed):
    """strictly inside cells of the anchors -2 .. 2: a fraction in [0.2, 0.8] of a cell, so a step of 1e-3 stays inside"""
    rng = np.random.default_rng(seed)
    pts = OrderedDict(('s%d_rate_multiplier' % s, rng.uniform(0.6, 1.5, P)) for s in range(4))
    pts.update((n, rng.integers(-2, 2, P) + rng.uniform(0.2, 0.8, P)) for n in names)
    return pts


def user_terms(lf, model, pts, P):
    """-> (U [P, F, d + S] of hessian.user_jacobian, z [P, d], scale [P, S]) at the points"""
    from blueice_amd.hessian import user_jacobian
    z, scale, _ = lf._batch_terms(pts, LIVETIME)
    mult, L, eff, eff_axis, rate_sources = lf._chain_rule_terms(pts, P, LIVETIME)
    return user_jacobian(P, z.shape[1], scale.shape[1], mult, L, eff, eff_axis, rate_sources), z, scale


def test_jacobian_points_against_central_differences(nuisance_lf):
    """sourcewise_coarse_jacobian_points against central differences of expected_coarse_points at points strictly inside cells,
    h = 1e-3 (shape parameters) or 1e-3 of the value (multipliers).  mu_C is of degree <= 2 in every parameter (M_s and tau_s are
    each multilinear), so a central difference is exact up to the rounding of its two values: 8 2^-52 max|mu_C| / h on top of
    the device's own TOL max(1, |U| cond)."""
    from blueice_amd import coarse
    from test_factored_gpu import model_of
    lf, shape_names = nuisance_lf
    model = model_of(lf)
    P = 3
    pts = interior_points(shape_names, P, 17)
    names = lf._parameter_names()
    assert sorted(names) == sorted(pts) and len(names) == 12
    U, z, scale = user_terms(lf, model, pts, P)
    assert not np.array_equal(np.abs(U[0]).sum(axis=1), np.ones(12))
    fine_cond = [fine_products(model, z[p], scale[p])[1][0, 1:] for p in range(P)]           # [d + S, B], theta = (z, rate scales)
    worst = 0.0
    for label, b in binnings_for(lf).items():
        m = b.bin_map().astype(np.int64)
        got_names, mu, J = coarse.sourcewise_coarse_jacobian_points(lf, b, pts, livetime_days=LIVETIME)
        assert got_names == names and mu.shape == (P,) + b.shape and J.shape == (P, 12) + b.shape, label
        assert np.array_equal(bits(mu), bits(coarse.expected_coarse_points(lf, b, pts, livetime_days=LIVETIME))), label
        one = coarse.sourcewise_coarse_jacobian(lf, b, livetime_days=LIVETIME, **{k: float(v[1]) for k, v in pts.items()})
        assert one[0] == names and np.array_equal(bits(one[1]), bits(mu[1])) and np.array_equal(bits(one[2]), bits(J[1])), label
        _, mu_s, J_s = coarse.sourcewise_coarse_jacobian_points(lf, b, pts, per_source=True, livetime_days=LIVETIME)
        assert mu_s.shape == (P, 4) + b.shape and J_s.shape == (P, 4, 12) + b.shape, label
        h = {k: 1e-3 * (pts[k] if k.endswith('_rate_multiplier') else 1.0) for k in names}
        stencil = {k: np.concatenate([np.concatenate([v + (h[f] if f == k else 0.0), v - (h[f] if f == k else 0.0)]) for f in names])
                   for k, v in pts.items()}
        at = coarse.expected_coarse_points(lf, b, stencil, livetime_days=LIVETIME).reshape((12, 2, P) + b.shape)
        at_s = coarse.expected_coarse_points(lf, b, stencil, per_source=True, livetime_days=LIVETIME).reshape((12, 2, P, 4) + b.shape)
        assert np.isfinite(at).all()
        for p in range(P):
            cond = (np.abs(U[p]) @ np.asarray(reduce_wide(m, b.n_cells, fine_cond[p]), dtype=float)).reshape((12,) + b.shape)
            for f, k in enumerate(names):
                step = np.broadcast_to(h[k], (P,))[p]
                x = stencil[k].reshape(12, 2, P)[f, :, p]
                for got, pair in ((J[p, f], at[f, :, p]), (J_s[p, :, f], at_s[f, :, p])):
                    diff = (pair[0] - pair[1]) / (x[0] - x[1])                        # (the step the two points really are apart)
                    bound = 8 * 2.0 ** -52 * np.max(np.abs(pair)) / step + TOL * np.maximum(1.0, cond[f])
                    err = np.abs(got - diff)
                    assert np.all(err <= bound), '%s, point %d, %s: off by %.3g of the bound' % (label, p, k, float(np.max(err / bound)))
                    worst = max(worst, float(np.max(err / bound)))
    print('central differences: the worst entry is at %.3g of its bound' % worst)
    dead = OrderedDict(pts)
    dead[shape_names[2]] = np.array([pts[shape_names[2]][0], 2.5, pts[shape_names[2]][2]])          # outside the anchor box: nan throughout
    b = binnings_for(lf)['keep_first']
    for per_source in (False, True):
        _, mu, J = coarse.sourcewise_coarse_jacobian_points(lf, b, dead, per_source=per_source, livetime_days=LIVETIME)
        assert np.isnan(mu[1]).all() and np.isnan(J[1]).all() and np.isfinite(mu[[0, 2]]).all() and np.isfinite(J[[0, 2]]).all()


def test_band_from_the_covariance_of_hesse(nuisance_lf):
    """sourcewise_coarse_band with inference.hesse's covariance -- some parameters floating, one held -- is the numpy propagation
    of sourcewise_coarse_jacobian's J; an unknown name is a ValueError, a nan covariance a nan band and a finite mu."""
    from blueice_amd import coarse, inference
    lf, shape_names = nuisance_lf
    fixed = dict(s3_rate_multiplier=1.0, livetime_days=LIVETIME)
    best, _ = inference.bestfit_device(lf, **fixed)
    names, cov = inference.hesse(lf, best, **fixed)
    assert len(names) == 11 and 's3_rate_multiplier' not in names and np.all(np.isfinite(cov))
    at = dict(best, s3_rate_multiplier=1.0)
    binnings = binnings_for(lf)
    for label in ('keep_first', 'box', 'rebin', 'identity'):
        b = binnings[label]
        mu, sigma, impacts = coarse.sourcewise_coarse_band(lf, b, names, cov, livetime_days=LIVETIME, **at)
        all_names, mu2, J = coarse.sourcewise_coarse_jacobian(lf, b, livetime_days=LIVETIME, **at)
        assert mu.shape == sigma.shape == b.shape and list(impacts) == names, label
        assert np.array_equal(bits(mu), bits(mu2)) and np.array_equal(bits(mu), bits(coarse.expected_coarse(lf, b, livetime_days=LIVETIME, **at)))
        Jk = J[[all_names.index(k) for k in names]]
        want = np.sqrt(np.einsum('k...,kl,l...->...', Jk, cov, Jk))
        assert np.all(sigma >= 0) and sigma.max() > 0 and np.all(np.abs(sigma - want) <= 1e-12 * want), label
        for i, k in enumerate(names):
            assert np.array_equal(bits(impacts[k]), bits(Jk[i] * np.sqrt(cov[i, i]))), (label, k)
    b = binnings['box']
    with pytest.raises(ValueError, match='bogus'):
        coarse.sourcewise_coarse_band(lf, b, ['s0_rate_multiplier', 'bogus'], np.eye(2), livetime_days=LIVETIME, **at)
    mu, sigma, impacts = coarse.sourcewise_coarse_band(lf, b, names, np.full((11, 11), np.nan), livetime_days=LIVETIME, **at)
    assert np.all(np.isfinite(mu)) and np.isnan(sigma).all() and all(np.isnan(v).all() for v in impacts.values())


def test_coarse_information_against_the_fisher_information(nuisance_lf):
    """With the identity binning the cells' information adds up to inference.fisher_information_points(priors=False) within
    TOL max(1, |U| cond |U|^T), cond from factored_curvature_oracle.information; for every other binning I_fine - sum_C I_C has no
    eigenvalue below -TOL ||I_fine||; with everything summed into one cell I = J J^T / mu bitwise."""
    from blueice_amd import coarse, inference
    from test_factored_gpu import model_of
    lf, shape_names = nuisance_lf
    model = model_of(lf)
    pts = interior_points(shape_names, 1, 23)
    truth = {k: float(v[0]) for k, v in pts.items()}
    names, I_fine, _ = inference.fisher_information_points(lf, pts, livetime_days=LIVETIME, priors=False)
    I_fine = I_fine[0]
    U, z, scale = user_terms(lf, model, pts, 1)
    cond = np.abs(U[0]) @ fco.information(model, z[0], scale[0])['cond'] @ np.abs(U[0]).T
    norm = np.linalg.norm(I_fine, 2)
    for label, b in binnings_for(lf).items():
        got_names, info, unbounded = coarse.sourcewise_coarse_information(lf, b, livetime_days=LIVETIME, **truth)
        assert got_names == names and info.shape == (12, 12) + b.shape and unbounded.shape == (12,) + b.shape and unbounded.dtype == bool
        total = info.reshape(12, 12, -1).sum(axis=2)
        if label == 'identity':
            err = np.abs(total - I_fine)
            ratio = float(np.max(err / np.maximum(1.0, cond)) / TOL)
            print('identity binning against fisher_information_points: the worst entry is at %.3g of TOL max(1, cond)' % ratio)
            assert np.all(err <= TOL * np.maximum(1.0, cond)), 'off by %.3g of TOL max(1, cond)' % ratio
        else:
            lowest = np.linalg.eigvalsh(I_fine - total).min()
            assert lowest >= -TOL * norm, '%s: an eigenvalue of I_fine - sum_C I_C at %.3g ||I_fine||' % (label, lowest / norm)
        if label == 'all_summed':
            _, mu, J = coarse.sourcewise_coarse_jacobian(lf, b, livetime_days=LIVETIME, **truth)
            assert info.shape == (12, 12) and np.array_equal(bits(info), bits(np.outer(J, J) / mu))


def test_pinned_refusals_stay(nuisance_lf):
    """The four grid-model functions still refuse a source-wise model, and the message names the new spelling."""
    from blueice_amd import coarse
    lf, shape_names = nuisance_lf
    b = binnings_for(lf)['rebin']
    at = {shape_names[0]: 0.1}
    for call, spelling in ((lambda: coarse.expected_coarse_jacobian_points(lf, b, {shape_names[0]: np.array([0.1])}), 'sourcewise_coarse_jacobian_points('),
                           (lambda: coarse.expected_coarse_jacobian(lf, b, **at), 'sourcewise_coarse_jacobian('),
                           (lambda: coarse.expected_coarse_band(lf, b, [shape_names[0]], np.eye(1), **at), 'sourcewise_coarse_band('),
                           (lambda: coarse.coarse_information(lf, b, **at), 'sourcewise_coarse_information(')):
        with pytest.raises(NotImplementedError, match='source-wise') as e:
            call()
        assert 'blueice_amd.coarse.' + spelling in str(e.value)
