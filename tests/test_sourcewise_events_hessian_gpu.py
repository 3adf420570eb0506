"""The analytic Hessian of unbinned source-wise likelihoods on the device: bi_eval_sourcewise_events_hess (kernel
k_sourcewise_events_curv over the event store) and SourceWiseUnbinnedLogLikelihood with analytic_hessian = True.

Every comparison of a finite number is derivative_oracle.check_entries with C_POISSON = 256 against
`derivatives(expand(model), unbinned=True, hessian=True)`, the same likelihood on the full tensor-product grid (an empty set,
which the expansion cannot hold, against sourcewise_events_curvature_oracle, which the host tests hold to that oracle); ll,
gradient and status against bi_eval_factored on the same store, H against its transpose, a point against itself in another
batch, -inf, nan and status words are compared exactly.  The one other bar is the scale-relative 1e-5 sqrt(|H_ii H_jj|) of
tests/test_sourcewise_events_gpu.py between the analytic route and differences of the analytic gradient (its derivation is
there).  Shapes are the event-store tests': every class on (2, 2, 2, 2) anchors at the set lengths 0, 1, 5, 512, 513, 1025,
sets of different lengths in one launch, one set longer than the blocks of an item, and the smallest batch that crosses the host's
sub-batch seam.  Every test here fails without the feature."""
import warnings

import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_events_curvature_oracle as co
import sourcewise_toy_cases as toy_cases
from derivative_oracle import C_POISSON, check_entries, derivatives
from test_sourcewise_events_gpu import CLASSES, LENGTHS, OUTLIER, event_model, twelve_nuisances, uploaded
from test_sourcewise_sampler_gpu import bits, class_case

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
IN_FLIGHT = 2 ** 23       # kFacPartialDoubles (bi_factored.h)


def expanded_oracle(model, outlier=OUTLIER):
    full = fo.expand(model)
    return lambda z, rs: derivatives(full, z, rs, unbinned=True, outlier=outlier, hessian=True)


def own_oracle(model, outlier=OUTLIER):
    return lambda z, rs: co.events_curvature(model, z, rs, outlier=outlier)


def copy_of(model):
    return {k: [np.array(p) for p in v] if k == 'ps' else v for k, v in model.items()}


def check_points(ctx, z, rs, oracles, what, dataset=None):
    """ll, gradient and status bit for bit eval_grad's; H exactly symmetric; every finite number against
    oracles[dataset[p]](z, rs) -> (the worst ratio, the call's results)"""
    ll, gz, gs, H, st = ctx.eval_events_hess(z, rs, dataset)
    ll1, gz1, gs1, st1 = ctx.eval_grad(z, rs, dataset)
    assert not st.any() and np.array_equal(st, st1)
    assert np.array_equal(bits(ll), bits(ll1)) and np.array_equal(bits(gz), bits(gz1)) and np.array_equal(bits(gs), bits(gs1))
    assert np.array_equal(bits(H), bits(np.swapaxes(H, 1, 2)))
    worst = 0.0
    for p in range(len(z)):
        want = oracles[0 if dataset is None else int(dataset[p])](z[p], rs[p])
        worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (what, p)))
        worst = max(worst, check_entries(np.concatenate([gz[p], gs[p]]), want['grad'], want['grad_cond'], what='%s grad[%d]' % (what, p)))
        w = check_entries(H[p], want['hess'], want['hess_cond'], what='%s hess[%d]' % (what, p))
        print('%s hess[%d]: worst |err| / (2^-52 cond) = %.3g' % (what, p, w))
        worst = max(worst, w)
    print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (what, worst, C_POISSON))
    return worst, (ll, gz, gs, H, st)


# ---- 1. every class at every set length --------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CLASSES)
def test_every_class_at_every_set_length(name):
    """the seven single-launch classes, <8, 2> in four panels (s8_e2) and <8, 3> in eight (e3x8, mixed_padded)"""
    own = class_case(name)[0]['own']
    worst = 0.0
    for N in LENGTHS:
        rng = np.random.default_rng(sum(name.encode()) + 31 * N)
        model = event_model(rng, (2, 2, 2, 2), own, N)
        z, rs = toy_cases.box_points(model, rng, 2)
        ctx = uploaded(model)
        try:
            if N == 0:
                # H is the second derivatives of -sum_s r_s: d_j M_s at (z_i, rs_s), rs_s d_jk M_s at (z_i, z_k), zero elsewhere
                w, (ll, gz, gs, H, st) = check_points(ctx, z, rs, [own_oracle(model)], '%s N=0' % name)
                d = len(model['anchor_z'])
                for p in range(2):
                    d2 = co.rate_curvature(model, z[p], rs[p])[2]
                    assert np.all(H[p][d:, d:] == 0.0) and np.all(np.diag(H[p]) == 0.0)
                    assert np.count_nonzero(H[p][np.triu_indices(d + len(own))]) == np.count_nonzero(d2.v)
            else:
                w, _ = check_points(ctx, z, rs, [expanded_oracle(model)], '%s N=%d' % (name, N))
            worst = max(worst, w)
            assert ctx.get_param('last_morph_nbx') == max(1, -(-N // 512))
        finally:
            ctx.close()
    print('%s: worst over the lengths %.3g of C = %d' % (name, worst, C_POISSON))


# ---- 2. the clamp and nan ----------------------------------------------------------------------------------------------------

def test_clamp_and_nan():
    rng = np.random.default_rng(34)
    own = ((0,), (1, 2), ())
    N = 63
    model = event_model(rng, (3, 2, 4), own, N, zero_quarter=())
    z, rs = toy_cases.box_points(model, rng, 3)
    z[0, 2] = 0.5 * (model['anchor_z'][2][2] + model['anchor_z'][2][3])     # a cell of axis 2 that has the corner below
    holed = copy_of(model)
    holed['ps'][1][1, 2, ::4] = np.nan                      # one corner of source 1 at a quarter of the events
    dead = copy_of(holed)
    for p in dead['ps']:
        p[..., 5] = 0.0                                     # event 5: every row is 0 (lam = 0: the clamp) ...
        p[..., 9] = 0.0
    dead['ps'][1][1, 2, 9] = np.nan                         # ... and event 9: zeros and a nan source
    base = uploaded(model)
    try:
        ll_base = base.eval_events_hess(z, rs)[0]
        ctx = uploaded(holed)
        _, (ll, _, _, H, _) = check_points(ctx, z, rs, [expanded_oracle(holed)], 'nan at a quarter of the events')
        touched = z[:, 2] >= holed['anchor_z'][2][1]
        assert touched[0] and np.isfinite(H).all()
        for p in range(3):
            assert (ll[p] != ll_base[p]) == bool(touched[p])
        ctx.close()
        # clamped events contribute log(outlier) to ll and nothing to any derivative
        ctx = uploaded(dead)
        _, (ll, gz, gs, H, _) = check_points(ctx, z, rs, [expanded_oracle(dead)], 'clamped events')
        without = {k: [np.delete(p, [5, 9], axis=-1) for p in v] if k == 'ps' else v for k, v in holed.items()}
        for p in range(3):
            want = co.events_curvature(without, z[p], rs[p])
            check_entries(ll[p] - 2 * np.log(OUTLIER), want['ll'], want['ll_cond'] + 2 * abs(np.log(OUTLIER)), what='clamp ll[%d]' % p)
            check_entries(H[p], want['hess'], want['hess_cond'], what='clamp hess[%d]' % p)
        ctx.close()
        # ... and with outlier = 0: -inf, a nan gradient and a nan Hessian
        ctx = uploaded(dead, outlier=0.0)
        ll, gz, gs, H, st = ctx.eval_events_hess(z, rs)
        assert not st.any() and np.all(ll == -np.inf) and np.isnan(gz).all() and np.isnan(gs).all() and np.isnan(H).all()
        ctx.close()
    finally:
        base.close()


# ---- 3. several sets in one launch -------------------------------------------------------------------------------------------

def test_several_sets_in_one_launch():
    """N_t = (513, 0, 5, 1025) of a <8, 2> model (four panels): two, one, one and three tiles.  A point has the bits it has alone
    whatever is evaluated beside it; a bad dataset index and a point outside the box answer with their status, -inf and nan"""
    n = [513, 0, 5, 1025]
    own = class_case('s8_e2')[0]['own']
    rng = np.random.default_rng(45)
    model = event_model(rng, (2, 2, 2, 2), own, sum(n))
    off = np.concatenate([[0], np.cumsum(n)])
    per_set = [{k: [p[..., off[t]:off[t + 1]] for p in v] if k == 'ps' else v for k, v in model.items()} for t in range(4)]
    ctx = uploaded(model, n)
    try:
        P = 24
        z, rs = toy_cases.box_points(model, rng, P)
        ds = rng.integers(0, 4, P)
        ds[:8] = [0, 1, 2, 3, 3, 2, 1, 0]
        oracles = [own_oracle(m) if n[t] == 0 else expanded_oracle(m) for t, m in enumerate(per_set)]
        _, (ll, gz, gs, H, st) = check_points(ctx, z[:8], rs[:8], oracles, 'mixed sets', dataset=ds[:8])
        full = ctx.eval_events_hess(z, rs, ds)
        assert not full[4].any() and ctx.get_param('last_morph_nbx') == 3
        for a, b in zip(full[:4], (ll, gz, gs, H)):
            assert np.array_equal(bits(a[:8]), bits(b))
        again = ctx.eval_events_hess(z, rs, ds)
        for a, b in zip(again, full):
            assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
        for p in range(P):
            alone = ctx.eval_events_hess(z[p], rs[p:p + 1], ds[p:p + 1])
            for a, b in zip(alone[:4], full[:4]):
                assert np.array_equal(bits(a[0]), bits(b[p])), p
        # a set in a context of its own: the same bits (nothing of the other sets enters)
        solo = uploaded(per_set[3])
        pick = np.flatnonzero(ds == 3)
        assert np.array_equal(bits(solo.eval_events_hess(z[pick], rs[pick])[3]), bits(full[3][pick]))
        solo.close()
        ds_bad, z_bad, rs_bad = ds.copy(), z.copy(), rs.copy()
        ds_bad[3], ds_bad[5] = 4, -1
        z_bad[7, 1] = model['anchor_z'][1][-1] + 1.0
        rs_bad[9, 2] = -1.0
        ll_b, gz_b, gs_b, H_b, st_b = ctx.eval_events_hess(z_bad, rs_bad, ds_bad)
        assert st_b[3] == st_b[5] == ST_BAD_DATASET and st_b[7] == ST_OUT_OF_BOUNDS and st_b[9] == ST_UNPHYSICAL
        assert st_b.sum() == 2 * ST_BAD_DATASET + ST_OUT_OF_BOUNDS + ST_UNPHYSICAL
        gone = [3, 5, 7, 9]
        assert np.all(ll_b[gone] == -np.inf) and np.isnan(gz_b[gone]).all() and np.isnan(gs_b[gone]).all() and np.isnan(H_b[gone]).all()
        keep = np.delete(np.arange(P), gone)
        assert np.array_equal(bits(ll_b[keep]), bits(full[0][keep])) and np.array_equal(bits(H_b[keep]), bits(full[3][keep]))
    finally:
        ctx.close()


# ---- 4. a set longer than an item's blocks -----------------------------------------------------------------------------------

def test_a_set_longer_than_the_blocks_of_an_item():
    """1026 tiles of events on the 1024 blocks of an item: blocks 0 and 1 walk a second tile, k_finish adds 1024 partials"""
    N = 1026 * 512 - 100
    rng = np.random.default_rng(1027)
    model = event_model(rng, (2, 2), [(0,), (1,)], N, zero_quarter=())
    z, rs = toy_cases.box_points(model, rng, 2)
    ctx = uploaded(model)
    try:
        _, (ll, gz, gs, H, st) = check_points(ctx, z[:1], rs[:1], [expanded_oracle(model)], '1026 tiles')
        assert ctx.get_param('last_morph_nbx') == 1024
        both = ctx.eval_events_hess(z, rs)
        assert np.array_equal(bits(both[3][0]), bits(H[0])) and bits(both[0])[0] == bits(ll)[0]
    finally:
        ctx.close()


# ---- 5. an axis nobody owns, and the host's sub-batch seam -------------------------------------------------------------------

def test_an_axis_nobody_owns_has_zero_rows_and_columns():
    own = class_case('s2_e1')[0]['own']                     # [(1,), ()] on four axes: nobody owns axes 0, 2 and 3
    rng = np.random.default_rng(51)
    model = event_model(rng, (2, 2, 2, 2), own, 5, zero_quarter=())
    z, rs = toy_cases.box_points(model, rng, 2)
    ctx = uploaded(model)
    try:
        _, (_, _, _, H, _) = check_points(ctx, z, rs, [expanded_oracle(model)], 'unowned axes')
        for i in (0, 2, 3):
            assert np.all(H[:, i, :] == 0.0) and np.all(H[:, :, i] == 0.0)
        assert np.all(H[:, 1, 1] != 0.0) and np.all(H[:, 4, 4] != 0.0)
    finally:
        ctx.close()


def test_the_host_seam():
    """One event (one tile, one block per item) of a <4, 3> model, the single-launch class with the most result slots
    (29 linear + 136 pairs): FacBatch::run_lists cuts the items into sub-batches of kFacPartialDoubles / 165, and one item more
    than that crosses the seam.  The items on either side of it have the bits they have alone, and the oracle's numbers"""
    own = class_case('mixed')[0]['own']
    nsl = 1 + 4 * 4 + 4 * 3 + 16 * 17 // 2
    assert nsl == 165
    per_call = IN_FLIGHT // nsl
    P = per_call + 4                                        # two rejected points, per_call items, and two items behind the seam
    rng = np.random.default_rng(52)
    model = event_model(rng, (2, 2, 2, 2), own, 1)
    z, rs = toy_cases.box_points(model, rng, P)
    z[4], rs[6, 0] = model['anchor_z'][0][0] - 1.0, -1.0     # two rejected points in front: live numbers are not point numbers
    ctx = uploaded(model)
    try:
        ll, gz, gs, H, st = ctx.eval_events_hess(z, rs)
        assert ctx.get_param('last_point_pieces') == 2 and ctx.get_param('last_morph_nbx') == 1
        assert st[4] == ST_OUT_OF_BOUNDS and st[6] == ST_UNPHYSICAL and st.sum() == ST_OUT_OF_BOUNDS + ST_UNPHYSICAL
        # live item per_call is point per_call + 2: the first of the second piece; the rejected points move the seam by two
        seam = per_call + 2
        probes = np.array([0, 5, 7, seam - 2, seam - 1, seam, P - 1])
        assert P - 1 == seam + 1
        alone = ctx.eval_events_hess(z[probes], rs[probes])
        assert ctx.get_param('last_point_pieces') == 1 and not alone[4].any()
        for a, b in zip(alone[:4], (ll, gz, gs, H)):
            assert np.array_equal(bits(a), bits(b[probes]))
        g1 = ctx.eval_grad(z[probes], rs[probes])
        assert np.array_equal(bits(g1[0]), bits(ll[probes])) and np.array_equal(bits(g1[1]), bits(gz[probes]))
        oracle = expanded_oracle(model)
        for p in (seam - 1, seam, P - 1):
            want = oracle(z[p], rs[p])
            check_entries(ll[p], want['ll'], want['ll_cond'], what='seam ll[%d]' % p)
            check_entries(H[p], want['hess'], want['hess_cond'], what='seam hess[%d]' % p)
        live = np.delete(np.arange(P), [4, 6])
        assert np.isfinite(H[live]).all() and np.isnan(H[[4, 6]]).all()
    finally:
        ctx.close()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------

def test_state():
    from blueice_amd.exceptions import NotPreparedException
    model, counts = class_case('mixed')
    B = fo.n_bins(model)
    rng = np.random.default_rng(9)
    z, rs = toy_cases.box_points(model, rng, 3)
    ds = np.array([0, 1, 2])
    ctx = toy_cases.upload(model, counts)
    try:
        before = ctx.eval_hess(z, rs, ds)
        # no store: the new call refuses and says so, though counts are there
        with pytest.raises(NotPreparedException, match='bi_eval_sourcewise_events_hess.*no event store'):
            ctx.eval_events_hess(z, rs, ds)
        edges = [np.arange(B + 1, dtype=float)]
        coords = [[rng.integers(0, B, 40) + 0.5], [rng.integers(0, B, 7) + 0.5]]
        ctx.score_events('piecewise', edges, coords, OUTLIER)
        # with a store: the binned Hessian still refuses, the new call answers; dataset 2 is not one of the two event sets
        with pytest.raises(NotPreparedException, match='event store') as info:
            ctx.eval_hess(z, rs)
        assert 'bi_eval_sourcewise_hess' in str(info.value)
        ll, gz, gs, H, st = ctx.eval_events_hess(z, rs, ds)
        assert st.tolist() == [0, 0, ST_BAD_DATASET] and np.isfinite(H[:2]).all() and np.isnan(H[2]).all() and ll[2] == -np.inf
        g = ctx.eval_grad(z, rs, ds)
        assert np.array_equal(bits(g[0]), bits(ll)) and np.array_equal(bits(g[1]), bits(gz)) and np.array_equal(bits(g[2]), bits(gs))
        # a store that is still being filled refuses
        from blueice_amd._capi import ptr
        dev = ctx._dev
        n_ev = np.array([3], dtype=np.int64)
        dev._check(dev._lib.bi_sourcewise_events_begin(dev._h, 1, ptr(n_ev), OUTLIER))
        with pytest.raises(NotPreparedException, match='bi_sourcewise_events_end'):
            ctx.eval_events_hess(z, rs)
        # dropped: the binned Hessian has its old bits, and the new call refuses again
        ctx.drop_events()
        after = ctx.eval_hess(z, rs, ds)
        for a, b in zip(after, before):
            assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
        with pytest.raises(NotPreparedException, match='no event store'):
            ctx.eval_events_hess(z, rs, ds)
    finally:
        ctx.close()


# ---- 7. through the likelihood -----------------------------------------------------------------------------------------------

def test_through_the_likelihood():
    """d = 12 nuisances with Gaussian constraints, six sources of one or two own parameters (class <8, 2>: four panels), F = 18"""
    from blueice_amd import LogLikelihoodSum, inference
    lf, names = twelve_nuisances(analytic_hessian=True)
    try:
        assert not lf.supports_hessian                      # no data yet
        np.random.seed(12)
        lf.set_data(lf.base_model.simulate()[:300])
        assert lf.supports_hessian and lf.hessian_method == 'analytic' and LogLikelihoodSum([lf, lf]).hessian_method == 'analytic'
        rng = np.random.default_rng(10)
        P = 3
        pts = {n: rng.uniform(-1.9, 1.9, P) for n in names}
        pts.update({'s%d_rate_multiplier' % s: rng.uniform(0.6, 1.5, P) for s in range(6)})
        ll, grads, order, H = lf.values_gradients_hessians(pts)
        assert lf.hessian_method == 'analytic' and H.shape == (P, 18, 18) and np.isfinite(H).all()
        assert order == ['s%d_rate_multiplier' % s for s in range(6)] + names
        ll1, grads1 = lf.values_and_gradients(pts)
        assert np.all(np.abs(ll - ll1) <= 1e-12 * np.abs(ll1))
        for n in order:
            assert np.all(np.abs(grads[n] - grads1[n]) <= 1e-9 * np.maximum(1.0, np.abs(grads1[n])))
        assert np.array_equal(bits(H), bits(np.swapaxes(H, 1, 2)))
        one = lf.value_gradient_hessian(**{k: float(v[1]) for k, v in pts.items()})
        assert one[0] == ll[1] and np.array_equal(bits(one[3]), bits(H[1]))
        # the Gaussian constraints' curvature -1 / sigma^2 = -1 on every nuisance's diagonal entry, and nothing else: against the
        # device Hessian over (z, rate_scale), which knows no priors.  Shape parameters are z; a rate multiplier m_s enters as
        # rate_scale_s = J_s m_s (J_s: live time and efficiency, constants here), so H_user = J H_theta J with J = 1 on z
        zb, sb, _ = lf._batch_terms(pts, None)
        Hth = lf.ctx.eval_events_hess(zb, sb)[3]
        J = np.concatenate([sb / np.stack([pts['s%d_rate_multiplier' % s] for s in range(6)], axis=1), np.ones((P, 12))], axis=1)
        perm = list(range(12, 18)) + list(range(12))
        want = Hth[:, perm][:, :, perm] * J[:, :, None] * J[:, None, :]
        want[:, np.arange(6, 18), np.arange(6, 18)] -= 1.0
        err = np.abs(H - want) / np.sqrt(np.abs(np.einsum('pi,pj->pij', np.diagonal(H, axis1=1, axis2=2), np.diagonal(H, axis1=1, axis2=2))))
        print('GaussianPrior curvature: worst |H - (H_theta - 1 on the nuisances)| / sqrt(|H_ii H_jj|) = %.3g' % err.max())
        assert err.max() <= 64 * 2.0 ** -52                 # (a few roundings per entry: the products with J, the sum with the prior)
        # the gradient-difference route of the same object: the bar of tests/test_sourcewise_events_gpu.py
        lf.config['analytic_hessian'] = False
        assert not lf.supports_hessian
        ll_d, _, order_d, H_d = lf.values_gradients_hessians(pts)
        assert lf.hessian_method == 'gradient-differences' and order_d == order and np.array_equal(bits(ll_d), bits(ll))
        lf.config['analytic_hessian'] = True
        worst = 0.0
        for p in range(P):
            sc = np.sqrt(np.abs(np.outer(np.diag(H[p]), np.diag(H[p]))))
            worst = max(worst, float(np.max(np.abs(H_d[p] - H[p]) / sc)))
        print('analytic against gradient differences: worst |difference| / sqrt(|H_ii H_jj|) = %.3g' % worst)
        assert worst <= 1e-5
        # errors of all eighteen parameters from the fit
        best, ll_best = lf.bestfit_minuit()
        assert lf.hessian_method == 'analytic' and np.isfinite(ll_best)
        errors = np.array([best[n + '_error'] for n in order])
        print('bestfit_minuit errors: %s' % np.array2string(errors, precision=4))
        assert np.all(np.isfinite(errors)) and np.all(errors > 0)
        # an ensemble: three sets (one empty), fitted at once; their Hessians and covariances in one call and set by set.  (-H need
        # not be positive definite -- the empty set's rate block is 0 -- and hesse answers nan there, in either form of the call)
        np.random.seed(13)
        sets = [lf.base_model.simulate()[:k] for k in (250, 0, 300)]
        lf.set_datasets(sets)
        fitted, lls = inference.bestfit_toys(lf)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            names_c, cov = inference.hesse(lf, fitted, datasets=np.arange(3))
            assert lf.hessian_method == 'analytic' and cov.shape == (3, 18, 18) and names_c == order
            _, _, _, H3 = lf.values_gradients_hessians(fitted, dataset=np.arange(3))
            assert np.isfinite(H3).all()
            for t in range(3):
                at = {k: np.asarray(v)[t:t + 1] for k, v in fitted.items()}
                _, _, _, Ht = lf.values_gradients_hessians(at, dataset=np.array([t]))
                assert np.array_equal(bits(Ht[0]), bits(H3[t]))
                names_t, cov_t = inference.hesse(lf, at, datasets=np.array([t]))
                assert names_t == names_c and (np.isfinite(cov[t]).all() or np.isnan(cov[t]).all())
                np.testing.assert_array_equal(cov_t[0], cov[t])
        print('hesse over three sets: covariance finite at %s' % [bool(np.isfinite(c).all()) for c in cov])
        for name in ('fisher_information', 'expected_errors'):
            with pytest.raises(NotImplementedError, match='unbinned source-wise'):
                getattr(lf, name)()
    finally:
        lf.ctx.close()
