"""Every derivative route of the device against the exact derivative oracle (tests/derivative_oracle.py) with the per-entry
bound |device - oracle| <= C 2^-52 cond: bi_eval_hess (k_morph_hess) at every (G, DM) variant and tiling that changes its
code path, bi_eval_grad one work item per point (every column class), planned on the device (k_grad_fill), on the matrix
cores (k_grad_mfma, every KG with and without padding), with Beeston-Barlow (k_morph_bbgrad, every (G, DZ)) and unbinned.
Points: random interior ones, exact anchors and the top corner, single-anchor axes, and one near the best fit, where the
gradient is mostly cancellation.  Run with -s for the worst |err| / (2^-52 cond) per case."""
import numpy as np
import pytest

import derivative_oracle as do

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    print('\nworst |err| / (2^-52 cond) per case (C = %d):' % do.C_POISSON)
    for k in sorted(WORST):
        print('  %-40s %.3g' % (k, WORST[k]))


def note(tag, worst):
    WORST[tag] = max(WORST.get(tag, 0.0), worst)


def ctx_of(m, counts=None, sparse=0, model=None, **params):
    """A DeviceContext holding SyntheticModel m (or the dense `model` dict, for edited tensors) and `counts` [T, B]."""
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', sparse)
    for k, v in params.items():
        ctx.set_param(k, v)
    if model is None:
        m.upload(ctx)
    else:
        ctx.upload_model(model['anchor_z'], model['ps'], model['mus'], n_model=model.get('n_model'), bb_source=m.bb_source)
    if counts is not None:
        ctx.upload_counts(counts)
    return ctx


def synth(S, n_anchor, bins, bb_source=-1, seed=1234):
    from blueice_amd.synthetic import SyntheticModel
    return SyntheticModel(S, n_anchor, bins, seed=seed, bb_source=bb_source)


def oracle_model(m, z, model=None):
    return model if model is not None else (m.dense_model() if m.A * m.S * m.B <= 2_000_000 else m.cell_model(z))


def newton_point(m, counts, model=None, steps=12):
    """A point near the best fit (Newton on the oracle from the central anchor, kept inside the central cell)."""
    z = np.array([g[len(g) // 2] for g in m.anchor_z], dtype=float)
    if m.d:
        z = np.array([min(g[len(g) // 2] + 0.1 * (g[1] - g[0]) if len(g) > 1 else g[0], g[-1]) for g in m.anchor_z])
    r = np.ones(m.S)
    lo = np.array([g[min(len(g) // 2, len(g) - 2)] if len(g) > 1 else g[0] for g in m.anchor_z] + [0.05] * m.S)
    hi = np.array([g[min(len(g) // 2, len(g) - 2) + 1] if len(g) > 1 else g[0] for g in m.anchor_z] + [5.0] * m.S)
    th = np.concatenate([z, r])
    for _ in range(steps):
        o = do.derivatives(oracle_model(m, th[:m.d], model), th[:m.d], th[m.d:], counts=counts)
        F = len(th)
        free = np.array([hi[j] > lo[j] for j in range(F)])
        H = o['hess'][np.ix_(free, free)]
        step = np.zeros(F)
        try:
            step[free] = np.linalg.solve(H, -o['grad'][free])
        except np.linalg.LinAlgError:
            break
        th = np.clip(th + step, lo + 1e-3 * (hi - lo), hi - 1e-3 * (hi - lo))
    return th[:m.d], th[m.d:]


def standard_points(m, n_random, seed, counts=None, model=None, best_fit=True):
    """Random interior points, an interior anchor on every axis that has one, the top corner, and (binned) one near the best
    fit.  -> (z [P, d], r [P, S])."""
    zs, rs = m.random_points(n_random, seed=seed)
    rng = np.random.default_rng(seed)
    extra_z = [[g[len(g) // 2] if len(g) > 2 else g[0] for g in m.anchor_z], [g[-1] for g in m.anchor_z]]
    extra_r = [rng.uniform(0.6, 1.4, m.S) for _ in extra_z]
    if best_fit and counts is not None:
        z, r = newton_point(m, counts, model)
        extra_z.append(list(z))
        extra_r.append(r)
    zs = np.concatenate([zs, np.array(extra_z, dtype=float).reshape(len(extra_z), m.d)])
    rs = np.concatenate([rs, np.array(extra_r)])
    return zs, rs


def check_hess(tag, ctx, m, counts, zs, rs, ds=None, model=None, unbinned=False, outlier=1e-12):
    """bi_eval_hess against the oracle per entry, against bi_eval (status, value) and bi_eval_grad (value, gradient), and
    exactly symmetric."""
    z_arg = zs if m.d else None
    ll, gz, gs, H, st = ctx.eval_hess(z_arg, rs, ds)
    ll_g, gz_g, gs_g, st_g = ctx.eval_grad(z_arg, rs, ds)
    ll_e, st_e = ctx.eval(z_arg, rs, ds) if not unbinned else (ll_g, st_g)
    assert np.array_equal(st, st_e) and np.array_equal(st, st_g)
    assert np.array_equal(H, np.swapaxes(H, 1, 2), equal_nan=True)
    g, g_g = np.concatenate([gz, gs], 1), np.concatenate([gz_g, gs_g], 1)
    worst = 0.0
    for p in range(len(rs)):
        assert st[p] == 0 and np.isfinite(ll[p])
        cnt = None if unbinned else (counts if counts.ndim == 1 else counts[0 if ds is None else ds[p]])
        o = do.derivatives(oracle_model(m, zs[p], model), zs[p], rs[p], counts=cnt, unbinned=unbinned, outlier=outlier)
        worst = max(worst, do.check_entries(ll[p], o['ll'], o['ll_cond'], what='%s ll p%d' % (tag, p)),
                    do.check_entries(g[p], o['grad'], o['grad_cond'], what='%s grad p%d' % (tag, p)),
                    do.check_entries(H[p], o['hess'], o['hess_cond'], what='%s hess p%d' % (tag, p)))
        # the same numbers through the other entry points (both within the bound of the exact value: within twice of each other)
        do.check_entries(ll[p], ll_e[p], o['ll_cond'], 2 * do.C_POISSON, '%s ll vs bi_eval' % tag)
        do.check_entries(ll[p], ll_g[p], o['ll_cond'], 2 * do.C_POISSON, '%s ll vs bi_eval_grad' % tag)
        do.check_entries(g[p], g_g[p], o['grad_cond'], 2 * do.C_POISSON, '%s grad vs bi_eval_grad' % tag)
    note(tag, worst)


def check_grad(tag, ctx, m, counts, zs, rs, ds=None, model=None, unbinned=False, outlier=1e-12, sample=None):
    z_arg = zs if m.d else None
    ll, gz, gs, st = ctx.eval_grad(z_arg, rs, ds)
    if not unbinned:
        # (Beeston-Barlow: bi_eval flags the reference's first-root assertion, a coin flip where U_b == 0; the gradient
        # differentiates the special case there)
        ll_e, st_e = ctx.eval(z_arg, rs, ds)
        mask = ~4 if m.bb_source >= 0 else ~0
        assert np.array_equal(st & mask, st_e & mask)
    g = np.concatenate([gz, gs], 1)
    worst = 0.0
    for p in (range(len(rs)) if sample is None else sample):
        assert st[p] & (~4 if m.bb_source >= 0 else ~0) == 0 and np.isfinite(ll[p])
        cnt = None if unbinned else (counts if counts.ndim == 1 else counts[0 if ds is None else ds[p]])
        mod = oracle_model(m, zs[p], model)
        if m.bb_source >= 0:
            o = do.bb_gradient(mod, zs[p], rs[p], cnt, m.bb_source)
        else:
            o = do.derivatives(mod, zs[p], rs[p], counts=cnt, unbinned=unbinned, outlier=outlier, hessian=False)
        worst = max(worst, do.check_entries(ll[p], o['ll'], o['ll_cond'], what='%s ll p%d' % (tag, p)),
                    do.check_entries(g[p], o['grad'], o['grad_cond'], what='%s grad p%d' % (tag, p)))
        if not unbinned and st_e[p] == 0:
            do.check_entries(ll[p], ll_e[p], o['ll_cond'], 2 * do.C_POISSON, '%s ll vs bi_eval' % tag)
    note(tag, worst)
    return st


# ---- k_morph_hess: every (G, DM) variant -----------------------------------------------------------------------------

def hess_variant(de, S):
    """(G, DM) the library picks for de effective shape axes and S sources, or None where it refuses (bi_hess.h)."""
    D = de + S
    Gc = 1 + D + de * (de + 1) // 2 + de * S
    G = 8 if Gc <= 8 else 16 if Gc <= 16 else 32 if Gc <= 32 else 64
    DM = 4 if D <= 4 else 8 if D <= 8 else 16
    if G >= 32 and DM < 8:
        DM = 8
    if Gc > 64 or D > 16 or (G, DM) == (64, 16):
        return None
    return G, DM


HESS_VARIANTS = [                 # (G, DM): S, anchors per axis (1 = a single-anchor axis)
    ((8, 4), 2, (3,)),
    ((8, 8), 5, (1,)),
    ((16, 4), 3, (3,)),
    ((16, 8), 3, (3, 2)),
    ((16, 16), 9, ()),
    ((32, 8), 2, (2, 3, 2)),
    ((32, 16), 7, (3, 2)),
    ((64, 8), 4, (2, 2, 3, 2)),
]


@pytest.mark.parametrize('variant,S,n_anchor', HESS_VARIANTS, ids=['G%d_DM%d' % v[0] for v in HESS_VARIANTS])
def test_hessian_variants_match_the_oracle(variant, S, n_anchor):
    de = sum(1 for n in n_anchor if n > 1)
    assert hess_variant(de, S) == variant
    m = synth(S, n_anchor, (700,))
    counts = m.counts(dense=True)
    ctx = ctx_of(m, counts)
    try:
        zs, rs = standard_points(m, 3, seed=S, counts=counts)
        check_hess('hess G%d DM%d' % variant, ctx, m, counts, zs, rs)
    finally:
        ctx.close()


def test_hessian_refuses_64_16_and_the_likelihood_falls_back():
    from blueice_amd.likelihood import DeviceLogLikelihood
    assert hess_variant(4, 6) is None
    m = synth(6, (2, 2, 2, 2), (40,))
    ctx = ctx_of(m, m.counts(dense=True))
    try:
        z, r = m.random_points(2, seed=1)
        with pytest.raises(ValueError, match='no kernel variant'):
            ctx.eval_hess(z, r)
        class Holder:                  # the likelihood class's route decision, on this context
            supports_hessian = DeviceLogLikelihood.supports_hessian
            hessian_method = DeviceLogLikelihood.hessian_method
            is_data_set = True

            def _bb_source_index(self):
                return -1
        lf = Holder()
        lf.ctx = ctx
        assert lf.supports_hessian is False and lf.hessian_method == 'gradient-differences'
    finally:
        ctx.close()


# ---- k_morph_hess: tiling, loads, forms --------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [511, 512, 513, 'mini3'])
def test_hessian_tile_edges(B):
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel.named('mini3') if B == 'mini3' else synth(2, (3,), (B,))
    counts = m.counts(dense=True)
    ctx = ctx_of(m, counts)
    try:
        zs, rs = standard_points(m, 2, seed=3, counts=counts)
        check_hess('hess tiles B=%s' % B, ctx, m, counts, zs, rs)
        zs, rs = zs[:1], rs[:1]                              # one point: nbx = all the slots' blocks
        check_hess('hess tiles B=%s' % B, ctx, m, counts, zs, rs)
    finally:
        ctx.close()


@pytest.mark.parametrize('B,chunks', [(270_000, 8), (100_000, 3)])
def test_hessian_tile_chunked_walk(B, chunks):
    """tile_chunks regions (8 from 512 tiles on; 3 over 196 tiles: uneven regions), two points per launch (nbx > 1)."""
    m = synth(2, (2,), (B,))
    counts = m.counts(dense=True)
    ctx = ctx_of(m, counts, tile_chunks=chunks)
    try:
        assert B // 512 >= 64 * chunks
        zs, rs = m.random_points(1, seed=2)
        zs = np.concatenate([zs, [[m.anchor_z[0][-1]]]])
        rs = np.concatenate([rs, [[0.9, 1.2]]])
        check_hess('hess tile_chunks=%d B=%d' % (chunks, B), ctx, m, counts, zs, rs)
    finally:
        ctx.close()


@pytest.mark.parametrize('nt', [0, 1])
@pytest.mark.parametrize('sparse', [0, 2])
def test_hessian_loads_forms_and_datasets(sparse, nt):
    """Datasets whose non-empty-bin counts differ widely, one of them all zeros (an item with no tiles)."""
    m = synth(3, (3, 2), (1500,))
    counts = np.stack([m.counts(dense=True), m.counts(), m.counts(scale=0.02), np.zeros(m.B)])
    ctx = ctx_of(m, counts, sparse=sparse, nt_loads=nt)
    try:
        zs, rs = standard_points(m, 4, seed=5, counts=counts[0])
        ds = np.arange(len(rs)) % 4
        check_hess('hess sparse=%d nt=%d' % (sparse, nt), ctx, m, counts, zs, rs, ds)
    finally:
        ctx.close()


def unbinned_model(n_ev, nan=False):
    """S = 3 sources on 3 x 2 anchors over n_ev events; events 0, 7 and the last have density 0 at every anchor (the
    outlier clamp); with `nan`, source 1 has nan densities at a few events of one anchor."""
    m = synth(3, (3, 2), (n_ev,))
    model = m.dense_model()
    ps = model['ps'] * 300.0
    ps[..., [0, 7, n_ev - 1]] = 0.0
    if nan:
        ps[1, 0, 1, 20:26] = np.nan
    return m, dict(model, ps=ps)


def unbinned_ctx(m, model, outlier=1e-12):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.begin_model(model['anchor_z'], m.S, m.B)
    ps = model['ps'].reshape((-1, m.S, m.B))
    mus = model['mus'].reshape((-1, m.S))
    for a in range(len(mus)):
        ctx.set_anchor(a, ps[a], mus[a])
    ctx.end_model()
    ctx.set_unbinned(outlier)
    return ctx


def test_hessian_unbinned_ragged_events_and_clamp():
    m, model = unbinned_model(1300)
    ctx = unbinned_ctx(m, model)
    try:
        zs, rs = standard_points(m, 4, seed=7, best_fit=False)
        check_hess('hess unbinned', ctx, m, None, zs, rs, model=model, unbinned=True)
        check_hess('hess unbinned', ctx, m, None, zs[:1], rs[:1], model=model, unbinned=True)
    finally:
        ctx.close()


# ---- bi_eval_grad: one work item per point, planned on the device, matrix cores ----------------------------------------

@pytest.mark.parametrize('G,S,n_anchor', [(2, 1, ()), (4, 2, (3,)), (8, 3, (3, 1)), (16, 6, (3, 2, 2))])
def test_gradient_per_item_column_classes(G, S, n_anchor):
    m = synth(S, n_anchor, (700,))
    W = 1 + m.d + S
    assert max(2, 1 << (W - 1).bit_length()) == G
    counts = m.counts(dense=True)
    ctx = ctx_of(m, counts)
    try:
        zs, rs = standard_points(m, 3, seed=G, counts=counts)
        check_grad('grad per item G=%d' % G, ctx, m, counts, zs, rs)
    finally:
        ctx.close()


def test_gradient_refuses_17_columns():
    m = synth(12, (2, 2, 1, 1), (20,))
    assert 1 + m.d + m.S == 17
    ctx = ctx_of(m, m.counts(dense=True))
    try:
        z, r = m.random_points(1, seed=1)
        with pytest.raises(ValueError, match='exceeds 16'):
            ctx.eval_grad(z, r)
    finally:
        ctx.close()


def many_points(m, P, seed, counts):
    zs, rs = m.random_points(P - 3, seed=seed)
    z2, r2 = standard_points(m, 0, seed=seed, counts=counts)
    return np.concatenate([zs, z2]), np.concatenate([rs, r2])


@pytest.mark.parametrize('sparse', [0, 2])
def test_gradient_planned_on_the_device(sparse):
    m = synth(3, (3, 2), (900,))
    counts = np.stack([m.counts(dense=True), m.counts(), np.zeros(m.B)])
    ctx = ctx_of(m, counts, sparse=sparse, grad_mfma=0)
    try:
        zs, rs = many_points(m, 600, seed=4, counts=counts[0])
        ds = np.arange(600) % 3
        ds[-3:] = 0
        P = len(rs)
        check_grad('grad device-planned sparse=%d' % sparse, ctx, m, counts, zs, rs, ds,
                   sample=[0, 1, 2, 301, P - 3, P - 2, P - 1])
    finally:
        ctx.close()


MFMA = [(1, False, 4, ()), (1, True, 3, ()), (2, False, 4, (3,)), (2, True, 3, (3,)),
        (4, False, 4, (3, 2)), (4, True, 3, (3, 2)), (8, False, 4, (2, 3, 2)), (8, True, 3, (2, 3, 2))]


@pytest.mark.parametrize('KG,pad,S,n_anchor', MFMA, ids=['KG%d_%s' % (v[0], 'pad' if v[1] else 'full') for v in MFMA])
def test_gradient_matrix_cores(KG, pad, S, n_anchor):
    m = synth(S, n_anchor, (600,))
    NS = (1 << m.d) * S
    assert (1 if NS <= 4 else 2 if NS <= 8 else 4 if NS <= 16 else 8) == KG and (NS != 4 * KG) == pad
    counts = m.counts(dense=True)
    ctx = ctx_of(m, counts, grad_mfma_min=512)
    try:
        zs, rs = many_points(m, 520, seed=KG, counts=counts)
        before = ctx.get_param('n_grad_mfma_launches')
        P = len(rs)
        check_grad('grad mfma KG=%d pad=%d' % (KG, pad), ctx, m, counts, zs, rs, sample=[0, 1, 260, P - 3, P - 2, P - 1])
        assert ctx.get_param('n_grad_mfma_launches') == before + 1, 'the batch did not take k_grad_mfma'
    finally:
        ctx.close()


# ---- Beeston-Barlow (k_morph_bbgrad) -----------------------------------------------------------------------------------

BBG = [((8, 4), 2, (3,)), ((8, 8), 2, (2, 2, 2, 1)), ((16, 4), 6, (3, 2)), ((16, 8), 4, (2, 2, 3, 1))]


@pytest.mark.parametrize('nt', [0, 1])
@pytest.mark.parametrize('variant,S,n_anchor', BBG, ids=['G%d_DZ%d' % v[0] for v in BBG])
def test_beeston_barlow_gradient_variants(variant, S, n_anchor, nt):
    """B > 512 and a block of bins where the other sources expect exactly nothing (U_b == 0)."""
    m = synth(S, n_anchor, (700,), bb_source=0)
    d, W = m.d, 1 + m.d + S
    assert ((8 if W <= 8 else 16), (4 if 1 + d <= 4 else 8)) == variant
    model = m.dense_model()
    ps = model['ps'].reshape(model['ps'].shape[:d + 1] + (m.B,)).copy()
    ps[..., 1:, 100:160] = 0.0
    model = dict(model, ps=ps.reshape(model['ps'].shape))
    counts = m.counts(dense=True)
    ctx = ctx_of(m, counts, model=model, nt_loads=nt)
    try:
        zs, rs = standard_points(m, 3, seed=S + nt, counts=counts, model=dict(model, n_model=None))
        check_grad('bbgrad G%d DZ%d nt=%d' % (variant + (nt,)), ctx, m, counts, zs, rs, model=model)
    finally:
        ctx.close()


# ---- the unbinned gradient ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nan', [False, True])
def test_unbinned_gradient(nan):
    m, model = unbinned_model(1300, nan=nan)
    ctx = unbinned_ctx(m, model)
    try:
        zs, rs = standard_points(m, 4, seed=11, best_fit=False)
        check_grad('grad unbinned nan=%d' % nan, ctx, m, None, zs, rs, model=model, unbinned=True)
        check_grad('grad unbinned nan=%d' % nan, ctx, m, None, zs[:1], rs[:1], model=model, unbinned=True)
    finally:
        ctx.close()
