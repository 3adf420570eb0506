"""The likelihood VALUE of the device at every launch geometry, against the exact oracle (tests/derivative_oracle.py) with its
per-entry bound |device - oracle| <= C 2^-52 cond and no tolerance of the test's own: k_morph_reduce<G, BB, NT, 0> under the
chunked tile walk (ragged last chunks, narrow and double counts, both load forms), at every grid width class (blocks striding
over the tiles, the XCD rounding, both forms of k_finish), across the 256-item limit of the in-launch finish and the 65 535-item
launch seam, in every group class; k_morph_single with its launch shapes, its collector's second trip, the two-kernel
fallback and the kept rows; changes of geometry within one context (same bits, no mailbox reset); the Beeston-Barlow vector
kernel at every group size, G = 16 included; and a Beeston-Barlow batch whose one group is larger than k_scan_bb's grid.
The counters last_morph_nbx / last_morph_items / last_morph_fused say which geometry a case reached: the tests never restate the
host's formulas and assume no CU count.  The models and points are tests/value_geometry_cases.py's.  Run with -s for the worst
|err| / (2^-52 cond) per family."""
import numpy as np
import pytest

import derivative_oracle as do
import value_geometry_cases as vg

pytestmark = pytest.mark.gpu

WORST = {}
REACHED = {}
BIG = 1 << 40


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    print('\nworst |err| / (2^-52 cond) per family (C = %d):' % do.C_POISSON)
    for k in sorted(WORST):
        print('  %-40s %.3g' % (k, WORST[k]))
    for k in sorted(REACHED):
        print('  reached %-32s %s' % (k, REACHED[k]))


def context(c, **params):
    """A DeviceContext with the model and data of case c: dense evaluations, every batch planned on the host."""
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', 0)
    ctx.set_param('device_plan_min', BIG)
    for k, v in params.items():
        ctx.set_param(k, v)
    c.upload(ctx)
    return ctx


DEFAULTS = dict(tile_chunks=8, narrow_counts=1, nt_loads=2, max_group=16, blocks_per_cu=8, xcd_affine=1, fuse_finish=1,
                single_blocks_per_cu=4, fuse_max_blocks=1 << 20, single_kernel=1, keep_rows=-1)


def settings(ctx, **over):
    for k, v in dict(DEFAULTS, **over).items():
        ctx.set_param(k, v)


def geometry(ctx):
    return ctx.get_param('last_morph_nbx'), ctx.get_param('last_morph_items'), ctx.get_param('last_morph_fused')


def hold(family, tag, got, st, want, cond, C=do.C_POISSON, named=()):
    """Every entry within the bound and every status word 0; `named`: indices whose results the failure message spells out."""
    got, st, want, cond = (np.atleast_1d(x) for x in (got, st, want, cond))
    extra = ''.join('\n  [%d] got %r want %r status %d' % (i, got[i], want[i], st[i]) for i in named)
    assert (st == 0).all(), '%s: status %s at %s%s' % (tag, st[st != 0][:4], np.flatnonzero(st)[:4], extra)
    try:
        worst = do.check_entries(got, want, cond, C, tag)
    except AssertionError as e:
        raise AssertionError(str(e) + extra) from None
    WORST[family] = max(WORST.get(family, 0.0), worst)


def eval_one(ctx, c, z, r, ds=0, halves=False):
    if halves:
        ctx.eval_begin(z if c.m.d else None, r, ds)
        return ctx.eval_end()
    ll, st = ctx.eval(z[None] if c.m.d else None, r[None], dataset=[ds])
    return ll[0], st[0]


# ---- the tile walk (batched, few items) -----------------------------------------------------------------------------------

WALK = [dict(), dict(tile_chunks=1), dict(tile_chunks=2), dict(tile_chunks=3), dict(narrow_counts=0), dict(nt_loads=0),
        dict(nt_loads=1), dict(tile_chunks=2, narrow_counts=0, nt_loads=0), dict(tile_chunks=3, narrow_counts=0, nt_loads=1),
        dict(tile_chunks=2, nt_loads=1), dict(tile_chunks=3, nt_loads=0)]


@pytest.mark.parametrize('n_tiles,fill', vg.TILE_SHAPES, ids=['tiles%d_fill%d' % tf for tf in vg.TILE_SHAPES])
def test_tile_walk(n_tiles, fill):
    c = vg.tile_case(n_tiles, fill)
    zs, rs = vg.standard_points(c)
    want, cond = c.oracle_many(zs, rs)
    ctx = context(c)
    try:
        assert ctx.get_param('narrow_ready') == 1
        for over in WALK:
            settings(ctx, **over)
            before = ctx.get_param('n_narrow_launches')
            ll, st = ctx.eval(zs, rs)
            tag = 'walk tiles=%d fill=%d %s' % (n_tiles, fill, over)
            hold('tile walk', tag, ll, st, want, cond)
            assert (ctx.get_param('n_narrow_launches') > before) == (over.get('narrow_counts', 1) == 1), tag
            nbx, items, fused = geometry(ctx)
            assert 1 <= nbx <= n_tiles and 1 <= items <= len(rs) and fused == 1, tag
    finally:
        ctx.close()


# ---- the grid width ---------------------------------------------------------------------------------------------------------

def repeated(c, P, n_proto=5):
    """P points, the standard points of c repeated -> (z, r, want, cond)."""
    zs, rs = vg.standard_points(c)
    want, cond = c.oracle_many(zs, rs)
    idx = np.arange(P) % n_proto
    return zs[idx], rs[idx], want[idx], cond[idx]


def test_grid_width_classes():
    """One work item per point (max_group = 1) on the 196-tile model: the fixed requests, then a few whose P follows from the
    device's CU count (four blocks per slot over P items: P near 4 n_cu blocks_per_cu / k aims at about k blocks per item)."""
    c = vg.tile_case(196, vg.TILE - 1)
    ctx = context(c)
    try:
        n_cu = ctx.info()['n_cu']
        requests = [(bpc, P) for bpc in (1, 8, 32) for P in (2, 64, 100, 255, 256, 257)]
        requests += [(1, max(2, min(600, 4 * n_cu // k))) for k in (3, 11, 13, 100)] + [(8, max(2, min(600, 32 * n_cu // k))) for k in (100, 150)]
        classes = {k: [] for k in ('nbx == tiles', 'rounded to 8', 'same request unrounded', 'nbx <= 4', 'k_finish whole block',
                                   'k_finish one wave')}
        for bpc, P in requests:
            zs, rs, want, cond = repeated(c, P)
            seen = {}
            for affine, fuse in ((1, 1), (0, 1), (1, 0)):
                settings(ctx, max_group=1, blocks_per_cu=bpc, xcd_affine=affine, fuse_finish=fuse)
                ll, st = ctx.eval(zs, rs)
                nbx, items, fused = geometry(ctx)
                tag = 'width bpc=%d P=%d affine=%d fuse=%d nbx=%d' % (bpc, P, affine, fuse, nbx)
                hold('grid width', tag, ll, st, want, cond)
                assert items == P and 1 <= nbx <= c.n_tiles, tag
                assert fused == (1 if fuse and P <= 256 else 0), tag
                seen[(affine, fuse)] = nbx
                if nbx == c.n_tiles:
                    classes['nbx == tiles'].append(tag)
                if nbx <= 4:
                    classes['nbx <= 4'].append(tag)
                if not fuse:
                    classes['k_finish whole block' if nbx > 64 else 'k_finish one wave'].append(tag)
            if 4 < seen[(1, 1)] < c.n_tiles and seen[(1, 1)] % 8 == 0:
                classes['rounded to 8'].append('bpc=%d P=%d nbx=%d' % (bpc, P, seen[(1, 1)]))
                if seen[(0, 1)] % 8 != 0:
                    classes['same request unrounded'].append('bpc=%d P=%d nbx=%d' % (bpc, P, seen[(0, 1)]))
        for k, v in classes.items():
            REACHED[k] = '%d launches, e.g. %s' % (len(v), v[0] if v else '-')
        missing = [k for k, v in classes.items() if not v]
        assert not missing, 'no launch of the list reached %s on this device (%d CUs)' % (missing, n_cu)
    finally:
        ctx.close()


# ---- the finish route -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fuse', [1, 0])
def test_finish_route_around_256_items(fuse):
    c = vg.tile_case(9, 1)
    ctx = context(c)
    try:
        for P in (255, 256, 257):
            zs, rs, want, cond = repeated(c, P)
            settings(ctx, max_group=1, fuse_finish=fuse)
            ll, st = ctx.eval(zs, rs)
            nbx, items, fused = geometry(ctx)
            tag = 'finish P=%d fuse_finish=%d' % (P, fuse)
            hold('finish route', tag, ll, st, want, cond)
            assert items == P, tag
            assert fused == (1 if fuse and P <= 256 else 0), tag
    finally:
        ctx.close()


# ---- the launch seam --------------------------------------------------------------------------------------------------------

def test_launch_seam_at_65535_items():
    c = vg.seam_case()
    P, n_proto = vg.SEAM_POINTS, vg.SEAM_PROTOTYPES
    pz, pr = vg.prototypes(c, n_proto)
    want, cond = c.oracle_many(pz, pr)
    idx = np.arange(P) % n_proto
    ctx = context(c)
    try:
        settings(ctx, max_group=1)
        ll, st = ctx.eval(None, pr[idx])
        nbx, items, fused = geometry(ctx)
        hold('launch seam', 'seam P=%d' % P, ll, st, want[idx], cond[idx], named=(P - 3, P - 2, P - 1))
        assert items == 2 and fused == 0, 'the second launch should hold 2 work items, not %d' % items
    finally:
        ctx.close()


# ---- group classes ----------------------------------------------------------------------------------------------------------

def group_pool(c):
    """17 points of the lower cell on dataset 0, then 2 of the upper cell, then 2 of the lower cell on dataset 1."""
    rng = np.random.default_rng(31)
    g = c.m.anchor_z[0]
    z = np.concatenate([rng.uniform(g[0], g[1] - 0.01, 17), rng.uniform(g[1], g[2], 2), rng.uniform(g[0], g[1] - 0.01, 2)])[:, None]
    r = rng.uniform(0.6, 1.4, (21, c.m.S))
    ds = np.array([0] * 19 + [1] * 2)
    return z, r, ds


@pytest.mark.parametrize('max_group', [1, 2, 4, 8, 16])
def test_group_classes(max_group):
    c = vg.group_case()
    z, r, ds = group_pool(c)
    want, cond = c.oracle_many(z, r, ds)
    ctx = context(c)
    try:
        for n in (1, 2, 3, 5, 9, 16, 17):
            take = np.r_[0:n, 17:21]
            # the group's points are not neighbours in the batch
            order = np.random.default_rng(n).permutation(len(take))
            take = take[order]
            settings(ctx, max_group=max_group)
            ll, st = ctx.eval(z[take], r[take], dataset=ds[take])
            hold('group classes', 'groups max_group=%d n=%d' % (max_group, n), ll, st, want[take], cond[take])
            assert ctx.get_param('last_morph_fused') == 1
    finally:
        ctx.close()


# ---- single evaluations -----------------------------------------------------------------------------------------------------

SINGLE = [dict(), dict(single_blocks_per_cu=1), dict(single_blocks_per_cu=32), dict(fuse_max_blocks=0), dict(single_kernel=0),
          dict(keep_rows=0), dict(keep_rows=3), dict(keep_rows=3, nt_loads=1, tile_chunks=2), dict(single_blocks_per_cu=32, tile_chunks=3),
          dict(narrow_counts=0, nt_loads=0, tile_chunks=2)]


@pytest.mark.parametrize('n_tiles,fill', vg.TILE_SHAPES, ids=['tiles%d_fill%d' % tf for tf in vg.TILE_SHAPES])
def test_single_evaluation(n_tiles, fill):
    c = vg.tile_case(n_tiles, fill)
    zs, rs = vg.standard_points(c)
    want, cond = c.oracle_many(zs, rs)
    ctx = context(c)
    try:
        for over in SINGLE:
            settings(ctx, **over)
            # three calls in the lower cell, then the upper cell (the kept rows follow the cell)
            for call, p in enumerate((0, 1, 0, 2, 3, 4)):
                ll, st = eval_one(ctx, c, zs[p], rs[p], halves=bool(call & 1))
                nbx, items, fused = geometry(ctx)
                tag = 'single tiles=%d fill=%d %s call %d nbx=%d' % (n_tiles, fill, over, call, nbx)
                hold('single evaluation', tag, ll, st, want[p], cond[p])
                assert items == 1 and 1 <= nbx <= n_tiles, tag
                assert fused == (0 if over.get('single_kernel') == 0 or over.get('fuse_max_blocks') == 0 else 1), tag
    finally:
        ctx.close()


def test_single_evaluation_collector_second_trip():
    """No shape axis, one source, 1025 tiles, 32 blocks per CU asked for: more than 1024 blocks, so the collecting block's loop over
    the mailbox makes a second trip."""
    c = vg.single_big_case()
    zs, rs = vg.standard_points(c)
    want, cond = c.oracle_many(zs[:2], rs[:2])
    ctx = context(c)
    try:
        for over in (dict(single_blocks_per_cu=32, blocks_per_cu=32), dict(single_blocks_per_cu=32, blocks_per_cu=32, fuse_max_blocks=0)):
            settings(ctx, **over)
            for p in (0, 1):
                ll, st = eval_one(ctx, c, zs[p], rs[p], halves=bool(p))
                nbx, items, fused = geometry(ctx)
                tag = 'single %d tiles %s nbx=%d' % (c.n_tiles, over, nbx)
                hold('single evaluation, > 1024 blocks', tag, ll, st, want[p], cond[p])
                assert nbx > 1024, tag
                assert fused == (0 if 'fuse_max_blocks' in over else 1), tag
        REACHED['single blocks'] = nbx
    finally:
        ctx.close()


# ---- changes of geometry in one context ----------------------------------------------------------------------------------------

def test_shape_changes_keep_the_bits_and_the_mailbox():
    c = vg.tile_case(129, vg.TILE - 1)
    zs, rs = vg.standard_points(c)
    want, cond = c.oracle_many(zs, rs)
    zb, rb, want_b, cond_b = repeated(c, 100)
    ctx = context(c)
    try:
        geo_a = dict(tile_chunks=2)
        resets = ctx.get_param('n_mail_resets')

        def run_a():
            settings(ctx, **geo_a)
            ll, st = ctx.eval(zs, rs)
            assert ctx.get_param('last_morph_fused') == 1
            hold('shape changes', 'geometry A', ll, st, want, cond)
            return ll, geometry(ctx)

        a1, g1 = run_a()
        # B: a hundred one-point items on a narrow grid, the plain walk
        settings(ctx, max_group=1, blocks_per_cu=1, tile_chunks=1)
        ll_b, st_b = ctx.eval(zb, rb)
        gb = geometry(ctx)
        assert gb[2] == 1 and gb != g1, (g1, gb)
        hold('shape changes', 'geometry B', ll_b, st_b, want_b, cond_b)
        a2, g2 = run_a()
        assert g2 == g1
        assert np.array_equal(a1, a2), 'the same geometry gave other bits after a launch of another shape: %r' % (a1 - a2)
        # the single-evaluation kernel between two batched launches (the same mailbox)
        settings(ctx, **geo_a)
        for p in range(len(rs)):
            ll, st = eval_one(ctx, c, zs[p], rs[p])
            assert ctx.get_param('last_morph_fused') == 1
            hold('shape changes', 'single between', ll, st, want[p], cond[p])
        a3, g3 = run_a()
        assert g3 == g1 and np.array_equal(a1, a3)
        assert ctx.get_param('n_mail_resets') == resets
    finally:
        ctx.close()


# ---- the Beeston-Barlow vector kernel ---------------------------------------------------------------------------------------

def bb_points(c):
    """17 points of the lower cell and 3 of the upper: two prototypes of each repeated -> (z, r, prototype index)."""
    zs, rs = vg.standard_points(c)                      # 0, 1: lower cell; 2: upper cell; 3: the middle anchor (upper cell)
    idx = np.array([i % 2 for i in range(17)] + [2, 3, 2])
    return zs, rs, idx


@pytest.mark.parametrize('n_tiles', vg.BB_TILES)
@pytest.mark.parametrize('bb_max_group', [1, 2, 4, 8, 16])
def test_beeston_barlow_vector_kernel(bb_max_group, n_tiles):
    c = vg.bb_case(n_tiles)
    zs, rs, idx = bb_points(c)
    want, cond = c.oracle_many(zs[:4], rs[:4])
    ctx = context(c, scan_bb=0)
    try:
        for over in (dict(), dict(nt_loads=1, narrow_counts=0)):
            settings(ctx, tile_chunks=2 if n_tiles >= 128 else 8, **over)
            ctx.set_param('bb_max_group', bb_max_group)
            scans = ctx.get_param('n_bb_scan_launches')
            ll, st = ctx.eval(zs[idx], rs[idx])
            tag = 'bb G<=%d tiles=%d %s' % (bb_max_group, n_tiles, over)
            hold('beeston-barlow G<=%d' % bb_max_group, tag, ll, st, want[idx], cond[idx], C=do.C_BB)
            assert ctx.get_param('n_bb_scan_launches') == scans and ctx.get_param('last_morph_fused') == 1, tag
    finally:
        ctx.close()


def test_beeston_barlow_group_beyond_the_scan_grid():
    """One (cell, dataset) group of 4 x 65 535 + 1 sixteen-point items: more quads than k_scan_bb's gridDim.z can count, so the
    device-planned batch runs through k_morph_reduce<16, true> (no k_scan_bb launch) and every value meets the bound."""
    c = vg.bb_scan_case()
    n_proto = 64
    pz, pr = vg.prototypes(c, n_proto)
    want, cond = c.oracle_many(pz, pr)
    P = 16 * vg.BB_SCAN_ITEMS
    idx = np.arange(P) % n_proto
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    try:
        ctx.set_param('sparse', 0)
        c.upload(ctx)
        assert ctx.get_param('scan_bb') == 1 and P >= ctx.get_param('device_plan_min')
        scans = ctx.get_param('n_bb_scan_launches')
        ll, st = ctx.eval(None, pr[idx])
        assert ctx.get_param('n_bb_scan_launches') == scans, 'the batch went to k_scan_bb'
        hold('beeston-barlow beyond the scan grid', 'bb %d items' % vg.BB_SCAN_ITEMS, ll, st, want[idx], cond[idx], C=do.C_BB,
             named=(0, P - 1))
        nbx, items, fused = geometry(ctx)
        assert items == vg.BB_SCAN_ITEMS % 65535 and fused == 0
        # a batch the scan kernel does take, in the same context: the route is chosen by the group's size
        ll, st = ctx.eval(None, pr[idx[:4096]])
        assert ctx.get_param('n_bb_scan_launches') == scans + 1
        assert (st == 0).all() and np.isfinite(ll).all()
    finally:
        ctx.close()
