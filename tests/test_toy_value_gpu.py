"""The toy-MC EVALUATION kernels (bi_eval_datasets, bi_eval_datasets_points: csrc/bi_toys.h, csrc/bi_k_toys.h) held to the exact
oracle, every dataset of every call: |device - oracle| <= 256 * 2^-52 * cond (derivative_oracle.check_entries), status 0, rows
the oracle gives as -inf compared with ==.  The table (tests/toy_value_cases.py) places every edge of the tile-major lists and
of the walk over them on purpose; tests/test_toy_value_cases.py shows on the CPU that it does and that the bound rejects every
mutant.  Every case asserts the route it took -- tm_entry_bytes / tmm_entry_bytes (0 after a build that failed), the movement of
n_toy_polled (a tiled single-point call with toy_fast_call = 7 polls its completion word once; no row kernel call does) and of
n_toy_points_passes -- so that a fallback cannot turn a case into a repeat of another.  Run with -s for the worst ratio per route."""
import time

import numpy as np
import pytest

import toy_value_cases as tv

pytestmark = pytest.mark.gpu

WORST = {}


def note(route, worst):
    WORST[route] = max(WORST.get(route, 0.0), worst)


@pytest.fixture(scope='module', autouse=True)
def report():
    t_start = time.time()
    yield
    print('\ntoy-MC evaluation, worst |err| / (2^-52 cond) per route (C = 256); wall time of the file %.1f s' % (time.time() - t_start))
    for k in sorted(WORST):
        print('  %-44s %.3g' % (k, WORST[k]))


def _context(tab):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    tab.upload(ctx)
    return ctx


def _fixture(name, anchors, variant):
    @pytest.fixture(scope='module', name=name)
    def f():
        tab = tv.edge_table(anchors, variant)
        ctx = _context(tab)
        yield tab, ctx
        ctx.close()
    return f


fx_base = _fixture('base', (0.0, 1.0), None)
fx_count8 = _fixture('count8', (0.0, 1.0), 'count8')
fx_count32767 = _fixture('count32767', (0.0, 1.0), 'count32767')
fx_count32768 = _fixture('count32768', (0.0, 1.0), 'count32768')
fx_base3 = _fixture('base3', tv.ANCHORS_3, None)
fx_wide3 = _fixture('wide3', tv.ANCHORS_3, 'count32767')

DEFAULTS = dict(sparse=1, dot_tiled=1, dot_entry16=1, dot_lanes=0, dot_blocks_per_cu=0, toy_fast_call=7, toy_points_pp=0,
                toy_points_lanes=0, toy_points_overlap=0)


class params:
    """set tunables for a case, put the defaults back after it"""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_param(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.ctx.set_param(k, DEFAULTS[k])


def single(tab, ctx, point, route, t0=0, t1=None):
    """One bi_eval_datasets call held to the oracle -> how far n_toy_polled moved."""
    z, rs = point
    t1 = tab.T if t1 is None else t1
    polled = ctx.get_param('n_toy_polled')
    ll, st = ctx.eval_datasets([z], rs, t0, t1)
    moved = ctx.get_param('n_toy_polled') - polled
    assert st == 0 and ll.shape == (t1 - t0,)
    want, cond = tab.oracle(z, rs)
    note(route, tv.check(ll, want[t0:t1], cond[t0:t1], '%s at z = %g, datasets [%d, %d)' % (route, z, t0, t1)))
    return moved


def several(tab, ctx, z, rs, route, t0=0, t1=None, rows=None, device=False):
    """One bi_eval_datasets_points call held to the oracle (rows: the points to hold; default all) -> (passes made, ll, status)."""
    t1 = tab.T if t1 is None else t1
    before = ctx.get_param('n_toy_points_passes')
    if device:
        buf = ctx.device_alloc(8 * len(z) * (t1 - t0))
        st = ctx.eval_datasets_points_device(buf.ptr, z, rs, t0, t1)
        ll = buf.to_host(np.float64, len(z) * (t1 - t0)).reshape(len(z), t1 - t0)
        buf.free()
    else:
        ll, st = ctx.eval_datasets_points(z, rs, t0, t1)
    passes = ctx.get_param('n_toy_points_passes') - before
    assert ll.shape == (len(z), t1 - t0)
    for p in (range(len(z)) if rows is None else rows):
        assert st[p] == 0
        want, cond = tab.oracle(z[p], rs[p])
        note(route, tv.check(ll[p], want[t0:t1], cond[t0:t1], '%s, point %d of %d, datasets [%d, %d)' % (route, p, len(z), t0, t1)))
    return passes, ll, st


POINTS = pytest.mark.parametrize('point', tv.POINTS_1, ids=['lower_half', 'upper_half_zero_rate'])


# ---- one point -------------------------------------------------------------------------------------------------------------------

@POINTS
def test_row_kernels(base, point):
    tab, ctx = base
    with params(ctx, sparse=0):                                       # the dense counts of the upload
        assert ctx.get_param('dense_counts') == 1 and ctx.get_param('sparse') == 0
        assert single(tab, ctx, point, 'single: dense row kernel') == 0
    with params(ctx, dot_tiled=0):                                    # the dataset-major lists, one block per dataset
        assert ctx.get_param('csr_ready') == 1
        assert single(tab, ctx, point, 'single: list row kernel') == 0


@POINTS
@pytest.mark.parametrize('entry16,lanes,width,name', [(1, 0, 2, '<4, 3, 2>'), (1, 8, 2, '<8, 2, 2>'), (0, 0, 4, '<8, 3, 4>'), (0, 16, 4, '<16, 2, 4>')],
                         ids=['L4_A3_W2', 'L8_A2_W2', 'L8_A3_W4', 'L16_A2_W4'])
def test_tiled_route_every_instantiation(base, point, entry16, lanes, width, name):
    tab, ctx = base
    with params(ctx, dot_entry16=entry16, dot_lanes=lanes):
        assert single(tab, ctx, point, 'single: tiled ' + name) == 1
        assert ctx.get_param('tm_entry_bytes') == width


@POINTS
def test_tiled_route_call_forms(base, point):
    tab, ctx = base
    with params(ctx, dot_blocks_per_cu=1):
        assert single(tab, ctx, point, 'single: tiled, dot_blocks_per_cu 1') == 1
    assert single(tab, ctx, point, 'single: tiled, toy_fast_call 7') == 1
    with params(ctx, toy_fast_call=0):
        # (descriptors copied, k_dataset_finish over the tiled partials, a stream synchronisation instead of the completion word;
        #  the gates of the tiled route do not depend on toy_fast_call, and the call above took it)
        assert single(tab, ctx, point, 'single: tiled, toy_fast_call 0') == 0
    assert ctx.get_param('tm_entry_bytes') == 2


@POINTS
def test_sub_ranges(base, point):
    tab, ctx = base
    assert single(tab, ctx, point, 'single: tiled, datasets [1, 65)', 1, 65) == 1            # n = 64: the gate of the tiled route
    assert single(tab, ctx, point, 'single: list row kernel, datasets [5, 68)', 5, 68) == 0  # n = 63: the row kernel
    assert single(tab, ctx, point, 'single: tiled, datasets [0, 257)', 0, 257) == 1          # two slices: 129 + 128
    assert single(tab, ctx, point, 'single: tiled, datasets [300, 600)', 300, 600) == 1
    assert ctx.get_param('tm_entry_bytes') == 2


@POINTS
def test_count_8_takes_four_byte_entries(count8, point):
    tab, ctx = count8
    assert single(tab, ctx, point, 'single: tiled, count 8') == 1
    assert ctx.get_param('tm_entry_bytes') == 4


@POINTS
def test_count_32767_is_the_largest_a_four_byte_entry_holds(count32767, point):
    tab, ctx = count32767
    assert single(tab, ctx, point, 'single: tiled, count 32767') == 1
    assert ctx.get_param('tm_entry_bytes') == 4
    with params(ctx, dot_lanes=16):
        assert single(tab, ctx, point, 'single: tiled, count 32767') == 1


@POINTS
def test_count_32768_fits_neither_width_and_takes_the_row_kernel(count32768, point):
    tab, ctx = count32768
    assert single(tab, ctx, point, 'single: list row kernel, count 32768') == 0
    assert ctx.get_param('tm_entry_bytes') == 0 and ctx.get_param('csr_ready') == 1


# ---- several points --------------------------------------------------------------------------------------------------------------

def n_passes(n_valid, pp=0):
    per = 2 if (pp == 2 or (pp == 0 and n_valid <= 2)) else 4
    return -(-n_valid // per)


@pytest.mark.parametrize('P', [2, 3, 4, 5, 8, 9])
def test_points_in_both_cells(base3, P):
    tab, ctx = base3
    z, rs = tv.multi_points(P)
    passes, _, _ = several(tab, ctx, z, rs, 'multi: two-byte entries')
    assert passes == n_passes(P) and ctx.get_param('tmm_entry_bytes') == 2


def test_points_that_differ_in_rates_only(base3):
    tab, ctx = base3
    z, rs = tv.rate_points(8)
    passes, _, _ = several(tab, ctx, z, rs, 'multi: one cell, rates only')
    assert passes == 2 and ctx.get_param('tmm_entry_bytes') == 2


def test_rejected_points_interleaved(base3):
    tab, ctx = base3
    z, rs = tv.multi_points(6)
    z, rs = z.copy(), rs.copy()
    z[1, 0] = 99.0                                                    # outside the grid
    rs[4, 1] = -1.0                                                   # a negative rate
    ok = [0, 2, 3, 5]
    passes, ll, st = several(tab, ctx, z, rs, 'multi: rejected points among them', rows=ok)
    assert passes == n_passes(4) and ctx.get_param('tmm_entry_bytes') == 2
    for p in (1, 4):                                                  # exactly what bi_eval answers for the point
        v, s = ctx.eval(z[p:p + 1], rs[p:p + 1])
        assert s[0] != 0 and st[p] == s[0] and np.all(ll[p] == v[0])
    assert st[1] != st[4]


@pytest.mark.parametrize('pp', [0, 2, 4])
def test_points_per_pass(base3, pp):
    tab, ctx = base3
    z, rs = tv.multi_points(5)
    with params(ctx, toy_points_pp=pp):
        passes, _, _ = several(tab, ctx, z, rs, 'multi: toy_points_pp %d' % pp)
    assert passes == n_passes(5, pp) and ctx.get_param('tmm_entry_bytes') == 2


@pytest.mark.parametrize('width,lanes', [(2, 2), (2, 4), (2, 8), (4, 4), (4, 8)])
@pytest.mark.parametrize('pp', [4, 2])
def test_lanes_of_every_instantiation(base3, width, lanes, pp):
    tab, ctx = base3
    z, rs = tv.multi_points(5)
    with params(ctx, dot_entry16=1 if width == 2 else 0, toy_points_lanes=lanes, toy_points_pp=pp):
        passes, _, _ = several(tab, ctx, z, rs, 'multi: <L %d, W %d, PP %d>' % (lanes, width, pp))
        assert passes == n_passes(5, pp) and ctx.get_param('tmm_entry_bytes') == width


@pytest.mark.parametrize('lanes', [4, 8])
def test_four_byte_entries_with_their_largest_count(wide3, lanes):
    tab, ctx = wide3
    z, rs = tv.multi_points(5)
    with params(ctx, toy_points_lanes=lanes):
        passes, _, _ = several(tab, ctx, z, rs, 'multi: four-byte entries, count 32767')
        assert passes == 2 and ctx.get_param('tmm_entry_bytes') == 4


@pytest.mark.parametrize('overlap', [0, 1])
def test_second_stream(base3, overlap):
    tab, ctx = base3
    z, rs = tv.multi_points(9)                                        # three passes: two groups, the second one pass short
    with params(ctx, toy_points_overlap=overlap):
        passes, _, _ = several(tab, ctx, z, rs, 'multi: toy_points_overlap %d' % overlap)
    assert passes == 3 and ctx.get_param('tmm_entry_bytes') == 2


def test_results_left_on_the_device(base3):
    tab, ctx = base3
    z, rs = tv.multi_points(5)
    passes, _, _ = several(tab, ctx, z, rs, 'multi: out_dev', device=True)
    assert passes == 2


def test_sub_ranges_of_several_points(base3):
    tab, ctx = base3
    z, rs = tv.multi_points(3)
    passes, _, _ = several(tab, ctx, z, rs, 'multi: datasets [0, 257)', 0, 257)
    assert passes == 1
    polled = ctx.get_param('n_toy_polled')
    passes, _, _ = several(tab, ctx, z, rs, 'multi: point by point, datasets [5, 68)', 5, 68)
    assert passes == 0 and ctx.get_param('n_toy_polled') == polled    # n = 63: bi_eval_datasets' row kernel, point by point


# ---- generated toys --------------------------------------------------------------------------------------------------------------

def test_generated_toys_every_dataset(base):
    """The generator's sum lgamma (k_toy_lgsum, k_toy_events) against an independent lgamma for every dataset: the toys are
    fetched back and every route is held to values() of the fetched counts."""
    from blueice_amd.device import DeviceContext
    model = base[0].model
    ctx = DeviceContext(0)
    try:
        ctx.upload_model(model['anchor_z'], model['ps'], model['mus'])
        ctx.set_param('sparse', 1)
        (z, rs), other = tv.POINTS_1
        T = tv.T_EDGE
        ctx.generate_toys([z], rs, T, seed=20)
        counts = np.stack([ctx.download_counts(t) for t in range(T)])
        nnz = int((counts > 0).sum())
        assert np.all(counts == np.floor(counts)) and counts.min() >= 0 and 1 <= counts.max() <= 7
        assert nnz == ctx.get_param('nnz_total') and nnz >= 16 * T * 5 and nnz >= 8 * T * 9
        tab = tv.Table(model, counts, {}, {}, None, [])
        for point in ((z, rs), other):
            assert single(tab, ctx, point, 'generated toys: tiled') == 1
            assert ctx.get_param('tm_entry_bytes') == 2
            with params(ctx, dot_tiled=0):
                assert single(tab, ctx, point, 'generated toys: list row kernel') == 0
        zs, rss = tv.rate_points(3, z=0.6)
        passes, _, _ = several(tab, ctx, zs, rss, 'generated toys: multi')
        assert passes == 1 and ctx.get_param('tmm_entry_bytes') == 2
        ctx.counts_to_dense()
        with params(ctx, sparse=0):
            assert ctx.get_param('dense_counts') == 1
            assert single(tab, ctx, (z, rs), 'generated toys: dense row kernel') == 0
    finally:
        ctx.close()


# ---- the dense seam --------------------------------------------------------------------------------------------------------------

def test_dense_datasets_past_the_chunk_of_the_dense_route():
    from blueice_amd.device import DeviceContext
    tab = tv.seam_table()
    ctx = DeviceContext(0)
    try:
        ctx.upload_model([], tab.model['ps'], tab.model['mus'])
        ctx.set_param('sparse', 0)
        ctx.upload_counts(tab.counts)
        assert ctx.get_param('dense_counts') == 1 and ctx.get_param('csr_ready') == 0
        rs = (1.2, 0.9)
        polled = ctx.get_param('n_toy_polled')
        ll, st = ctx.eval_datasets(None, rs)
        assert st == 0 and ll.shape == (tab.T,) and ctx.get_param('n_toy_polled') == polled
        want, cond = tab.oracle(None, rs)
        note('single: dense row kernel, 16 390 datasets', tv.check(ll, want, cond, 'dense seam'))
    finally:
        ctx.close()
