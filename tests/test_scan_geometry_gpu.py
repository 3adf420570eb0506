"""The likelihood scans on the fp64 matrix cores at every launch geometry, against the exact oracle (tests/derivative_oracle.py)
with its per-entry bound |device - oracle| <= C 2^-52 cond at EVERY point of every batch and no tolerance of the test's own:
k_scan_sorted (rows in count order: the sorted copy of dense data and the count-sorted compacted copy), k_scan_mfma<2> / <4> (rows
in bin order, PROD = 1 on compacted rows) and the split scan (k_morph_reduce on the compacted rows + k_scan_valid), under forced
strip splits, the three block mappings, every item-list remainder with and without chunked groups, every strip class, every
stream-group class, and the fallbacks.  nan / -inf patterns are asserted exactly, status words are 0, and the counters
last_scan_nslots / _groups / _max_items / _cb / _by_count / _prod, last_valid_nslots, n_scan_launches, n_sorted_scans and
n_valid_launches say which route and geometry a batch reached: the tests restate none of the planner's formulas and assume no
CU count.  The models, prototypes and batches are tests/scan_geometry_cases.py's.  Run with -s for the worst |err| / (2^-52 cond)
per family and the classes reached."""
import numpy as np
import pytest

import derivative_oracle as do
import scan_geometry_cases as sg

pytestmark = pytest.mark.gpu

WORST = {}
REACHED = {}

# route -> the parameters set before the upload (the compacted copy and its order are made at upload_counts)
ROUTES = {
    'sorted': dict(sparse=0),                              # k_scan_sorted on the count-sorted copy of all bins
    'compacted, count order': dict(sparse=2),              # k_scan_sorted on the count-sorted compacted rows
    'bin order, 32-bin strips': dict(sparse=0, scan_pow=0),           # k_scan_mfma<2>
    'bin order, 64-bin strips': dict(sparse=0, scan_cb=4),            # k_scan_mfma<4>
    'compacted, bin order': dict(sparse=2, scan_pow=0),    # k_scan_mfma<2, KG, MASK, 1>
}
# route -> (last_scan_by_count, last_scan_cb, last_scan_prod)
KERNEL = {'sorted': (1, 4, 0), 'compacted, count order': (1, 4, 0), 'bin order, 32-bin strips': (0, 2, 0),
          'bin order, 64-bin strips': (0, 4, 0), 'compacted, bin order': (0, 2, 1)}
SPLIT = dict(sparse=0, scan_split=1)


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    print('\nworst |err| / (2^-52 cond) per family (C = %d):' % do.C_POISSON)
    for k in sorted(WORST):
        print('  %-40s %.3g' % (k, WORST[k]))
    for k in sorted(REACHED):
        print('  reached %-40s %s' % (k, REACHED[k]))


def context(c, **params):
    """A DeviceContext with the model and data of case c in which a few hundred points are planned on the device and take a scan."""
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    for k, v in dict(dict(device_plan_min=1, scan_min_items=1), **params).items():
        ctx.set_param(k, v)
    c.upload(ctx)
    return ctx


COUNTERS = ('n_scan_launches', 'n_sorted_scans', 'n_valid_launches', 'last_scan_nslots', 'last_valid_nslots', 'last_scan_groups',
            'last_scan_max_items', 'last_scan_cb', 'last_scan_by_count', 'last_scan_prod')


def counters(ctx):
    return {k: ctx.get_param(k) for k in COUNTERS}


def run(ctx, c, family, tag, cell_points, ds_of_cell=None, seed=3):
    """Evaluate the batch, hold EVERY point to the oracle -> (values, counters before, counters after)."""
    z, r, ds, protos = sg.batch(c, cell_points, ds_of_cell, seed)
    before = counters(ctx)
    got, st = ctx.eval(z, r, dataset=ds if c.T > 1 else None)
    after = counters(ctx)
    want, cond, kind = c.expected(protos, ds)
    assert (st == 0).all(), '%s: status %s at %s' % (tag, st[st != 0][:4], np.flatnonzero(st)[:4])
    nan, inf, bound = kind == 'nan', kind == '-inf', kind == 'bound'
    wrong = np.flatnonzero(np.isnan(got) != nan)
    assert not len(wrong), '%s: nan pattern differs at points %s (prototypes %s)' % (tag, wrong[:4], protos[wrong[:4]])
    wrong = np.flatnonzero((got == -np.inf) != inf)
    assert not len(wrong), '%s: -inf pattern differs at points %s (prototypes %s): %s' % (tag, wrong[:4], protos[wrong[:4]], got[wrong[:4]])
    worst = do.check_entries(got[bound], want[bound], cond[bound], do.C_POISSON, tag)
    WORST[family] = max(WORST.get(family, 0.0), worst)
    return got, before, after


def took(route, before, after, tag):
    assert after['n_scan_launches'] == before['n_scan_launches'] + 1, '%s: no matrix-core scan launch' % tag
    assert (after['last_scan_by_count'], after['last_scan_cb'], after['last_scan_prod']) == KERNEL[route], (tag, after)
    assert after['n_sorted_scans'] == before['n_sorted_scans'] + (1 if route == 'sorted' else 0), tag
    assert after['n_valid_launches'] == before['n_valid_launches'], tag


def took_split(before, after, tag):
    assert after['n_valid_launches'] == before['n_valid_launches'] + 1, '%s: no validity pass' % tag
    assert after['n_scan_launches'] == before['n_scan_launches'], tag


def reach(key, what):
    REACHED.setdefault(key, [])
    if what not in REACHED[key]:
        REACHED[key].append(what)


# ---- 1. the split of a cell's strips over its waves -------------------------------------------------------------------------------

WAVES = (0, 1, 2, 3, 5, 8, 13, 24, 64)                      # scan_waves_per_cu: 0 = the planner's own choice
LONG = (16 * 1024, 16 * 1024)                               # item lists that scan_chunk cuts into many groups: few blocks per group


@pytest.mark.parametrize('route', list(ROUTES) + ['split'])
def test_strip_split(route):
    c = sg.five_tile_case('upto12' if route == 'split' else 'poisson')
    strips = 5 * sg.TILE // (32 if route in ('bin order, 32-bin strips', 'compacted, bin order') else 64)
    key = 'last_valid_nslots' if route == 'split' else 'last_scan_nslots'
    ctx = context(c, **(SPLIT if route == 'split' else ROUTES[route]))
    seen = set()
    try:
        for points, chunk in (((97, 33), 0), (LONG, 1)):
            ctx.set_param('scan_chunk', chunk)
            for w in WAVES:
                ctx.set_param('scan_waves_per_cu', w)
                tag = 'strip split %s waves_per_cu=%d points=%s' % (route, w, points)
                _, before, after = run(ctx, c, 'strip split, ' + route, tag, points)
                took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
                nslots = after[key]
                assert nslots % 4 == 0 and 4 <= nslots <= strips, (tag, nslots)
                seen.add(nslots)
                if w:
                    reach('nslots, ' + route, nslots)
        ctx.set_param('scan_waves_per_cu', 0)
        classes = {'4': 4 in seen, '8': 8 in seen, 'strips / 4 waves each': strips in seen,
                   'between, not dividing the strips': any(8 < n < strips and strips % n for n in seen)}
        missing = [k for k, v in classes.items() if not v]
        assert not missing, '%s: no request reached nslots %s (reached %s)' % (route, missing, sorted(seen))
    finally:
        ctx.close()


# ---- 2. the block -> (group, slot) mappings of k_scan_sorted -----------------------------------------------------------------------

WIDE = (0, 1, 2, 3, 5, 64)


def test_block_mapping():
    """Group counts 1, 2, 7, 8, 9 from cells x chunks, under scan_xcd 0, 1, 2 and forced splits: the block counts reached are
    recorded mod 8 (the grid is rounded up to 8; under scan_xcd = 2 the groups are) and must include 0, 1, 4 and 7."""
    c = sg.five_tile_case('poisson')
    ctx = context(c, **ROUTES['sorted'])
    groups_seen, mod8 = set(), set()
    try:
        # (points per cell, scan_chunk): one and two cells uncut; long lists cut into chunks of 16 items or more
        layouts = [((97,), 0, WIDE), ((97, 33), 0, WIDE)] + [((16 * k,), 1, WIDE) for k in (16 * 7, 16 * 8, 16 * 9, 16 * 7 + 5)]
        layouts += [((16 * 64, 16 * 64), 1, WIDE)]
        # many chunked groups of one block each (nslots = 4 under the smallest forced split): 63, 65, 127 and 129 groups are 7 and 1
        # blocks mod 8, 68 and 132 are 4 -- where the lists are cut into chunks of 16 items, as on a chip of some 250 CUs; the
        # short list of requests is tried, the residues reached are recorded
        layouts += [((16 * 16 * g,), 1, (1,)) for g in (63, 65, 68, 127, 129, 132)]
        for points, chunk, waves in layouts:
            ctx.set_param('scan_chunk', chunk)
            for w in waves:
                ctx.set_param('scan_waves_per_cu', w)
                out = {}
                for xcd in (0, 1, 2):
                    ctx.set_param('scan_xcd', xcd)
                    tag = 'mapping points=%s chunk=%d waves_per_cu=%d scan_xcd=%d' % (points, chunk, w, xcd)
                    out[xcd], before, after = run(ctx, c, 'block mapping', tag, points)
                    took('sorted', before, after, tag)
                g, blocks = after['last_scan_groups'], after['last_scan_groups'] * after['last_scan_nslots'] // 4
                groups_seen.add(g)
                mod8.add(blocks % 8)
                if g % 8:
                    reach('scan_xcd = 2, groups not a multiple of 8', g)
                if after['last_scan_nslots'] == 4:
                    reach('one block per group, groups', g)
                # the mapping moves blocks, not arithmetic: a wave owns its strips and partial slots whatever block it is
                assert np.array_equal(out[0], out[1], equal_nan=True) and np.array_equal(out[0], out[2], equal_nan=True), tag
        REACHED['group counts'] = sorted(groups_seen)
        REACHED['blocks mod 8'] = sorted(mod8)
        assert {1, 2} <= groups_seen and any(g % 8 == 7 for g in groups_seen) and any(g % 8 == 1 and g > 1 for g in groups_seen) \
            and any(g % 8 == 0 for g in groups_seen), 'group counts reached: %s' % sorted(groups_seen)
        # the grid is rounded up to 8 blocks: a whole grid, one block more, half a grid, one block fewer
        assert {0, 1, 4, 7} <= mod8, 'blocks mod 8 reached: %s' % sorted(mod8)
    finally:
        ctx.set_param('scan_xcd', 1)
        ctx.close()


# ---- 3. item lists ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', list(ROUTES) + ['split'])
def test_item_lists(route):
    """Every per-cell point count of the table in the lower cell beside 65 points in the upper one (dense data take the scan from
    two items per cell on average), uncut and -- with lists long enough -- cut into chunks; two datasets of one cell as two groups."""
    c = sg.stream_case(4, 'upto12') if route == 'split' else sg.bins_case(1023)
    ctx = context(c, **(SPLIT if route == 'split' else ROUTES[route]))
    try:
        for chunk in (0, 1):
            ctx.set_param('scan_chunk', chunk)
            for n in sg.CELL_POINTS:
                for points in ((n, 65), (65, n)):
                    tag = 'items %s points=%s chunk=%d' % (route, points, chunk)
                    _, before, after = run(ctx, c, 'item lists, ' + route, tag, points, seed=n)
                    took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
                    if not chunk:
                        assert after['last_scan_groups'] == 2 and after['last_scan_max_items'] == -(-max(points) // 16), (tag, after)
        # lists that chunk_groups cuts: more groups than (cell, dataset) pairs, every chunk a multiple of four items
        ctx.set_param('scan_chunk', 1)
        for points in ((16 * 200 + 1, 16 * 37 + 3), (16 * 1024 + 1,)):
            tag = 'items %s points=%s cut' % (route, points)
            _, before, after = run(ctx, c, 'item lists, ' + route, tag, points)
            took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
            assert after['last_scan_groups'] > len(points) and after['last_scan_max_items'] % 4 == 0 and after['last_scan_max_items'] >= 16, (tag, after)
            reach('chunked groups, ' + route, '%d groups of <= %d items' % (after['last_scan_groups'], after['last_scan_max_items']))
    finally:
        ctx.close()


@pytest.mark.parametrize('sparse', [2, 0])
def test_two_datasets_of_one_cell_are_two_groups(sparse):
    c = sg.two_dataset_case()
    ctx = context(c, sparse=sparse, scan_chunk=0)
    try:
        for points, ds in (((33, 17, 49), (0, 0, 1)), ((97, 1, 15, 16), (0, 1, 1, 0))):
            tag = 'two datasets sparse=%d points=%s datasets=%s' % (sparse, points, ds)
            _, before, after = run(ctx, c, 'two datasets', tag, points, ds_of_cell=ds)
            assert after['n_scan_launches'] + after['n_valid_launches'] > before['n_scan_launches'] + before['n_valid_launches'], tag
            assert after['last_scan_groups'] == len(points), (tag, after)
    finally:
        ctx.close()


@pytest.mark.parametrize('B', sg.BINS)
@pytest.mark.parametrize('route', list(ROUTES) + ['split'])
def test_bins(route, B):
    """Every bin count of the table on every route: 64 and 65 (the other side of the count-sorted copy's refusal), 1, 2 and 5 tiles
    whose last tile is full, holds one bin or 511 (the padding behind the rows, the strip holding the last bin)."""
    c = sg.bins_case(B, 'upto12' if route == 'split' else 'poisson')
    ctx = context(c, scan_chunk=0, **(SPLIT if route == 'split' else ROUTES[route]))
    try:
        for points in ((17, 33), (97, 65)):
            tag = 'bins %d %s points=%s' % (B, route, points)
            _, before, after = run(ctx, c, 'bins, ' + route, tag, points, seed=B)
            took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
            assert after['last_scan_groups'] == 2 and after['last_scan_max_items'] == -(-max(points) // 16), (tag, after)
            reach('bins, ' + route, B)
    finally:
        ctx.close()


@pytest.mark.parametrize('kind', list(sg.INVALID_COUNTS))
def test_invalid_counts(kind):
    """One bin with a negative, a non-integer or a nan count: -inf (nan) at EVERY point, on every route -- the strip holding that
    bin is worked bin by bin in count order, the product form must not take its block."""
    for route in list(ROUTES) + ['split']:
        c = sg.invalid_counts_case(kind, 'upto12' if route == 'split' else 'poisson')
        ctx = context(c, **(SPLIT if route == 'split' else ROUTES[route]))
        try:
            for points in ((17, 33), (97, 65)):
                tag = '%s %s points=%s' % (kind, route, points)
                got, before, after = run(ctx, c, 'invalid counts', tag, points)
                took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
                assert np.isnan(got).all() if kind == 'nan count' else (got == -np.inf).all(), tag
        finally:
            ctx.close()


# ---- 4. strip classes of k_scan_sorted --------------------------------------------------------------------------------------------

def strip_class_cases():
    out = [('dense %s' % k, lambda k=k: sg.dense_case(k)) for k in sg.DENSE_DATA] + [('one count, no padding', lambda: sg.dense_case('one_count', 2560))]
    out += [('rates x 1e45', lambda: sg.scaled_case(1e45)), ('rates x 1e-135', lambda: sg.scaled_case(1e-135)),
            ('subnormal row entry', sg.subnormal_row_case), ('exact zero expectation', sg.zero_expectation_case),
            ('negative dense', sg.negative_case)]
    return out


@pytest.mark.parametrize('name,make', strip_class_cases(), ids=[n for n, _ in strip_class_cases()])
def test_strip_classes(name, make):
    c = make()
    ctx = context(c, **ROUTES['sorted'])
    try:
        for share in (1, 0):
            ctx.set_param('scan_share_slow', share)
            for w in (0, 64):
                ctx.set_param('scan_waves_per_cu', w)
                # (17, 33): fewer items than waves; (97, 65): several quads, a ragged one
                for points in ((17, 33)[:c.n_cells], (97, 65)[:c.n_cells], (337,)):
                    if len(points) == 1 and points[0] < 32:
                        points = (33,)
                    tag = 'strip classes %s share_slow=%d waves_per_cu=%d points=%s' % (name, share, w, points)
                    got, before, after = run(ctx, c, 'strip classes', tag, points)
                    took('sorted', before, after, tag)
                    if name == 'exact zero expectation':
                        assert (got == -np.inf).any() and np.isfinite(got).any(), tag
                    if name == 'negative dense':
                        assert np.isnan(got).any() and np.isfinite(got).any(), tag
    finally:
        ctx.close()


# ---- every stream-group class -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('NS', list(sg.STREAMS))
def test_stream_groups(NS):
    """KG = 1 .. 8 with and without padding streams: count order (dense and compacted), bin order, the split scan's validity pass."""
    dense, sparse = sg.stream_case(NS), sg.stream_case(NS, 'upto12')
    points = (49, 33, 17, 65)[:dense.n_cells] if dense.n_cells > 1 else (81,)
    for c, route in ((dense, 'sorted'), (dense, 'bin order, 32-bin strips'), (dense, 'bin order, 64-bin strips'),
                     (sparse, 'compacted, count order'), (sparse, 'compacted, bin order'), (sparse, 'split')):
        ctx = context(c, **(SPLIT if route == 'split' else ROUTES[route]))
        try:
            tag = 'streams NS=%d %s' % (NS, route)
            _, before, after = run(ctx, c, 'stream groups, ' + route, tag, points)
            took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
        finally:
            ctx.close()


# ---- 5. the bin-order kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', sg.DENSE_DATA)
@pytest.mark.parametrize('route', ['bin order, 32-bin strips', 'bin order, 64-bin strips'])
def test_bin_order_kernel_on_dense_rows(route, kind):
    c = sg.dense_case(kind)
    ctx = context(c, **ROUTES[route])
    try:
        for points in ((17, 33), (97, 65)):
            tag = '%s dense %s points=%s' % (route, kind, points)
            _, before, after = run(ctx, c, route, tag, points)
            took(route, before, after, tag)
    finally:
        ctx.close()


def test_bin_order_kernel_takes_two_datasets():
    """T = 2: no count-sorted copy (it holds one dataset), so dense data go to k_scan_mfma<2> with scan_pow left on."""
    c = sg.case('two dense datasets', 1023, T=2)
    ctx = context(c, sparse=0)
    try:
        tag = 'bin order, T = 2'
        _, before, after = run(ctx, c, 'bin order, 32-bin strips', tag, (33, 17, 49, 65), ds_of_cell=(0, 0, 1, 1))
        took('bin order, 32-bin strips', before, after, tag)
    finally:
        ctx.close()


@pytest.mark.parametrize('nnz', sg.SPARSE_NNZ)
@pytest.mark.parametrize('kind', sg.SPARSE_DATA)
def test_product_form_on_compacted_rows(kind, nnz):
    c = sg.sparse_case(kind, nnz)
    for route in ('compacted, bin order', 'compacted, count order'):
        ctx = context(c, **ROUTES[route])
        try:
            assert ctx.get_param('compact_sorted') == (1 if route == 'compacted, count order' else 0)
            for points in ((17, 33), (97, 65)):
                tag = '%s %s nnz=%d points=%s' % (route, kind, nnz, points)
                _, before, after = run(ctx, c, route, tag, points)
                took(route, before, after, tag)
        finally:
            ctx.close()


def test_product_form_with_subnormal_intermediates():
    """The model of test_scan_sorted_gpu.py::test_sparse_product_form_with_subnormal_intermediates (expectations of ~1e-162 beside
    ~1e3 in bins of counts 1 and 2: a pair product of the small ones is subnormal), every point held to the bound."""
    from blueice_amd.device import DeviceContext
    rng = np.random.default_rng(5)
    B, S = 8192, 2
    anchor_z = [np.array([0.0, 1.0])]
    ps = rng.uniform(0.5, 1.5, size=(2, S, B))
    hot = np.arange(0, 512)
    ps[:, :, hot[0::2]] *= 1e-165
    ps[:, :, hot[1::2]] *= 1e+3
    model = dict(anchor_z=anchor_z, ps=ps, mus=np.full((2, S), 1e3), n_model=None)
    counts = np.zeros(B)
    counts[hot] = rng.integers(1, 3, size=len(hot))
    pz, pr = rng.uniform(0.03, 0.97, (19, 1)), rng.uniform(0.5, 1.5, (19, S))
    oracle = [do.derivatives(model, pz[i], pr[i], counts=counts, hessian=False) for i in range(19)]
    want, cond = np.array([o['ll'] for o in oracle]), np.array([o['ll_cond'] for o in oracle])
    idx = np.random.default_rng(6).permutation(np.arange(337) % 19)
    for pow_on in (0, 1):
        ctx = DeviceContext(0)
        try:
            for k, v in dict(sparse=2, scan_pow=pow_on, device_plan_min=1, scan_min_items=1).items():
                ctx.set_param(k, v)
            ctx.upload_model(anchor_z, ps, model['mus'])
            ctx.upload_counts(counts)
            before = counters(ctx)
            got, st = ctx.eval(pz[idx], pr[idx])
            after = counters(ctx)
            tag = 'subnormal intermediates scan_pow=%d' % pow_on
            assert (st == 0).all() and after['n_scan_launches'] == before['n_scan_launches'] + 1, tag
            assert after['last_scan_prod'] == 1 - pow_on and after['last_scan_by_count'] == pow_on, (tag, after)
            worst = do.check_entries(got, want[idx], cond[idx], do.C_POISSON, tag)
            WORST['subnormal intermediates'] = max(WORST.get('subnormal intermediates', 0.0), worst)
        finally:
            ctx.close()


# ---- 6. the split scan ------------------------------------------------------------------------------------------------------------

def test_split_scan_with_negative_expectations():
    """A source allowed negative: nan exactly at the prototypes with a certainly negative expectation (found by k_scan_valid in
    an empty bin or by the non-empty-bin pass), the bound at the others; odd and even item counts per group (the kernel alternates
    two register sets per item pair); last_valid_nslots follows a forced scan_waves_per_cu."""
    c = sg.negative_case('upto12')
    ctx = context(c, **SPLIT)
    seen = set()
    try:
        assert ctx.get_param('split_ready') == 1
        for w in (0, 1, 3, 8, 64):
            ctx.set_param('scan_waves_per_cu', w)
            # (the last batch: lists that scan_chunk cuts into many groups -- with two groups every forced value asks for more
            #  blocks per group than the strips give, and the split stays at its maximum)
            for points in ((16, 33), (17, 64), (97, 1), (65, 48), (16 * 512 + 1, 16 * 512)):
                tag = 'split, negative rates, waves_per_cu=%d points=%s' % (w, points)
                got, before, after = run(ctx, c, 'split scan', tag, points)
                took_split(before, after, tag)
                assert np.isnan(got).any() and np.isfinite(got).any(), tag
                assert after['last_valid_nslots'] % 4 == 0 and after['last_valid_nslots'] >= 4, tag
            if w:
                seen.add(after['last_valid_nslots'])
        REACHED['split scan, last_valid_nslots'] = sorted(seen)
        assert len(seen) >= 2, 'last_valid_nslots did not follow scan_waves_per_cu: %s' % sorted(seen)
    finally:
        ctx.close()


@pytest.mark.parametrize('kind', sg.SPARSE_DATA)
def test_split_scan_on_sparse_data(kind):
    for nnz in sg.SPARSE_NNZ:
        c = sg.sparse_case(kind, nnz)
        ctx = context(c, **SPLIT)
        try:
            for points in ((17, 33), (97, 64)):
                tag = 'split %s nnz=%d points=%s' % (kind, nnz, points)
                _, before, after = run(ctx, c, 'split scan', tag, points)
                took_split(before, after, tag)
        finally:
            ctx.close()


# ---- 7. fallbacks and changes of route --------------------------------------------------------------------------------------------

def test_fallbacks_take_no_scan_route():
    for c in sg.fallback_cases():
        ctx = context(c, sparse=0)
        try:
            points = (97, 65)[:c.n_cells] if c.n_cells > 1 else (97,)
            tag = 'fallback %s' % c.name
            got, before, after = run(ctx, c, 'fallbacks', tag, points)
            if c.name == 'bins 63':
                # (the count-sorted copy is refused: the batch falls back to the bin-order kernel k_scan_mfma<2>, never k_scan_sorted)
                took('bin order, 32-bin strips', before, after, tag)
            else:
                assert after['n_scan_launches'] == before['n_scan_launches'] and after['n_valid_launches'] == before['n_valid_launches'], tag
            if c.name == 'nan template entry':
                assert np.isnan(got).any() and np.isfinite(got).any(), tag
        finally:
            ctx.close()


def test_route_changes_within_one_context_keep_the_bits():
    """sorted -> bin order -> compacted -> split -> sorted in ONE context (data uploaded again where the route needs another copy):
    the first batch gives the same bits at the end."""
    dense, sparse = sg.bins_case(1023), sg.stream_case(4, 'upto12')
    points = (97, 33)
    ctx = context(dense, **ROUTES['sorted'])
    try:
        def step(c, route, **params):
            for k, v in params.items():
                ctx.set_param(k, v)
            if params:
                c.upload(ctx)
            tag = 'route change: %s' % route
            got, before, after = run(ctx, c, 'route changes', tag, points)
            took_split(before, after, tag) if route == 'split' else took(route, before, after, tag)
            return got

        first = step(dense, 'sorted')
        step(dense, 'bin order, 32-bin strips', scan_pow=0)
        step(sparse, 'compacted, bin order', sparse=2)
        step(sparse, 'compacted, count order', scan_pow=1)
        step(sparse, 'split', sparse=0)
        last = step(dense, 'sorted', sparse=0)
        assert np.array_equal(first, last), 'the sorted route gave other bits after other routes: %r' % (first - last)[:8]
    finally:
        ctx.close()
