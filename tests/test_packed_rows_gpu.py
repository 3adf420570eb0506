"""The packed shadow of the template rows (7 bytes per value beside the doubles): it holds the uploaded
bits exactly, only models every tile of which has a packed form get one, the dense value kernels that read it give the SAME
BITS as the ones that read the doubles, every upload replaces it, and the byte accounting says what was saved.

Every comparison is np.array_equal on the uint64 view of the values and on the status words: decoding returns the stored
doubles and nothing behind the load changes, so no tolerance applies.  The shapes are small on purpose: one shape axis with
three anchors, two sources, 700 bins = two 512-bin tiles, the second one partial (188 bins and zero padding), which puts a
chunk seam and a ragged row end into every case."""
import numpy as np
import pytest

import value_geometry_cases as vg

pytestmark = pytest.mark.gpu

A, S, B = 3, 2, 700
TILE = 512
BIG = 1 << 40
ANCHOR_Z = [np.array([-1.0, 0.0, 1.0])]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


def from_parts(exponent, mantissa):
    return ((np.asarray(exponent, dtype=np.uint64) << np.uint64(52)) | np.asarray(mantissa, dtype=np.uint64)).view(np.float64)


@pytest.fixture()
def ctx():
    from blueice_amd.device import DeviceContext
    c = DeviceContext(0)
    c.set_param('sparse', 0)                     # the dense kernels
    c.set_param('device_plan_min', BIG)          # every batch planned on the host: max_group decides the group classes
    yield c
    c.close()


def pmf_tensor(seed=3):
    """[A, S, B] of strictly positive PMFs: (U[0, 1) + 0.05) / sum, at most 6 binades wide -- a model with a packed form."""
    rng = np.random.default_rng(seed)
    p = rng.random((A, S, B)) + 0.05
    return p / p.sum(axis=2, keepdims=True)


def mus():
    return np.array([[1000.0 * (s + 1) * (1 + 0.02 * a) for s in range(S)] for a in range(A)])


def counts(T=2, seed=5):
    return np.random.default_rng(seed).poisson(4.0, (T, B)).astype(float)


def upload(ctx, ps, data=None):
    ctx.upload_model(ANCHOR_Z, ps, mus())
    ctx.upload_counts(counts() if data is None else data)


def points(n, seed=9, cell=None):
    """n points (z [n, 1], r [n, S]); cell 0 / 1: all of them inside that grid cell."""
    rng = np.random.default_rng(seed)
    lo, hi = (-1.0, 1.0) if cell is None else ((-1.0, -0.01) if cell == 0 else (0.01, 1.0))
    return rng.uniform(lo, hi, (n, 1)), rng.uniform(0.6, 1.4, (n, S))


def eval_all_shapes(ctx, z, r, dataset=None):
    """(values, status words) of the three call shapes: single points, one batched eval, a plan's run."""
    out = []
    for j in range(len(z)):
        out.append(ctx.eval(z[j], r[j], dataset=None if dataset is None else [dataset[j]]))
    out.append(ctx.eval(z, r, dataset=dataset))
    plan = ctx.plan(z, r, dataset=dataset)
    plan.run()
    out.append(plan.read())
    info = dict(plan_bytes=plan.bytes, streamed=ctx.get_param('last_streamed_bytes'), saved=ctx.get_param('last_packed_saved_bytes'))
    plan.close()
    return out, info


def both_ways(ctx, z, r, dataset=None):
    """The evaluations with packed_rows = 1 and 0: same bits; -> (results, info, launches that read the shadow)."""
    res = {}
    for on in (1, 0):
        ctx.set_param('packed_rows', on)
        n0 = ctx.get_param('n_packed_launches')
        res[on] = eval_all_shapes(ctx, z, r, dataset) + (ctx.get_param('n_packed_launches') - n0,)
    ctx.set_param('packed_rows', 1)
    for (v1, s1), (v0, s0) in zip(res[1][0], res[0][0]):
        assert same_bits(v1, v0), (v1, v0)
        assert np.array_equal(s1, s0)
    assert res[0][2] == 0 and res[0][1]['saved'] == 0
    assert res[1][1]['plan_bytes'] == res[0][1]['plan_bytes'] and res[1][1]['streamed'] == res[0][1]['streamed']
    return res[1]


# ---- round trip ---------------------------------------------------------------------------------------------------------------

def test_round_trip_of_random_bit_patterns(ctx):
    """Random bit patterns inside the set that has a packed form -- per (row, tile) a window of 15 exponents anywhere in the
    normal range, random mantissas -- with the corner patterns planted: bi_unpack_rows returns the uploaded bits."""
    rng = np.random.default_rng(17)
    rows = A * S
    n_tiles = (B + TILE - 1) // TILE
    e = np.empty((rows, B), dtype=np.uint64)
    emin = rng.integers(1, 2046 - 14 + 1, (rows, n_tiles))
    emin[0, 0], emin[1, 0] = 1, 2046 - 14                       # the two ends of the normal range
    for t in range(n_tiles):
        w = slice(t * TILE, min(B, (t + 1) * TILE))
        e[:, w] = emin[:, t:t + 1] + rng.integers(0, 15, (rows, w.stop - w.start))
    m = rng.integers(0, 1 << 52, (rows, B), dtype=np.uint64)
    m[0, 3] = (1 << 52) - 1                                     # mantissa all ones
    m[0, 4] = 0                                                 # mantissa all zeros
    m[0, 5] = (m[0, 5] & ~np.uint64(0xFFFFFFFF)) | np.uint64(0xFFFFFFFF)    # low word all ones
    m[0, 6] = np.uint64(0xF) << np.uint64(48)                   # the top nibble alone
    m[0, 7] = np.uint64(0xFFFF) << np.uint64(32)                # the middle half-word alone
    for r_ in range(rows):                                      # exponents at both ends of the window, side by side, in both tiles
        for t in range(n_tiles):
            e[r_, t * TILE + 8] = emin[r_, t]
            e[r_, t * TILE + 9] = emin[r_, t] + 14
            e[r_, t * TILE + 10] = emin[r_, t]
    ps = from_parts(e, m)
    ps[2, 20:30:2] = 0.0                                        # +0.0 next to non-zeros, even and odd bins of a lane's pair
    ps[2, 41] = 0.0
    ps[3, 0] = 0.0
    ps[3, B - 1] = 0.0
    ps[4, TILE:] = 0.0                                          # one tile of zeros (the second tile of row 4)
    ps[5, :TILE] = 0.0                                          # ... and a first tile of zeros
    assert np.isfinite(ps).all() and (ps >= 0).all()
    ctx.upload_model(ANCHOR_Z, ps.reshape(A, S, B), mus())
    assert ctx.get_param('packed_rows_valid') == 1
    Bp = ctx.get_param('padded_bins')
    assert Bp == n_tiles * TILE
    out = ctx.unpack_rows()
    assert out.shape == (rows, Bp)
    assert np.array_equal(bits(out[:, :B]), bits(ps))
    assert np.array_equal(bits(out[:, B:]), np.zeros((rows, Bp - B), dtype=np.uint64))       # the padding bins are +0.0


# ---- eligibility ----------------------------------------------------------------------------------------------------------------

def windowed_tensor(width, seed=21):
    """The PMF tensor with the exponents of row 3's second tile forced into a window of exactly `width` values (both ends
    present, zeros in between left alone)."""
    ps = pmf_tensor(seed)
    row = ps.reshape(A * S, B)[3]
    u = bits(row[TILE:]).copy()
    man = u & np.uint64((1 << 52) - 1)
    e0 = 1000
    ex = np.uint64(e0) + (np.arange(len(u)) % width).astype(np.uint64)
    ex[0], ex[1] = e0, e0 + width - 1
    row[TILE:] = ((ex << np.uint64(52)) | man).view(np.float64)
    row[TILE + 5] = 0.0
    return ps


def test_exponent_window_of_15_is_eligible_and_16_is_not(ctx):
    z, r = points(4)
    upload(ctx, windowed_tensor(15))
    assert ctx.get_param('packed_rows_valid') == 1
    _, _, n_packed = both_ways(ctx, z, r)
    assert n_packed > 0
    assert np.array_equal(bits(ctx.unpack_rows()[:, :B]), bits(windowed_tensor(15).reshape(A * S, B)))
    upload(ctx, windowed_tensor(16))
    assert ctx.get_param('packed_rows_valid') == 0
    _, info, n_packed = both_ways(ctx, z, r)
    assert n_packed == 0 and info['saved'] == 0


@pytest.mark.parametrize('odd', [-0.0, -1e-6, 5e-324, 2.2250738585072009e-308, np.inf, np.nan], ids=['minus_zero', 'negative', 'smallest_subnormal',
                                                                                                    'largest_subnormal', 'inf', 'nan'])
@pytest.mark.parametrize('where', [(0, 1), (5, B - 1)], ids=['first_tile', 'last_bin'])
def test_values_without_a_packed_form_keep_the_double_path(ctx, odd, where):
    """One value that is -0.0, negative, subnormal, inf or nan: the model has no shadow, no launch reads one, and the results
    are those of packed_rows = 0, bit for bit."""
    ps = pmf_tensor()
    ps.reshape(A * S, B)[where] = odd
    upload(ctx, ps)
    assert ctx.get_param('packed_rows_valid') == 0
    z, r = points(4)
    _, info, n_packed = both_ways(ctx, z, r)
    assert n_packed == 0 and info['saved'] == 0
    with pytest.raises(Exception):
        ctx.unpack_rows()


def test_parameter_off_builds_no_shadow(ctx):
    ctx.set_param('packed_rows', 0)
    upload(ctx, pmf_tensor())
    assert ctx.get_param('packed_rows_valid') == 0
    ctx.set_param('packed_rows', 1)
    z, r = points(3)
    n0 = ctx.get_param('n_packed_launches')
    eval_all_shapes(ctx, z, r)
    assert ctx.get_param('n_packed_launches') == n0               # (read at upload: the next upload builds one)
    upload(ctx, pmf_tensor())
    assert ctx.get_param('packed_rows_valid') == 1


# ---- same bits ------------------------------------------------------------------------------------------------------------------

SETTINGS = [dict(), dict(max_group=1), dict(max_group=4), dict(max_group=16), dict(nt_loads=0), dict(nt_loads=1), dict(nt_loads=1, max_group=1),
            dict(narrow_counts=0), dict(narrow_counts=0, nt_loads=1, max_group=1), dict(narrow_counts=0, max_group=4, nt_loads=0),
            dict(single_kernel=0), dict(single_kernel=0, narrow_counts=0), dict(fuse_max_blocks=0), dict(fuse_finish=0),
            dict(keep_rows=3), dict(keep_rows=3, narrow_counts=0), dict(keep_rows=0), dict(tile_chunks=1)]
DEFAULTS = dict(max_group=16, nt_loads=2, narrow_counts=1, single_kernel=1, fuse_max_blocks=1 << 20, fuse_finish=1, keep_rows=-1, tile_chunks=8)


@pytest.mark.parametrize('over', SETTINGS, ids=[','.join('%s=%s' % kv for kv in s.items()) or 'defaults' for s in SETTINGS])
def test_same_bits_as_the_double_rows(ctx, over):
    """G = 1 and larger group classes, both load policies (nt_loads 1 / 0, and 2: a batch over two cells that share an anchor,
    a batch inside one cell), kept rows (the second and third single call in a cell), narrow and double counts, the single-point
    kernel with and without its in-launch finish, and the fallback through k_morph_reduce<1>."""
    upload(ctx, pmf_tensor())
    assert ctx.get_param('packed_rows_valid') == 1 and ctx.get_param('narrow_ready') == 1
    for k, v in dict(DEFAULTS, **over).items():
        ctx.set_param(k, v)
    # seven points of the lower cell (groups of up to max_group), then two of the upper one
    z0, r0 = points(7, seed=1, cell=0)
    z1, r1 = points(2, seed=2, cell=1)
    z, r = np.concatenate([z0, z1]), np.concatenate([r0, r1])
    ds = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1])
    _, info, n_packed = both_ways(ctx, z, r, dataset=ds)
    assert n_packed >= len(z) + 2                                  # the single calls, the batched eval, the plan
    assert info['saved'] > 0
    # one cell only: no anchor shared between items of different cells
    _, _, n_packed = both_ways(ctx, z0, r0, dataset=ds[:7])
    assert n_packed >= len(z0) + 2


def test_same_bits_across_launch_geometries(ctx):
    """A batch whose points fall into several group classes (17 points of one cell, 2 of the other, 2 on a second dataset: the
    pool of the group-class test of tests/test_value_geometry_gpu.py on its 1025-bin model), so that one run makes several
    launches of different shapes; and the 129-tile model, whose tile walk is chunked."""
    c = vg.group_case()
    rng = np.random.default_rng(31)
    g = c.m.anchor_z[0]
    z = np.concatenate([rng.uniform(g[0], g[1] - 0.01, 17), rng.uniform(g[1], g[2], 2), rng.uniform(g[0], g[1] - 0.01, 2)])[:, None]
    r = rng.uniform(0.6, 1.4, (21, c.m.S))
    ds = np.array([0] * 19 + [1] * 2)
    c.upload(ctx)
    assert ctx.get_param('packed_rows_valid') == 1
    for max_group in (1, 2, 4, 8, 16):
        ctx.set_param('max_group', max_group)
        _, info, n_packed = both_ways(ctx, z, r, dataset=ds)
        assert n_packed >= len(z) + 2 and info['saved'] > 0
    c = vg.tile_case(129, vg.TILE - 1)
    c.upload(ctx)
    assert ctx.get_param('packed_rows_valid') == 1
    zs, rs = vg.standard_points(c)
    for over in (dict(tile_chunks=2, max_group=16), dict(tile_chunks=1, max_group=1, blocks_per_cu=1)):
        for k, v in over.items():
            ctx.set_param(k, v)
        _, _, n_packed = both_ways(ctx, zs, rs)
        assert n_packed >= len(zs) + 2


# ---- invalidation -----------------------------------------------------------------------------------------------------------------

def fresh_values(ps, z, r, data=None, load=None):
    """The same evaluations in a new context that never builds or reads a shadow."""
    from blueice_amd.device import DeviceContext
    c = DeviceContext(0)
    try:
        c.set_param('sparse', 0)
        c.set_param('device_plan_min', BIG)
        c.set_param('packed_rows', 0)
        if load is not None:
            load(c)
        else:
            upload(c, ps, data)
        return eval_all_shapes(c, z, r)[0]
    finally:
        c.close()


def assert_same_results(got, want):
    assert len(got) == len(want)
    for (v1, s1), (v0, s0) in zip(got, want):
        assert same_bits(v1, v0), (v1, v0)
        assert np.array_equal(s1, s0)


def test_every_upload_replaces_the_shadow(ctx):
    """Model A, then model B (other values) into the same context by each upload route: the results are B's, and the shadow
    holds B's bits; then a model without a packed form and back."""
    z, r = points(5, seed=4)
    a, b = pmf_tensor(1), pmf_tensor(2)
    assert not np.array_equal(a, b)
    upload(ctx, a)
    n0 = ctx.get_param('n_packed_launches')
    assert_same_results(eval_all_shapes(ctx, z, r)[0], fresh_values(a, z, r))
    assert ctx.get_param('n_packed_launches') > n0
    want_b = fresh_values(b, z, r)
    # the whole-tensor upload
    upload(ctx, b)
    assert ctx.get_param('packed_rows_valid') == 1
    assert np.array_equal(bits(ctx.unpack_rows()[:, :B]), bits(b.reshape(A * S, B)))
    n0 = ctx.get_param('n_packed_launches')
    assert_same_results(eval_all_shapes(ctx, z, r)[0], want_b)
    assert ctx.get_param('n_packed_launches') > n0
    # back to A, anchor by anchor (begin_model / set_anchor / end_model)
    ctx.begin_model(ANCHOR_Z, S, B)
    assert ctx.get_param('packed_rows_valid') == 0               # gone with the first step of the new upload
    for i in range(A):
        ctx.set_anchor(i, a[i], mus()[i])
    ctx.end_model()
    ctx.upload_counts(counts())
    assert ctx.get_param('packed_rows_valid') == 1
    assert np.array_equal(bits(ctx.unpack_rows()[:, :B]), bits(a.reshape(A * S, B)))
    assert_same_results(eval_all_shapes(ctx, z, r)[0], fresh_values(a, z, r))
    # a model without a packed form, then B again
    bad = b.copy()
    bad[1, 1, 600] = -0.0
    upload(ctx, bad)
    assert ctx.get_param('packed_rows_valid') == 0
    n0 = ctx.get_param('n_packed_launches')
    assert_same_results(eval_all_shapes(ctx, z, r)[0], fresh_values(bad, z, r))
    assert ctx.get_param('n_packed_launches') == n0
    upload(ctx, b)
    assert_same_results(eval_all_shapes(ctx, z, r)[0], want_b)


def test_an_event_tensor_has_no_shadow(ctx):
    """bi_score_events fills the target context's tensor with pdf values at events and makes it unbinned: a context that held
    a binned model with a shadow has none afterwards, and evaluates as a fresh context scored the same way."""
    from blueice_amd.device import DeviceContext
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel(2, (3,), (40, 25))
    tp = DeviceContext(0)
    try:
        m.upload(tp)
        assert tp.get_param('packed_rows_valid') == 1           # the templates context keeps its own
        upload(ctx, pmf_tensor())
        assert ctx.get_param('packed_rows_valid') == 1
        rng = np.random.default_rng(8)
        edges = [np.arange(b + 1, dtype=float) for b in m.bins]
        cols = [rng.uniform(0, b, 900) for b in m.bins]

        def score(c):
            tp.score_events(c, 'piecewise', edges, cols)

        score(ctx)
        assert ctx.get_param('packed_rows_valid') == 0
        z, r = m.random_points(4, seed=3)
        n0 = ctx.get_param('n_packed_launches')
        got = eval_all_shapes(ctx, z, r)[0]
        assert ctx.get_param('n_packed_launches') == n0
        assert_same_results(got, fresh_values(None, z, r, load=score))
        assert tp.get_param('packed_rows_valid') == 1
    finally:
        tp.close()


# ---- accounting -------------------------------------------------------------------------------------------------------------------

def test_bytes_saved_by_a_plan(ctx):
    """bi_plan_bytes keeps its all-double definition; a plan's run saves one byte per value of every row an item streams:
    padded bins x rows per item (2 corners x S sources) x items.  last_streamed_bytes -- what the counts format saved -- is
    untouched by it."""
    upload(ctx, pmf_tensor())
    ctx.set_param('max_group', 1)                                # one work item per point
    z, r = points(6, seed=6)
    Bp = ctx.get_param('padded_bins')
    got = {}
    for on in (1, 0):
        ctx.set_param('packed_rows', on)
        plan = ctx.plan(z, r)
        plan.run()
        plan.read()
        got[on] = (plan.bytes, ctx.get_param('last_streamed_bytes'), ctx.get_param('last_packed_saved_bytes'))
        plan.close()
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1]
    assert got[0][2] == 0
    assert got[1][2] == Bp * (2 * S) * len(z)
    assert got[1][1] == got[1][0] - 7 * Bp * len(z)              # (the narrow counts, as before)
