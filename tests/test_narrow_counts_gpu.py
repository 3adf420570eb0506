"""The narrow copy of the event counts (one byte per bin beside the doubles, DESIGN.md "The counts format"): the dense
morph kernels that read it give the SAME BITS as the ones that read the doubles, they really read it where the data
allow it, and data that have no exact one-byte form -- or a batch that touches one such dataset -- keep the double path.

Every comparison here is np.array_equal on values and status words: u8 -> double is exact and nothing behind the load
changes, so no tolerance applies."""
import numpy as np
import pytest

from golden_util import case_names, load_case, rate_scale_of

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                 b.view(np.uint64) if b.dtype == np.float64 else b)


@pytest.fixture()
def ctx():
    from blueice_amd.device import DeviceContext
    c = DeviceContext(0)
    c.set_param('sparse', 0)                 # the dense kernels: every evaluation streams its counts row
    yield c
    c.close()


def upload_case(ctx, c, counts=None):
    bb = c['bb_source']
    ctx.upload_model(c['model']['anchor_z'], c['model']['ps'], c['model']['mus'],
                     n_model=c['model']['n_model'] if bb >= 0 else None, bb_source=bb)
    if c.get('allow_negative') is not None:
        ctx.set_allow_negative([1 if a else 0 for a in c['allow_negative']])
    ctx.upload_counts(c['counts'] if counts is None else counts)


def c2_shaped(bb_source=-1):
    """The headline's shape (4 sources, 5^3 anchors) at 20 x 17 x 13 = 4420 bins: not a multiple of the 512-bin tile."""
    from blueice_amd.synthetic import SyntheticModel
    return SyntheticModel(4, (5, 5, 5), (20, 17, 13), bb_source=bb_source)


def eval_all_shapes(ctx, z, r, dataset):
    """(values, status words) of the three call shapes: single points, one batched eval, a plan's run."""
    out = []
    for j in range(len(z)):
        out.append(ctx.eval(z[j], r[j], dataset=None if dataset is None else [dataset[j]]))
    out.append(ctx.eval(z, r, dataset=dataset))
    plan = ctx.plan(z, r, dataset=dataset)
    plan.run()
    out.append(plan.read())
    info = dict(plan_bytes=plan.bytes, streamed=ctx.get_param('last_streamed_bytes'))
    plan.close()
    return out, info


def both_ways(ctx, z, r, dataset=None):
    res = {}
    for on in (1, 0):
        ctx.set_param('narrow_counts', on)
        n0 = ctx.get_param('n_narrow_launches')
        res[on] = eval_all_shapes(ctx, z, r, dataset) + (ctx.get_param('n_narrow_launches') - n0,)
    ctx.set_param('narrow_counts', 1)
    for (v1, s1), (v0, s0) in zip(res[1][0], res[0][0]):
        assert same_bits(v1, v0), (v1, v0)
        assert np.array_equal(s1, s0)
    assert res[0][2] == 0 and res[0][1]['streamed'] == res[0][1]['plan_bytes']
    return res[1]


@pytest.mark.parametrize('name', case_names())
def test_golden_models_bit_identical(ctx, name):
    """Every golden model (weighted data, Beeston-Barlow, sources that may go negative among them): narrow_counts = 1 and 0
    give the same bits in all call shapes, whether or not the data have a narrow form."""
    c = load_case(name)
    upload_case(ctx, c)
    n = len(c['call_ll'])
    rs = np.array([rate_scale_of(c, j) for j in range(n)])
    both_ways(ctx, c['call_z'], rs)
    # the same model on whole-number data, which do have one: the narrow kernels run, same bits again
    rng = np.random.default_rng(11)
    counts = rng.poisson(3.0, int(np.prod(c['bins']))).astype(float)
    ctx.upload_counts(counts)
    assert ctx.get_param('narrow_ready') == 1
    vals, info, n_narrow = both_ways(ctx, c['call_z'], rs)
    if np.any(np.isfinite(vals[-1][0])):         # (some point was answered by a launch)
        assert n_narrow > 0


@pytest.mark.parametrize('bb', [-1, 1])
def test_headline_call_shape_streams_narrow_rows(ctx, bb):
    """One dataset per point, points in cells that share no anchor (bench.py's step), on the C2-shaped model, plain and
    Beeston-Barlow: same bits, and the plan really read one byte per bin: last_streamed_bytes = bytes - 7 Bp n_items."""
    m = c2_shaped(bb)
    m.upload(ctx)
    z, r = m.disjoint_cell_points(parity=0, seed=3)
    P = len(z)
    ctx.upload_counts(np.stack([m.counts(dense=True, dataset=i) for i in range(P)]))
    (vals, info, n_narrow) = both_ways(ctx, z, r, dataset=np.arange(P))
    assert bb >= 0 or np.all(np.isfinite(vals[-1][0]))
    Bp = ctx.get_param('padded_bins')
    assert Bp % ctx.get_param('tile_bins') == 0 and Bp > m.B
    # P distinct (cell, dataset) pairs = P work items
    assert info['streamed'] == info['plan_bytes'] - 7 * Bp * P
    assert n_narrow >= P + 2                     # P single calls, the batched eval, the plan


@pytest.mark.parametrize('odd', [256.0, 0.5, -1.0, np.nan, np.inf])
def test_fallback_for_data_without_a_narrow_form(ctx, odd):
    """One bin holding 256, 0.5, -1, nan or +inf: the dataset keeps the double path, bit for bit."""
    m = c2_shaped()
    m.upload(ctx)
    counts = m.counts(dense=True)
    counts[m.B // 3] = odd
    ctx.upload_counts(counts)
    z, r = m.random_points(5, seed=2)
    _, info, n_narrow = both_ways(ctx, z, r)
    assert n_narrow == 0
    assert info['streamed'] == info['plan_bytes']
    assert same_bits(ctx.download_counts(0), counts)


def test_mixed_batch_takes_the_double_path(ctx):
    """A launch over an eligible and an ineligible dataset reads doubles for both; a launch over the eligible one alone reads
    its narrow row."""
    m = c2_shaped()
    m.upload(ctx)
    good = m.counts(dense=True, dataset=0)
    weighted = m.counts(dense=True, dataset=1) * 0.5
    ctx.upload_counts(np.stack([good, weighted]))
    z, r = m.disjoint_cell_points(parity=1, seed=4)
    ds = np.arange(len(z)) % 2
    _, info, n_narrow = both_ways(ctx, z, r, dataset=ds)
    assert info['streamed'] == info['plan_bytes']
    assert n_narrow == (len(z) + 1) // 2          # only the single calls on dataset 0
    _, info, n_narrow = both_ways(ctx, z, r, dataset=np.zeros(len(z), dtype=np.int64))
    assert info['streamed'] == info['plan_bytes'] - 7 * ctx.get_param('padded_bins') * len(z)


def fresh_values(m, load, z, r, dataset=None):
    """The same evaluations in a new context that takes its data the same way (`load(ctx)`) and never reads a narrow row."""
    from blueice_amd.device import DeviceContext
    c = DeviceContext(0)
    try:
        c.set_param('sparse', 0)
        c.set_param('narrow_counts', 0)
        m.upload(c)
        load(c)
        return eval_all_shapes(c, z, r, dataset)[0]
    finally:
        c.close()


def assert_same_results(got, want):
    assert len(got) == len(want)
    for (v1, s1), (v0, s0) in zip(got, want):
        assert same_bits(v1, v0), (v1, v0)
        assert np.array_equal(s1, s0)


def test_no_stale_narrow_rows(ctx):
    """Every writer of the dense counts rebuilds the narrow copy: a second upload, an upload of data without a narrow form
    and back, toys made dense, and the event histogram all evaluate as a fresh context that holds the same data (and reads
    doubles only) does."""
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel.named('mini3')
    m.upload(ctx)
    z, r = m.random_points(4, seed=7)
    first = m.counts(dense=True, dataset=0)
    second = m.counts(dense=True, dataset=5)
    assert not np.array_equal(first, second)
    for counts, narrow in ((first, True), (second, True), (second * 1.5, False), (first, True)):
        ctx.upload_counts(counts)
        n0 = ctx.get_param('n_narrow_launches')
        assert_same_results(eval_all_shapes(ctx, z, r, None)[0], fresh_values(m, lambda c: c.upload_counts(counts), z, r))
        assert (ctx.get_param('n_narrow_launches') > n0) == narrow

    # device-generated toys exist as lists only (no narrow copy); made dense, the copy is rebuilt from them
    zt, rt = m.default_point()

    def toys(c):
        c.generate_toys(zt, rt, T=3, seed=9)
        c.counts_to_dense()

    ctx.generate_toys(zt, rt, T=3, seed=9)
    assert ctx.get_param('narrow_ready') == 0
    ctx.counts_to_dense()
    assert ctx.get_param('narrow_ready') == 1
    drawn = np.stack([ctx.download_counts(t) for t in range(3)])
    assert drawn.sum() > 0 and not np.array_equal(drawn[0], first) and not np.array_equal(drawn[0], drawn[1])
    ds = np.arange(len(z)) % 3
    n0 = ctx.get_param('n_narrow_launches')
    assert_same_results(eval_all_shapes(ctx, z, r, ds)[0], fresh_values(m, toys, z, r, ds))
    assert ctx.get_param('n_narrow_launches') >= n0 + len(z) + 2

    # the event histogram: dataset 0 binned on the device
    edges = [np.arange(b + 1, dtype=float) for b in m.bins]
    rng = np.random.default_rng(4)
    cols = [rng.uniform(0, b, 3000) for b in m.bins]

    def events(c):
        c.set_analysis_space(edges)
        c.upload_events(*cols)

    events(ctx)
    hist = ctx.download_counts(0)
    assert hist.sum() == 3000 and same_bits(hist, np.histogramdd(np.stack(cols, 1), bins=edges)[0].ravel())
    n0 = ctx.get_param('n_narrow_launches')
    assert_same_results(eval_all_shapes(ctx, z, r, None)[0], fresh_values(m, events, z, r))
    assert ctx.get_param('n_narrow_launches') > n0


def test_boundaries_and_download(ctx):
    """255 -- the largest value with a narrow form -- in the LAST real bin of rows that end inside a tile: the padding
    behind it reads as 0 (the result equals the double path's, which sees the zero padding of the doubles), and
    download_counts returns the uploaded doubles exactly."""
    m = c2_shaped()
    m.upload(ctx)
    assert m.B % ctx.get_param('tile_bins') != 0
    counts = m.counts(dense=True)
    counts[-1] = 255.0
    counts[0] = 255.0
    counts[1] = 0.0
    ctx.upload_counts(counts)
    z, r = m.random_points(6, seed=5)
    _, info, n_narrow = both_ways(ctx, z, r)
    assert n_narrow > 0 and info['streamed'] < info['plan_bytes']
    assert same_bits(ctx.download_counts(0), counts)
    # one more than 255 in that bin: no narrow form any more
    counts[-1] = 256.0
    ctx.upload_counts(counts)
    _, info, n_narrow = both_ways(ctx, z, r)
    assert n_narrow == 0 and info['streamed'] == info['plan_bytes']
    assert same_bits(ctx.download_counts(0), counts)
    # minus zero compares equal to 0 but is not the same double: it keeps the double path, too
    counts[-1] = -0.0
    ctx.upload_counts(counts)
    _, info, n_narrow = both_ways(ctx, z, r)
    assert n_narrow == 0
    assert same_bits(ctx.download_counts(0), counts)
