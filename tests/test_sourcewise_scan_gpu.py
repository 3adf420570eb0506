"""Source-wise models on the matrix-core scan route (bi_eval_sourcewise_scan; k_sourcewise_scan_key / _cut / _groups / _fill in front
of k_scan_mfma<2, KG, MASK, 1> over the compacted rows of the non-empty-bin form).

Every finite ll is held to derivative_oracle.check_entries with C_POISSON = 256 against `derivatives(expand(model))`, the same
likelihood on the full tensor-product grid -- the bar tests/test_scan_geometry_gpu.py holds k_scan_mfma to.  Status words, -inf and
nan are exact.  The shapes are the smallest at which the planner can go wrong: groups of 1, 16, 17 and 33 points (one slot, a full
item, a full item and one slot, two full items and one slot) in three cell tuples and two datasets, a point exactly on an anchor and
one on the box edge, lists of no, five, 512, 513 and all bins."""
import time

import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_nonempty_oracle as no
import sourcewise_toy_cases as toy_cases
from derivative_oracle import C_POISSON, check_entries
from test_sourcewise_nonempty_gpu import CLASSES, LISTS, built, class_model, expanded_oracle, filled_counts
from test_sourcewise_sampler_gpu import OWN_4_2, bits, planner_points

pytestmark = pytest.mark.gpu

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET = 1, 2, 16
ROW_LIMIT = 32


def rows_per_point(own):
    return sum(1 << len(o) for o in own)


def own_of(name):
    """the own axes class_model gives the class (test_sourcewise_sampler_gpu.class_case), without building a model"""
    return OWN_4_2 if name == 's4_e2' else toy_cases.CLASS_OWN[name]


ELIGIBLE = [name for name in CLASSES if rows_per_point(own_of(name)) <= ROW_LIMIT]
REFUSED = [name for name in CLASSES if name not in ELIGIBLE]
SIZES, CELLS, DATASETS = (1, 16, 17, 33), (0, 1, 2, 0), (0, 0, 0, 1)


def scan_model(name, B):
    """class_model's own axes and recipe on four axes of FOUR anchors: three cells per axis, so that three cell tuples exist
    whatever axes the class owns"""
    small, rng = class_model(name, B)
    assert [tuple(o) for o in small['own']] == [tuple(o) for o in own_of(name)]
    return fo.random_model(rng, (4, 4, 4, 4), small['own'], B, zero_quarter=(1,)), rng


def grouped_points(model, rng, sizes=SIZES, cells=CELLS, datasets=DATASETS):
    """Group g: sizes[g] points with EVERY axis in cell cells[g], evaluated against datasets[g]; the first point of the group in
    cell 1 lies exactly on anchor 1 of every axis, the first of the group in the last cell on the upper edge of the box.  The
    call's order is shuffled -> (z, rs, ds, group of every point)"""
    g = [np.asarray(a, dtype=float) for a in model['anchor_z']]
    d, S = len(g), len(model['own'])
    z, ds, grp = [], [], []
    for k, (n, c, t) in enumerate(zip(sizes, cells, datasets)):
        for j in range(n):
            u = rng.uniform(0.05, 0.95, d)
            row = np.array([g[i][c] + (g[i][c + 1] - g[i][c]) * u[i] for i in range(d)])
            if j == 0 and c == 1:
                row = np.array([g[i][1] for i in range(d)])
            if j == 0 and c == len(g[0]) - 2:
                row = np.array([g[i][-1] for i in range(d)])
            z.append(row)
            ds.append(t)
            grp.append(k)
    order = rng.permutation(len(z))
    rs = rng.uniform(0.5, 1.6, (len(z), S))
    return np.array(z)[order], rs, np.array(ds, dtype=np.int64)[order], np.array(grp)[order]


def check_scan(ctx, z, rs, ds, counts, oracle, what):
    """every ll of one bi_eval_sourcewise_scan call against oracle(z, rs, counts[ds]) -> (ll, the worst ratio)"""
    ll, st = ctx.eval_scan(z, rs, ds)
    assert not st.any()
    worst = 0.0
    for p in range(len(z)):
        want = oracle(z[p], rs[p], counts[ds[p]])
        worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (what, p)))
    print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (what, worst, C_POISSON))
    return ll, worst


@pytest.mark.parametrize('B,nnz', LISTS)
@pytest.mark.parametrize('name', ELIGIBLE)
def test_every_eligible_class_at_every_list(name, B, nnz):
    t0 = time.time()
    model, rng = scan_model(name, B)
    z, rs, ds, grp = grouped_points(model, rng)
    if nnz == B:
        counts = np.stack([filled_counts(rng, model, z[0], rs[0]), filled_counts(rng, model, z[1], rs[1])])
    else:
        counts = np.stack([no.sparse_counts(rng, B, nnz), no.sparse_counts(rng, B, nnz)])
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx, [nnz, nnz])
        before = ctx.get_param('n_scan_launches')
        ll, worst = check_scan(ctx, z, rs, ds, counts, expanded_oracle(model), '%s B=%d nnz=%d' % (name, B, nnz))
        c = ctx.last_scan_counters
        assert list(c) == [4, 1 + 1 + 2 + 3, sum(SIZES), c[3], 1] and c[3] > 0
        assert ctx.get_param('n_scan_launches') == before + 1 and ctx.get_param('last_scan_groups') == 4
        assert ctx.get_param('last_scan_max_items') == 3 and ctx.get_param('last_scan_prod') == 1
        if nnz == 0:                                        # no listed bin: ll = -sum_s lambda_s, from the planner alone
            for p in range(0, len(z), 9):
                total = fo.expectation(model, z[p], rs[p]).sum()
                assert abs(ll[p] + total) <= 1e-12 * total
    finally:
        ctx.close()
    print('%s B=%d nnz=%d: %.1f s' % (name, B, nnz, time.time() - t0))


@pytest.fixture(scope='module')
def small():
    """toy_cases' small shape at B = 63: three sources over (3, 2, 4) anchors, one without own axes"""
    rng = np.random.default_rng(63)
    return fo.random_model(rng, toy_cases.N_ANCHOR, toy_cases.OWN, 63), rng


def test_the_product_form_and_its_exits(small):
    """Lists of ones and twos alone (every block takes one logarithm of the product), mixed counts, and the exits: a listed bin
    that expects nothing and a count that is no integer -- exactly bi_eval_factored's -inf and -inf.  (A nan count, the third
    exit of k_scan_mfma, cannot reach a source-wise store: bi_factored_set_counts refuses it, which is asserted here.)"""
    model, _ = small
    rng = np.random.default_rng(12)
    model = dict(model, ps=[np.array(p) for p in model['ps']])
    for s in range(3):
        model['ps'][s][..., 5] = 0.0                        # bin 5: every template is 0 at every anchor
    ones_twos = no.sparse_counts(rng, 63, 40, high=2)
    mixed = no.sparse_counts(rng, 63, 40, high=4)
    ones_twos[5] = mixed[5] = 0.0
    assert set(np.unique(ones_twos)) == {0.0, 1.0, 2.0} and mixed.max() > 2
    hit, half, bad = ones_twos.copy(), ones_twos.copy(), ones_twos.copy()
    hit[5] = 2.0
    half[int(np.flatnonzero(ones_twos)[3])] = 2.5
    bad[int(np.flatnonzero(ones_twos)[7])] = np.nan
    counts = np.stack([ones_twos, mixed, hit, half])
    z, rs, ds, _ = grouped_points(model, rng, sizes=(17, 17, 17, 17), cells=(0, 0, 0, 0), datasets=(0, 1, 2, 3))
    ctx = toy_cases.upload(model, counts)
    try:
        with pytest.raises(ValueError, match='every count must be finite'):
            ctx.set_counts(np.stack([ones_twos, bad]))
        ctx.set_counts(counts)
        built(ctx)
        ll, st = ctx.eval_scan(z, rs, ds)
        ref, st_ref = ctx.eval(z, rs, ds)
        assert not st.any() and not st_ref.any() and ctx.last_scan_counters[0] == 4 and ctx.get_param('last_scan_prod') == 1
        assert np.all(ll[ds == 2] == -np.inf) and np.all(ll[ds == 3] == -np.inf)
        special = ds >= 2
        assert np.array_equal(bits(ll[special]), bits(ref[special]))
        oracle = expanded_oracle(model)
        worst = 0.0
        for p in np.flatnonzero(~special):
            want = oracle(z[p], rs[p], counts[ds[p]])
            worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='product form ll[%d] (dataset %d)' % (p, ds[p])))
        print('product form and mixed counts: worst |err| / (2^-52 cond) = %.3g of C = %d' % (worst, C_POISSON))
    finally:
        ctx.close()


def test_rejected_points_among_live_ones(small):
    """Out of bounds, a negative rate, a bad dataset, mixed in with live points: status words and -inf are the planner's, bit for
    bit those of bi_eval_sourcewise_planned; the live points meet the oracle's bound"""
    model, _ = small
    rng = np.random.default_rng(5)
    counts = np.stack([no.sparse_counts(rng, 63, k) for k in (20, 0, 63)])
    z, rs, ds, _ = planner_points(model, 3, 240, 17)
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx, [20, 0, 63])
        ll, st = ctx.eval_scan(z, rs, ds)
        want_ll, want_st = ctx.eval_planned(z, rs, ds)
        assert np.array_equal(st, want_st) and set(np.unique(st)) == {0, ST_OUT_OF_BOUNDS, ST_UNPHYSICAL, ST_BAD_DATASET}
        dead = st != 0
        assert np.array_equal(bits(ll[dead]), bits(want_ll[dead])) and np.all(ll[dead] == -np.inf)
        assert ctx.last_scan_counters[2] == np.count_nonzero(~dead) >= 150
        oracle = expanded_oracle(model)
        worst = 0.0
        for p in np.flatnonzero(~dead):
            want = oracle(z[p], rs[p], counts[ds[p]])
            worst = max(worst, check_entries(ll[p], want['ll'], want['ll_cond'], what='live ll[%d]' % p))
        print('live points among rejected ones: worst |err| / (2^-52 cond) = %.3g of C = %d' % (worst, C_POISSON))
        # every point rejected: nothing is evaluated
        before = ctx.get_param('n_scan_launches')
        ll0, st0 = ctx.eval_scan(z[dead], rs[dead], ds[dead])
        assert np.all(ll0 == -np.inf) and np.array_equal(st0, st[dead]) and ctx.get_param('n_scan_launches') == before
        assert list(ctx.last_scan_counters[:3]) == [0, 0, 0]
        # P = 0 is a no-op
        assert ctx._dev._lib.bi_eval_sourcewise_scan(ctx._dev._h, 0, None, None, None, None, None, None) == 0
        # NULL rate scales and datasets: ones, dataset 0
        a, _ = ctx.eval_scan(z[~dead][:20])
        b, _ = ctx.eval_scan(z[~dead][:20], np.ones((20, 3)), np.zeros(20, dtype=np.int64))
        assert np.array_equal(bits(a), bits(b))
    finally:
        ctx.close()


def test_two_datasets_of_one_cell_are_two_groups():
    """lists of different lengths in one call, an empty one among them: (cell tuple, dataset) is the group"""
    B = 1027
    model, rng = scan_model('mixed', B)
    counts = np.stack([no.sparse_counts(rng, B, 0), no.sparse_counts(rng, B, 700), no.sparse_counts(rng, B, 5)])
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx, [0, 700, 5])
        z, rs, ds, _ = grouped_points(model, rng, sizes=(9, 18), cells=(1, 1), datasets=(1, 0))
        _, worst = check_scan(ctx, z, rs, ds, counts, expanded_oracle(model), 'two datasets of one cell')
        assert list(ctx.last_scan_counters[:3]) == [2, 1 + 2, 27]
        z, rs, ds, _ = grouped_points(model, rng, sizes=(5, 5, 5), cells=(2, 2, 2), datasets=(0, 1, 2))
        check_scan(ctx, z, rs, ds, counts, expanded_oracle(model), 'three datasets of one cell')
        assert list(ctx.last_scan_counters[:3]) == [3, 3, 15]
    finally:
        ctx.close()


def test_repeatability_and_permutation():
    """The same call gives the same bits; the same points in another order of the call meet the oracle's bound (the items' make-up
    may differ, so the bits may)"""
    B = 1027
    model, rng = scan_model('s4_e1', B)
    counts = np.stack([no.sparse_counts(rng, B, 513), no.sparse_counts(rng, B, 100)])
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx)
        z, rs, ds, _ = grouped_points(model, rng)
        oracle = expanded_oracle(model)
        ll, _ = check_scan(ctx, z, rs, ds, counts, oracle, 'first call')
        again, _ = ctx.eval_scan(z, rs, ds)
        assert np.array_equal(bits(again), bits(ll))
        order = rng.permutation(len(z))
        check_scan(ctx, z[order], rs[order], ds[order], counts, oracle, 'permuted call')
    finally:
        ctx.close()


def test_a_long_group_is_cut():
    """530 points of one (cell tuple, dataset) beside a group of 5: a group of equal keys is cut every 16 items (the least cut; the
    rule grows it only for batches of about 10^5 points and more), so the 530 are groups of 256, 256 and 18 points -- 16, 16 and 2
    items, the last one padded -- with the rows of the first: more groups than keys, the same values"""
    B = 1027
    model, rng = scan_model('s2_e2', B)
    counts = no.sparse_counts(rng, B, 513)[None]
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx, [513])
        z, rs, ds, grp = grouped_points(model, rng, sizes=(530, 5), cells=(1, 2), datasets=(0, 0))
        oracle = expanded_oracle(model)
        want = [oracle(z[p], rs[p], counts[0]) for p in range(len(z))]              # once, for every call below

        def check(ll, points, what):
            worst = max(check_entries(ll[i], want[p]['ll'], want[p]['ll_cond'], what='%s ll[%d]' % (what, p)) for i, p in enumerate(points))
            print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (what, worst, C_POISSON))

        before = ctx.get_param('n_scan_launches')
        ll, st = ctx.eval_scan(z, rs, ds)
        assert not st.any()
        check(ll, np.arange(len(z)), 'a group of 530 points')
        assert list(ctx.last_scan_counters[:3]) == [3 + 1, 16 + 16 + 2 + 1, 535] and ctx.last_scan_counters[4] == 1
        assert ctx.get_param('last_scan_groups') == 4 and ctx.get_param('last_scan_max_items') == 16
        assert ctx.get_param('n_scan_launches') == before + 1
        again, _ = ctx.eval_scan(z, rs, ds)
        assert np.array_equal(bits(again), bits(ll))
        # one point less than a cut, exactly a cut, one more: 1, 1 and 2 groups
        for n, groups, items in ((255, 1, 16), (256, 1, 16), (257, 2, 17)):
            keep = np.flatnonzero(grp == 0)[:n]
            part, st = ctx.eval_scan(z[keep], rs[keep], ds[keep])
            assert not st.any() and list(ctx.last_scan_counters[:3]) == [groups, items, n]
            assert ctx.get_param('last_scan_max_items') == 16
            check(part, keep, '%d points of one group' % n)
    finally:
        ctx.close()


def test_refusals_launch_nothing():
    model, rng = scan_model('mixed', 63)
    counts = no.sparse_counts(rng, 63, 5)
    z, rs, ds, _ = grouped_points(model, rng, sizes=(3,), cells=(0,), datasets=(0,))
    ctx = toy_cases.upload(model, counts)
    try:
        before = ctx.get_param('n_scan_launches')
        with pytest.raises(ValueError, match='bi_sourcewise_build_nonempty'):           # the form is not built
            ctx.eval_scan(z, rs, ds)
        built(ctx)
        ctx.set_param('sourcewise_form', 0)                                             # built, not chosen
        with pytest.raises(ValueError, match='bi_sourcewise_build_nonempty'):
            ctx.eval_scan(z, rs, ds)
        assert ctx.get_param('n_scan_launches') == before
    finally:
        ctx.close()
    assert REFUSED == ['e3x8']
    model, rng = class_model('e3x8', 63)
    assert rows_per_point(model['own']) == 64
    z, rs = toy_cases.box_points(model, rng, 3)
    ctx = toy_cases.upload(model, counts)
    try:
        built(ctx)
        before = ctx.get_param('n_scan_launches')
        with pytest.raises(ValueError, match='64 rows.*at most 32'):
            ctx.eval_scan(z, rs)
        assert ctx.get_param('n_scan_launches') == before
        ll, st = ctx.eval_planned(z, rs)                                                # the per-point route takes it as before
        assert not st.any() and np.isfinite(ll).all()
    finally:
        ctx.close()
