"""The table of the toy-MC evaluation tests (tests/toy_value_cases.py) on the CPU: `values` is the exact oracle of
tests/derivative_oracle.py, the table holds every gate and edge it promises, the per-entry bound rejects every mutant of a plain
float64 evaluation, and that plain evaluation itself stays far inside the bound.  Run with -s for the mutants' smallest and the
reference's worst |err| / (2^-52 cond): the figures the device's margin under C = 256 is judged against."""
import math

import numpy as np

import derivative_oracle as do
import toy_value_cases as tv


def test_values_is_the_oracle_of_single_evaluations():
    tab = tv.edge_table(variant='count32767')
    rows = [tab.rows[k] for k in ('empty', 'one@1', 'one@%d' % (tv.B_EDGE - 1), 'all7', 'tile_end_4096', 'tile_end_8192', 'run1', 'run5', 'run8',
                                  'run17', 'run48', 'run49', 'run97', 'run128', 'run129', 'run257')]
    rows += [tab.cell[0]] + tab.fillers[:3] + tab.fillers[-3:]
    assert len(set(rows)) >= 20
    for z, rs in tv.POINTS_1:
        ll, cond = tab.oracle(z, rs)
        for t in rows:
            o = do.derivatives(tab.model, [z], rs, counts=tab.counts[t], hessian=False)
            assert abs(ll[t] - o['ll']) <= do.EPS * o['ll_cond'], (t, ll[t], o['ll'], o['ll_cond'])
            assert abs(cond[t] - o['ll_cond']) <= 1e-12 * o['ll_cond'], (t, cond[t], o['ll_cond'])
        t = tab.rows['minus_inf']
        assert ll[t] == -np.inf and cond[t] == np.inf
        with np.errstate(all='ignore'):
            assert do.derivatives(tab.model, [z], rs, counts=tab.counts[t], hessian=False)['ll'] == -np.inf
        assert np.all(np.isfinite(np.delete(ll, t))) and np.all(np.isfinite(np.delete(cond, t)))
    # no shape axis, dense Poisson data
    seam = tv.seam_table()
    ll, cond = seam.oracle(None, (1.2, 0.9))
    for t in (0, 1, 8191, 16384, seam.T - 1):
        o = do.derivatives(seam.model, np.zeros(0), (1.2, 0.9), counts=seam.counts[t], hessian=False)
        assert abs(ll[t] - o['ll']) <= do.EPS * o['ll_cond'] and abs(cond[t] - o['ll_cond']) <= 1e-12 * o['ll_cond']


def test_the_table_holds_the_gates_and_the_edges():
    tab = tv.edge_table()
    n, T, B = tab.counts, tab.T, tab.B
    assert (T, B) == (600, 4 * 8192 + 1)
    n_tl1, n_tlm = -(-B // tv.TILE1), -(-B // tv.TILE_MULTI)
    assert (n_tl1, n_tlm) == (5, 9) and B % tv.TILE1 == 1
    # the gates of both tiled routes, three dataset slices of 200 per tile, a ragged split for 257 datasets
    nnz = int((n > 0).sum())
    assert nnz >= 16 * T * n_tl1 and nnz >= 8 * T * n_tlm and n_tl1 >= 4 and n_tlm >= 4
    assert (T + 255) // 256 == 3 and T % 3 == 0 and (257 + 255) // 256 == 2 and 257 % 2 == 1
    assert n.min() >= 0 and np.all(n == np.floor(n))
    # the count maxima per variant; the variants differ from the base table in one cell of a filler row
    assert n.max() == 7
    for variant, top in tv.VARIANT_COUNTS.items():
        v = tv.edge_table(variant=variant)
        diff = np.argwhere(v.counts != n)
        if top is None:
            assert len(diff) == 0
        else:
            assert v.counts.max() == top and diff.tolist() == [list(v.cell)] and v.cell[0] in v.fillers and n[v.cell] > 0
    # run lengths per tiling
    r1, rm = tv.run_lengths(n, tv.TILE1), tv.run_lengths(n, tv.TILE_MULTI)
    assert r1.shape == (T, 5) and rm.shape == (T, 9)
    rows = tab.rows
    assert set(rows) == set(tv.ROW_NAMES) and len(set(rows.values())) == len(rows)
    assert rows['empty'] == 0 and max(rows.values()) == T - 1 and r1[0].sum() == 0
    for b in tv.ONE_ENTRY_BINS:
        t = rows['one@%d' % b]
        assert np.flatnonzero(n[t]).tolist() == [b]
    assert set(tv.ONE_ENTRY_BINS) == {1, 8190, 8193, 4094, 4097, B - 1}
    want = {1, 3, 4, 5, 7, 8, 9, 15, 16, 17}
    for s in (48, 64, 96, 128):
        want |= {s - 1, s, s + 1, s + 17, 2 * s + 1}
    assert set(tv.RUN_LENGTHS) == want and set(tab.runs.values()) == want
    t1, tm = tv.RUN_LO // tv.TILE1, tv.RUN_LO // tv.TILE_MULTI
    for t, k in tab.runs.items():
        assert r1[t].sum() == k and r1[t, t1] == k and rm[t, tm] == k     # the same run in either tiling, nothing else
    t = rows['tile_end_4096']
    assert n[t, tv.RUN_HI - 1] > 0 and rm[t, tm] == 5 and rm[t].sum() == 5 and tv.RUN_HI % tv.TILE_MULTI == 0
    t = rows['tile_end_8192']
    assert n[t, 3 * tv.TILE1 - 1] > 0 and r1[t, t1] == 5 and r1[t].sum() == 5
    t = rows['all7']
    assert set(np.unique(n[t])) == {0.0, 7.0} and (n[t] > 0).sum() == 250
    per = (n > 0).sum(axis=1)
    assert np.all((per[tab.fillers] >= 100) & (per[tab.fillers] <= 400)) and len(tab.fillers) > 500
    for lo in (0, 200, 400):                                          # every slice of 200 datasets holds named rows
        assert any(lo <= t < lo + 200 for t in rows.values())
    # long and short runs among the fillers: beyond the up-front slots of the narrowest variant, inside those of the widest
    assert rm[tab.fillers].max() > 48 and r1[tab.fillers].min() < 48
    # mu = 0 bins: empty everywhere but for n = 1 at bin 8192 of one dataset
    assert set(tv.ZERO_BINS) == {0, 8192, 12288, 8191, B - 1 - 8192}
    z = n[:, list(tv.ZERO_BINS)]
    assert z.sum() == 1 and n[rows['minus_inf'], 8192] == 1
    # mu_b is exactly 0 there and at most 1 / 2 elsewhere, at every test point of both models
    points = [(tab.model, z_, rs_) for z_, rs_ in tv.POINTS_1]
    m3 = tv.edge_table(tv.ANCHORS_3).model
    for zs, rss in (tv.multi_points(9), tv.rate_points(8)):
        points += [(m3, zs[p, 0], rss[p]) for p in range(len(zs))]
    cells = set()
    for model, z_, rs_ in points:
        mu, lg = tv.log_mu(model, [z_], rs_)
        zero = np.zeros(B, bool)
        zero[list(tv.ZERO_BINS)] = True
        assert np.all(mu.v[zero] == 0) and np.all(mu.v[~zero] > 0)
        assert np.all(np.abs(lg.v[~zero]) >= math.log(2.0))
        cells.add((len(model['anchor_z'][0]), do.Cell(model['anchor_z'], [z_]).k[0]))
    assert cells == {(2, 0), (3, 0), (3, 1)}
    assert any(0.0 in rs_ for _, _, rs_ in points) and tv.POINTS_1[0][0] < 0.5 < tv.POINTS_1[1][0] and 0.0 in tv.POINTS_1[1][1]
    for model in (tab.model, m3):                                     # ... for every anchor and source
        assert np.all(model['ps'][:, :, list(tv.ZERO_BINS)] == 0)
    seam = tv.seam_table()
    assert seam.T == 16390 and seam.T > 16384 and seam.T % 8 and seam.B == 600 and len(seam.model['anchor_z']) == 0


def test_the_bound_rejects_every_mutant():
    tab = tv.edge_table(variant='count8')
    (z0, r0), (z1, r1) = tv.POINTS_1
    want, cond = tab.oracle(z0, r0)
    fin = np.isfinite(want)
    p0, p1 = tv.Plain(tab.model, z0, r0, tab.counts), tv.Plain(tab.model, z1, r1, tab.counts)
    assert do.check_entries(p0.value()[fin], want[fin], cond[fin]) <= do.C_POISSON
    smallest = {}
    for name, f in tv.MUTANTS.items():
        got = f(tab, p0, p1)
        assert got.shape == want.shape
        q = do.ratio(got[fin], want[fin], cond[fin])
        smallest[name] = float(q.max())
        assert smallest[name] > do.C_POISSON, 'the mutant "%s" stays inside the bound (ratio %.3g)' % (name, smallest[name])
    assert len(smallest) == 9
    print('\nmutants, |err| / (2^-52 cond) of the worst dataset (C = %d):' % do.C_POISSON)
    for name in smallest:
        print('  %-48s %.3g' % (name, smallest[name]))
    print('smallest over all mutants: %.3g' % min(smallest.values()))


def test_a_plain_float64_evaluation_stays_inside_the_bound():
    """The reference's own error: pairwise np.sum per run, the runs, sum mu and sum lgamma as a kernel puts them together."""
    worst = {}
    for variant in tv.VARIANT_COUNTS:
        tab = tv.edge_table(variant=variant)
        for z, rs in tv.POINTS_1:
            want, cond = tab.oracle(z, rs)
            got = tv.numpy_values(tab.model, z, rs, tab.counts)
            worst['edge table'] = max(worst.get('edge table', 0.0), tv.check(got, want, cond, 'edge table %s' % variant))
    seam = tv.seam_table()
    want, cond = seam.oracle(None, (1.2, 0.9))
    worst['dense seam'] = tv.check(tv.numpy_values(seam.model, None, (1.2, 0.9), seam.counts), want, cond, 'dense seam')
    print('\nplain numpy evaluation, worst |err| / (2^-52 cond) (C = %d): %s' % (do.C_POISSON, ', '.join('%s %.3g' % kv for kv in worst.items())))
    assert max(worst.values()) <= do.C_POISSON
