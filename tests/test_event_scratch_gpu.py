"""The event-level host path (csrc/bi_events.h) after its entry points were folded onto one axis walk, one rates helper and
one simulation setup, with scoped scratch buffers: the texts of bi_last_error are the ones recorded before the change, the
scratch of a call comes back to the recycle cache (also after a refused call), and the simulators still hand their pmf
scratch back before the scoring pass allocates.

Everything runs on one small model: d = 1 with 3 anchors, S = 2 sources, 8 x 6 bins, rates near 20 and 31 events."""
import ctypes as C

import numpy as np
import pytest

import toy_oracle as orc

pytestmark = pytest.mark.gpu

ANCHORS = [np.array([-1., 0., 1.])]
EDGES = [np.linspace(-4, 4, 9), np.array([0., 0.4, 1., 2.2, 3.5, 5., 6.])]            # 8 x 6 bins
MUS = np.array([[18., 29.], [20., 31.], [22., 33.]])
INF = float('inf')


def centres(edges):
    return [0.5 * (e[1:] + e[:-1]) for e in edges]


def densities(edges, seed):
    """[3 anchors, S = 2, B]: positive densities, every row integrates to one over the bins"""
    rng = np.random.default_rng(seed)
    vol = orc.bin_volumes(edges)
    p = rng.uniform(0.2, 1.0, size=(3, 2, len(vol)))
    return p / (p * vol).sum(axis=-1, keepdims=True)


def contexts(edges=EDGES, seed=11):
    from blueice_amd.device import DeviceContext
    tp, c = DeviceContext(0), DeviceContext(0)
    tp.upload_model(ANCHORS, densities(edges, seed), MUS)
    return tp, c


def axes_args(arrs):
    """-> (k, n [k] int32, flat values) of a list of axes; for no axis at all the pointers stay valid"""
    n = np.array([len(a) for a in arrs] or [0], dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64) for a in arrs] or [np.zeros(1)]))
    return len(arrs), n, flat


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the raw entry points (the wrappers of blueice_amd.device refuse some of the bad inputs before the library sees them) ----

COORDS = np.ascontiguousarray(np.array([[-3.5, -1.2, 0.1, 2.2, 3.9], [0.1, 0.9, 2.0, 3.6, 5.5]]))      # 5 events inside the space


def call(entry, method, tp, c, axes, z=(0.,), rate_scale=None, seed=3):
    """-> (rc, the context the message is left with)"""
    lib = tp._lib
    k, n, flat = axes_args(axes)
    code = {'-': 0, 'piecewise': 0, 'linear': 1}[method]
    z = np.array(z, dtype=np.float64)
    rs = None if rate_scale is None else np.array(rate_scale, dtype=np.float64)
    if entry == 'set_analysis_space':
        return lib.bi_set_analysis_space(tp._h, k, p(n), p(flat)), tp
    if entry == 'histogram_events':
        out = np.zeros(4096)
        return lib.bi_histogram_events(tp._h, k, p(n), p(flat), COORDS.shape[1], p(COORDS), p(out)), tp
    if entry == 'score_events':
        return lib.bi_score_events(tp._h, c._h, code, k, p(n), p(flat), COORDS.shape[1], p(COORDS), 1e-12), c
    if entry == 'score_event_sets':
        offsets = np.array([0, 2, 5], dtype=np.int64)
        return lib.bi_score_event_sets(tp._h, c._h, code, k, p(n), p(flat), 2, p(offsets), p(COORDS), 1e-12), c
    if entry == 'simulate_events':
        per_source = np.zeros(2, dtype=np.int64)
        return lib.bi_simulate_events(tp._h, c._h, p(z), p(rs), code, k, p(n), p(flat), seed, 1e-12, p(per_source)), c
    assert entry == 'simulate_event_toys'
    counts = np.zeros((3, 2), dtype=np.int64)
    return lib.bi_simulate_event_toys(tp._h, c._h, p(z), p(rs), code, k, p(n), p(flat), 3, seed, 1e-12, p(counts)), c


def bad_axes(good, min_n):
    """the bad axis lists of an entry point whose good axes are `good` and which needs `min_n` values per axis"""
    short = [good[0], good[1][:min_n - 1]]
    rep = good[1].copy()
    rep[2] = rep[1]
    desc = good[0].copy()
    desc[[1, 2]] = desc[[2, 1]]
    return [('zero axes', []), ('short axis', short), ('repeated edge', [good[0], rep]), ('descending edge', [desc, good[1]]),
            ('bin count', [good[0][:-1], good[1]])]


def cases():
    """every (entry, method, case name, keyword arguments of call())"""
    out = []
    for entry in ('set_analysis_space', 'histogram_events'):
        for name, axes in bad_axes(EDGES, 2):
            if entry == 'histogram_events' and name == 'bin count':
                continue                                       # (it bins into whatever the edges describe: no templates to disagree with)
            out.append((entry, '-', name, dict(axes=axes)))
    for entry in ('score_events', 'score_event_sets', 'simulate_events', 'simulate_event_toys'):
        sim = entry.startswith('simulate')
        for method in ('piecewise', 'linear'):
            good = EDGES if (sim or method == 'piecewise') else centres(EDGES)
            for name, axes in bad_axes(good, 3 if (sim and method == 'linear') else 2):
                out.append((entry, method, name, dict(axes=axes)))
            if sim:
                out.append((entry, method, 'outside the box', dict(axes=EDGES, z=(2.,))))
                out.append((entry, method, 'negative rate scale', dict(axes=EDGES, rate_scale=(-1., 1.))))
                out.append((entry, method, 'infinite rate scale', dict(axes=EDGES, rate_scale=(INF, 1.))))
    return out


# bi_last_error of every case above, recorded from the library as it was before the entry points shared their checks
A2E = "axis 1 needs at least two edges"
A2G = "axis 1 needs at least two grid values"
FEW = "axis 1 has too few bin edges"
ASC_E = "bin edges of axis %d are not strictly ascending"
ASC_G = "grid values of axis %d are not strictly ascending"
RECORDED = {
    'set_analysis_space': ["need 1..8 axes with edges", A2E, ASC_E % 1, ASC_E % 0, "analysis space has 42 bins, the model 48"],
    'histogram_events': ["need 1..8 axes with edges, and a counts buffer", A2E, ASC_E % 1, ASC_E % 0],
    'score piecewise': ["need 1..8 axes with grid values", A2G, ASC_G % 1, ASC_G % 0, "the grid describes 42 bins, the templates have 48"],
    'score linear': ["need 1..8 axes with grid values", A2G, ASC_G % 1, ASC_G % 0, "the grid describes 42 bins, the templates have 48"],
    'simulate': ["need 1..8 axes with bin edges", FEW, ASC_E % 1, ASC_E % 0, "the edges describe 42 bins, the templates have 48",
                 "simulation point is outside the anchor box", "event simulation needs rates in [0, inf)",
                 "event simulation needs rates in [0, inf)"],
}


def recorded():
    table = {}
    for entry, method, name, _ in cases():
        key = entry if method == '-' else ('simulate' if entry.startswith('simulate') else 'score ' + method)
        done = sum(1 for q in table if q[:2] == (entry, method))
        table[entry, method, name] = RECORDED[key][done]
    return table


def parked(ctx):
    return ctx.get_param('recycle_cache_bytes'), ctx.get_param('user_allocations')


def one_toy(tp, c, seed=3):
    n = tp.simulate_events(c, 'piecewise', EDGES, [0.], seed=seed)
    coords, source = c.download_events()
    return n, coords, source, c.eval([0.])[0][0]


def same_toy(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_messages_are_the_recorded_ones_and_a_refused_call_keeps_nothing():
    tp, c = contexts()
    want = recorded()
    one_toy(tp, c)
    first = one_toy(tp, c)
    steady = parked(tp), parked(c)
    got = {}
    for entry, method, name, kw in cases():
        rc, owner = call(entry, method, tp, c, **kw)
        text = owner._lib.bi_last_error(owner._h).decode()
        print('%-20s %-10s %-20s rc %d  %s' % (entry, method, name, rc, text))
        assert rc == -1, (entry, method, name, rc, text)           # BI_ERR_INVALID
        got[entry, method, name] = text
        assert (parked(tp), parked(c)) == steady, (entry, method, name)
        if entry not in ('set_analysis_space', 'histogram_events'):
            assert same_toy(one_toy(tp, c), first), (entry, method, name)
            assert (parked(tp), parked(c)) == steady, (entry, method, name)
    assert got == want
    # several event sets and an axis of one grid value: refused by the axis check itself
    for method in ('piecewise', 'linear'):
        assert got['score_event_sets', method, 'short axis'] == "axis 1 needs at least two grid values"
    tp.close()
    c.close()


def pick_seed(T):
    """the first seed whose T toys have decided counts, one of them odd -- on the CPU"""
    from blueice_amd import toy_seed
    for seed in range(1, 200):
        tot, decided = np.zeros(T), True
        for t in range(T):
            for s, M in enumerate(MUS[1]):
                n, und = orc.event_count(float(M), toy_seed(seed, t) ^ orc.SIM_COUNT_KEY, [s])
                tot[t] += n[0]
                decided &= not und[0]
        if decided and (tot % 2 == 1).any():
            return seed, tot
    raise AssertionError("no seed below 200 gives an odd toy")


def test_scratch_comes_back():
    tp, c = contexts()
    users = parked(tp)[1], parked(c)[1]
    runs, cache = [], []
    for _ in range(3):
        runs.append(one_toy(tp, c, seed=9))
        cache.append((parked(tp), parked(c)))
    print('simulate_events: parked bytes after each call', cache)
    assert cache[1] == cache[2]
    assert same_toy(runs[0], runs[1]) and same_toy(runs[0], runs[2])
    seed, tot = pick_seed(3)
    runs, cache = [], []
    for _ in range(3):
        counts = tp.simulate_event_toys(c, 'piecewise', EDGES, [0.], n_toys=3, seed=seed)
        coords, source = c.download_events()
        runs.append((counts, coords, source, c.eval([[0.]] * 3, dataset=[0, 1, 2])[0]))
        cache.append((parked(tp), parked(c)))
    print('simulate_event_toys: parked bytes after each call', cache)
    assert cache[1] == cache[2]
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0]))
    assert np.array_equal(runs[0][0].sum(axis=1), tot)
    off, n = c.event_set_offsets(), c.event_set_counts()
    assert (n % 2 == 1).any() and ((off[1:] - off[:-1]) > n).any()                      # an odd toy, and a padding column behind it
    assert (parked(tp)[1], parked(c)[1]) == users
    tp.close()
    c.close()


# recycle_cache_bytes of the target directly after the call below in fresh contexts, read from the library as it was before the
# change (the simulators released their pmf scratch with explicit calls ahead of the scoring pass)
PARKED_AFTER_SIMULATE_EVENTS = 67096
PARKED_AFTER_SIMULATE_EVENT_TOYS = 68136


def wide_edges():
    return [np.linspace(-4, 4, 65), np.linspace(0, 6, 65)]                              # 64 x 64 bins: 64 KiB of pmf scratch per buffer


def test_pmf_scratch_is_released_before_scoring():
    """S x B doubles twice (pmf rows and their running sums) dwarf what scoring about 50 events allocates: the target's new
    model takes one of them from the cache only if they were parked before the scoring pass began"""
    edges = wide_edges()
    tp, c = contexts(edges, seed=12)
    n = tp.simulate_events(c, 'piecewise', edges, [0.], seed=5)
    got = c.get_param('recycle_cache_bytes')
    print('simulate_events: %d events, %d bytes parked' % (n.sum(), got))
    assert 30 < n.sum() < 75
    tp.close()
    c.close()
    tp, c = contexts(edges, seed=12)
    tp.simulate_event_toys(c, 'piecewise', edges, [0.], n_toys=3, seed=5)
    got_toys = c.get_param('recycle_cache_bytes')
    print('simulate_event_toys: %d bytes parked' % got_toys)
    tp.close()
    c.close()
    assert got == PARKED_AFTER_SIMULATE_EVENTS
    assert got_toys == PARKED_AFTER_SIMULATE_EVENT_TOYS
