"""The cases of tests/sourcewise_walk_cases.py are what they claim to be: checked on the CPU, so that a case that silently stops
reaching its geometry or stops filling its tiles (a size edited, a rate rescaled) fails here and not only on the device, where
test_sourcewise_walk_gpu.py reads the launch geometry from the counters last_morph_nbx / last_morph_items."""
import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_toy_cases as toy_cases
import sourcewise_walk_cases as wc


@pytest.fixture(scope='module')
def cases():
    return {key: wc.make_case(*key) for key in wc.KEYS}


def test_the_families_and_their_classes():
    assert wc.FAMILIES['load_forms'] == ['e3x8', 'mixed', 'mixed_padded', 's2_e1', 's2_e2', 's2_e3', 's4_e1', 's8_e1', 's8_e2']
    assert sorted(wc.FAMILIES['load_forms']) == sorted(toy_cases.CLASS_OWN)
    assert sorted(wc.FAMILIES['chunked']) == ['mixed', 's2_e1', 's8_e2'] and sorted(wc.FAMILIES['striding']) == ['s2_e1', 's8_e2']
    assert wc.FAMILIES['past_the_end'] == ['s2_e1'] and sorted(wc.FAMILIES) == sorted(wc.GEOMETRIES)
    assert wc.VALUE_ONLY == {('striding', 's8_e2')} and len(wc.KEYS) == 15 and len(wc.FULL_KEYS) == 14
    assert len(wc.EXPECT_KEYS) == 13 and len(wc.CURVATURE_KEYS) == 5
    assert {c for c, _ in wc.GEOMETRIES['chunked']} == {1, 3} and {c for c, _ in wc.GEOMETRIES['striding']} == {8, 1}
    assert {c for c, _ in wc.GEOMETRIES['past_the_end']} == {34}
    for family in wc.FAMILIES:
        assert {nt for _, nt in wc.GEOMETRIES[family]} == {0, 1}


def test_row_lengths_give_the_intended_tiles():
    assert wc.bins_of('load_forms') == 1027 and wc.n_tiles(1027) == 3
    for family, tiles in (('chunked', 193), ('striding', 1025), ('past_the_end', 2177)):
        B = wc.bins_of(family)
        assert B == tiles * 512 - 100 and wc.n_tiles(B) == tiles and wc.n_tiles(B + 100) == tiles and wc.n_tiles(B + 101) == tiles + 1
    assert wc.bins_of('chunked') == 98716 and wc.bins_of('striding') == 524700


def test_the_walk_of_every_geometry_visits_every_tile_once():
    """ItemTiles replayed on min(tiles, 1024) blocks: chunking on or off as the case claims, the steps past a ragged last chunk,
    and the blocks' trip counts"""
    want = {(3, 8): (0, {1}, 0), (193, 1): (0, {1}, 0), (193, 3): (2, {1, 2}, 0), (1025, 1): (0, {1, 2}, 0), (1025, 8): (7, {1, 2}, 0),
            (2177, 34): (33, {2, 3}, 2)}
    for (tiles, chunks), (past, trips, behind) in want.items():
        visits, got_past, got_trips, got_behind = wc.walk(tiles, chunks)
        got = wc.walk(tiles, chunks)
        assert (got[0] == 1).all() and got[1:] == (past, trips, behind), (tiles, chunks) + got[1:]
    # the chunked order is what the 193-, 1025- and 2177-tile rows run, and not the three-tile rows
    assert 193 >= wc.CHUNK_MIN_TILES * 3 and 1025 >= wc.CHUNK_MIN_TILES * 8 and 3 < wc.CHUNK_MIN_TILES * 8
    assert wc.PAST_TILES == wc.CHUNK_MIN_TILES * wc.PAST_CHUNKS + 1


def test_where_a_tile_lies_behind_a_step_past_the_end():
    """Only `past_the_end` has tiles BEHIND a step past the end (a walk that stopped there would lose them).  The last chunk is
    short by at most chunks - 1 tiles, so the first such step is at most (chunks - 1)^2 steps before the end of the walk, and a
    later step of the same block exists only where nbx < (chunks - 1)^2.  On the grids of FacBatch::run, nbx = min(tiles, 1024)
    with tiles >= 64 chunks: never up to 33 chunks (32^2 = 1024), replayed here for EVERY chunk count up to 33 over every
    shortfall of the last chunk and at two, three and five trips per block; from 34 chunks on it happens (64 is spared only
    because 1024 is a multiple of it: a block stays in one region)."""
    assert (33 - 1) ** 2 <= wc.FAC_BLOCKS < (34 - 1) ** 2
    for chunks in range(2, 34):
        for first in (wc.CHUNK_MIN_TILES * chunks, max(wc.CHUNK_MIN_TILES * chunks, 2 * wc.FAC_BLOCKS + 7), 4 * wc.FAC_BLOCKS + 11):
            for tiles in range(first, first + chunks + 1):
                visits, _, _, behind = wc.walk(tiles, chunks)
                assert (visits == 1).all() and behind == 0, (tiles, chunks, behind)
    seen = {chunks: max(wc.walk(tiles, chunks)[3] for tiles in range(64 * chunks, 65 * chunks + 1)) for chunks in range(34, 67)}
    assert all(seen[chunks] > 0 for chunks in seen if chunks != 64) and seen[64] == 0, seen
    assert wc.PAST_CHUNKS == 34 and wc.walk(wc.PAST_TILES - 1, wc.PAST_CHUNKS)[3] == 0 and wc.walk(wc.PAST_TILES, wc.PAST_CHUNKS)[3] == 2


@pytest.mark.parametrize('key', wc.KEYS, ids='-'.join)
def test_the_case_fills_every_tile_and_its_points_are_live(cases, key):
    c = cases[key]
    family, name = key
    n_anchor, own = wc.own_axes(family, name)
    B = fo.n_bins(c.model)
    assert B == wc.bins_of(family) and c.tiles == wc.n_tiles(B)
    assert [len(g) for g in c.model['anchor_z']] == list(n_anchor) and c.model['own'] == own
    assert sorted(len(o) for o in own) == sorted(len(o) for o in toy_cases.CLASS_OWN[name])       # the class of the table
    if key in (('striding', 's2_e1'), ('past_the_end', 's2_e1')):
        assert sum(int(np.prod(np.shape(m))) for m in c.model['mus']) == 3                        # three rows
    # two points, one inside a cell and one on the upper edge of the box; two datasets, one per point
    assert c.z.shape == (2, len(n_anchor)) and c.rs.shape == (2, len(own)) and list(c.ds) == [0, 1]
    assert c.counts.shape == (2, B) and c.real.shape == (2, B)
    lo, hi = (np.array([g[k] for g in c.model['anchor_z']]) for k in (0, -1))
    assert np.all((lo < c.z[0]) & (c.z[0] < hi)) and np.array_equal(c.z[1], hi)
    for g, z0 in zip(c.model['anchor_z'], c.z[0]):
        assert z0 not in g
    # live: inside the box with rates in (0, inf); about PER_BIN events per bin
    for p in range(2):
        mu = fo.expectation(c.model, c.z[p], c.rs[p])
        assert np.isfinite(mu).all() and (mu > 0).all()
        assert 0.4 * wc.PER_BIN < mu.mean() < 2.5 * wc.PER_BIN
    assert np.all(c.rs > 0) and all(np.all(np.asarray(m) > 0) for m in c.model['mus'])
    # more than half of the bins of EVERY tile are filled, in every dataset of either kind
    for data in (c.counts, c.real):
        assert np.all(np.isfinite(data)) and np.all(data >= 0)
        filled, size = wc.filled_per_tile(data)
        assert filled.shape == (2, c.tiles) and size[-1] == B - (c.tiles - 1) * 512
        assert np.all(2 * filled > size[None, :]), (key, np.argwhere(2 * filled <= size[None, :])[:4])
    assert np.array_equal(c.counts, np.round(c.counts)) and not np.array_equal(c.counts[0], c.counts[1])
    # both branches of the per-bin terms are taken on every dataset
    assert np.all(np.count_nonzero(c.counts == 0, axis=1) > 0) and np.all(np.count_nonzero(c.real == 0, axis=1) >= B // 4)
    # the same arrays on every call
    again = wc.make_case(*key)
    assert np.array_equal(again.counts, c.counts) and np.array_equal(again.real, c.real) and np.array_equal(again.z, c.z)


@pytest.mark.parametrize('key', wc.KEYS, ids='-'.join)
def test_the_oracle_values_are_finite(cases, key):
    """the value and gradient oracle of both points (every other oracle of a case is a sum over the same finite per-bin
    expectations; the device test computes those)"""
    c = cases[key]
    for p in range(2):
        want = fo.factored_derivatives(c.model, c.z[p], c.rs[p], c.counts[c.ds[p]])
        assert np.isfinite(want['ll']) and np.isfinite(want['grad']).all() and np.isfinite(want['grad_cond']).all()
