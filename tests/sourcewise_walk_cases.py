"""Models, points and data of the source-wise tile-walk tests: shared by tests/test_sourcewise_walk_gpu.py (which runs every case
on the device at several launch geometries) and tests/test_sourcewise_walk_cases.py (which shows on the CPU that every case is
what it claims to be).  No test lives here.

The source-wise kernels (k_morph_factored, k_factored_curv, k_sourcewise_gof, k_sourcewise_real) walk an item's 512-bin tiles with
ItemTiles (bi_k_item.h) on min(tiles, 1024) blocks (FacBatch::run, bi_factored.h); k_sourcewise_expect writes bins.  Four families:

    load_forms   the nine (source slots, own axes) classes of sourcewise_toy_cases.CLASS_OWN at B = 1027 (three tiles, the last
                 of three bins): every instantiation, with plain and with nontemporal loads
    chunked      193 tiles: with tile_chunks = 3 three regions of 65 tiles, the last two tiles short (two steps past the end)
    striding     1025 tiles: one more than the blocks of an item, so that block 0 takes a second tile and k_finish adds 1024
                 partials per slot; with the default 8 chunks also chunked, seven steps past the end
    past_the_end 2177 tiles with tile_chunks = 34: regions of 65 tiles, the last of 32, so that 33 steps are past the end and two
                 tiles lie BEHIND such a step in their block's walk.  The first step past the end is 33^2 = (chunks - 1)^2 steps
                 before the end of the walk, so a block has a tile behind one only where nbx < (chunks - 1)^2: on the 1024
                 blocks of a long row from 34 chunks on, and on no grid of FacBatch::run with tile_chunks <= 33 (walk() below)

factored_oracle.random_model gives a few hundred events per source over ALL bins, which on a long row leaves nearly every bin
empty (the -mu branch alone); the rates are scaled to PER_BIN expected events per bin at the centre of the box.  Every case has
two points -- one inside a cell, one on the upper edge of the box -- and two datasets of either kind, dataset t drawn at point t
and read by point t, so that the counts of the second point start one padded row behind the first's."""
from collections import namedtuple

import numpy as np

import factored_oracle as fo
import sourcewise_toy_cases as toy_cases

TILE = 512                       # kTile
FAC_BLOCKS = 1024                # kFacBlocks: the blocks of an item at most
CHUNK_MIN_TILES = 64             # ItemTiles: the chunked order needs 64 tiles per chunk
PER_BIN = 1.6                    # expected events per bin (test_item_kernels_gpu.dense_case's figure)

LOAD_B = 1027                    # the row of the existing class tests
CHUNKED_TILES, STRIDING_TILES = 193, 1025
PAST_TILES, PAST_CHUNKS = 2177, 34         # the fewest chunks, and the shortest row for them, with a tile behind a step past the end
FAMILIES = {
    'load_forms': list(toy_cases.CLASS_CASES),
    'chunked': ['mixed', 's2_e1', 's8_e2'],
    'striding': ['s2_e1', 's8_e2'],
    'past_the_end': ['s2_e1'],
}
# (tile_chunks, nt_loads) of the two-point batches
GEOMETRIES = {
    'load_forms': [(8, 0), (8, 1)],
    'chunked': [(1, 0), (1, 1), (3, 0), (3, 1)],
    'striding': [(8, 0), (8, 1), (1, 0), (1, 1)],
    'past_the_end': [(PAST_CHUNKS, 0), (PAST_CHUNKS, 1)],
}
VALUE_ONLY = {('striding', 's8_e2')}         # value and gradient alone: the other oracles would need its 540 MB expansion
KEYS = [(family, name) for family in ('load_forms', 'chunked', 'striding', 'past_the_end') for name in FAMILIES[family]]
FULL_KEYS = [k for k in KEYS if k not in VALUE_ONLY]
EXPECT_KEYS = [k for k in FULL_KEYS if k[0] != 'past_the_end']      # k_sourcewise_expect writes bins: it has no walk
CURVATURE_KEYS = [k for k in FULL_KEYS if k[0] != 'load_forms']

Case = namedtuple('Case', 'family name model z rs ds counts real tiles')


def row_bins(tiles):
    """a row of `tiles` tiles whose last tile is 100 bins short"""
    return tiles * TILE - 100


def bins_of(family):
    return {'load_forms': LOAD_B, 'chunked': row_bins(CHUNKED_TILES), 'striding': row_bins(STRIDING_TILES),
            'past_the_end': row_bins(PAST_TILES)}[family]


def n_tiles(B):
    return (B + TILE - 1) // TILE


def own_axes(family, name):
    """-> (anchors per axis, own axes per source): CLASS_OWN's class on four axes of two anchors; on the longest rows `s2_e1` keeps
    the one axis it uses (three rows in all)"""
    own = [tuple(o) for o in toy_cases.CLASS_OWN[name]]
    if family in ('striding', 'past_the_end') and name == 's2_e1':
        used = sorted({i for o in own for i in o})
        return (2,) * len(used), [tuple(used.index(i) for i in o) for o in own]
    return (2, 2, 2, 2), own


def make_case(family, name):
    """-> Case; the same arrays on every call"""
    B = bins_of(family)
    rng = np.random.default_rng(sum((family + name).encode()) + 8200)
    n_anchor, own = own_axes(family, name)
    model = fo.random_model(rng, n_anchor, own, B, zero_quarter=(1,))
    centre = np.array([0.5 * (g[0] + g[-1]) for g in model['anchor_z']])
    scale = PER_BIN * B / fo.expectation(model, centre, np.ones(len(own))).sum()
    model['mus'] = [m * scale for m in model['mus']]
    z, rs = toy_cases.box_points(model, rng, 2)
    mu = np.stack([fo.expectation(model, z[t], rs[t]) for t in range(2)])
    # drawn again until more than half of the bins of EVERY tile are filled: the first draw on the long rows, a few on the
    # three-bin last tile of B = 1027
    for _ in range(64):
        counts = rng.poisson(mu).astype(float)
        real = mu * rng.uniform(0.4, 1.7, mu.shape)
        for t in range(2):                                  # a quarter of the bins at exactly 0, as sourcewise_real_oracle's sets
            real[t, rng.permutation(B)[:B // 4]] = 0.0
        if all(np.all(2 * filled > size) for filled, size in (filled_per_tile(counts), filled_per_tile(real))):
            break
    else:
        raise AssertionError('%s %s: no draw fills every tile' % (family, name))
    return Case(family, name, model, z, rs, np.arange(2, dtype=np.int64), counts, real, n_tiles(B))


def filled_per_tile(data):
    """data [T, B] -> (non-zero bins [T, tiles], bins [tiles]) of every 512-bin tile"""
    T, B = data.shape
    tiles = n_tiles(B)
    padded = np.zeros((T, tiles * TILE))
    padded[:, :B] = data
    size = np.minimum(TILE, B - TILE * np.arange(tiles))
    return np.count_nonzero(padded.reshape(T, tiles, TILE), axis=2), size


def walk(tiles, chunks, nbx=None):
    """ItemTiles replayed on the blocks of FacBatch::run: -> (visits [tiles], steps past the end of a ragged last chunk, the set
    of the blocks' trip counts, the tiles a block would lose if it stopped at its first step past the end)"""
    nbx = min(tiles, FAC_BLOCKS) if nbx is None else nbx
    ch = chunks if chunks > 1 and tiles >= CHUNK_MIN_TILES * chunks else 1
    per_chunk = (tiles + ch - 1) // ch
    lt = np.arange(per_chunk * ch)                          # every step of every block: block lt % nbx takes it on trip lt // nbx
    t = (lt % ch) * per_chunk + lt // ch if ch > 1 else lt
    valid = t < tiles
    visits = np.bincount(t[valid], minlength=tiles)
    first_past = np.full(nbx, len(lt))                      # per block: its first step past the end
    np.minimum.at(first_past, lt[~valid] % nbx, lt[~valid])
    behind = int(np.count_nonzero(valid & (lt > first_past[lt % nbx])))
    trips = set(np.bincount(lt % nbx, minlength=nbx).tolist())
    return visits, int(np.count_nonzero(~valid)), trips, behind
