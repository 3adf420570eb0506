"""Inputs and arithmetic of the host sub-batch seam tests: shared by tests/test_batch_seams_gpu.py (which runs every case on the
device) and tests/test_batch_seam_cases.py (which shows on the CPU, from the formulas restated here, that every case crosses the
seams it claims).  No test lives here.

Every entry point that takes P points cuts its live items into device pieces on the host, on up to two levels:

    launch limit   65 535 items per launch of run_item_chunks (bi_items.h) and of bi_set_asimov_counts (bi_real.h); 32 768 per
                   launch of the calls that write bins or cells (bi_gof.h, bi_coarse.h, kSwLaunchItems of bi_sourcewise.h)
    memory cap     2^23 doubles in flight: FacBatch::run (bi_factored.h) gives one run_item_chunks call
                   per_call = max(1, 2^23 / (nbx nsl)) items, nbx = min(Bp / 512, 1024) blocks per item and nsl result slots;
                   bi_expected_counts 2^23 / (R B) points, bi_sourcewise_expected_counts 2^23 / (R Bp); coarse_chunk (bi_coarse.h)
                   2^23 / max(R CR nsplit Lx, R C), the list form of bi_coarse_counts 2^23 / C

A `seam` is the LIVE index of the first item of a piece (other than the first piece).  The read-only parameter
`last_point_pieces` counts the pieces of the most recent call; `pieces` is what the formulas give for the case.

Slots per item (bi_common.h): value 1, goodness of fit 2, gradient 1 + SC (1 + EM); the curvature calls launch once per Gram
panel of PS sources, panel p holding the pairs of Gram rows [p PS W, (p + 1) PS W) with W = 1 + EM, panel 0 also the NL linear
slots (Hessian: 1 + SC W + SC EM (EM - 1) / 2, information: 1 + SC W).  SC = 2, 4 or 8 source slots, EM = max(1, own axes).

Models: factored_oracle.random_model (source-wise) and fisher_fixtures.synthetic_model (grid), nothing else.  Every case with
points has two dead ones before its first seam -- OUTSIDE (z left of the anchor box) and UNPHYSICAL (a negative rate scale) -- so
that live index and point index differ on both sides of every seam.  The calls that take truths (Asimov sets, the generator)
refuse a dead truth, and bi_coarse_counts takes dataset indices: those cases have no dead item.  Probes: the two live items on
either side of every seam, the first and the last point, and the neighbours of the dead points."""
import numpy as np

import factored_oracle as fo
import sourcewise_toy_cases as toy_cases
from fisher_fixtures import synthetic_model

TILE = 512                       # kTile
FAC_BLOCKS = 1024                # kFacBlocks
IN_FLIGHT = 2 ** 23              # kFacPartialDoubles, kSwExpectDoubles, the caps of bi_gof.h and bi_coarse.h
ITEM_CHUNK = 65535               # run_item_chunks, bi_set_asimov_counts
LAUNCH_ITEMS = 32768             # kSwLaunchItems, bi_expected_counts, coarse_chunk

OUTSIDE, UNPHYSICAL = 3, 7       # the dead points of every case that has points
ST_OUT_OF_BOUNDS, ST_UNPHYSICAL = 1, 2
SEED = 0x5EA35
TOY_SEED = toy_cases.SEED

N_ANCHOR, OWN = toy_cases.N_ANCHOR, toy_cases.OWN            # (3, 2, 4) anchors; S = 3: SC = 4, EM = 2
B_ROWS = 128 * TILE - 100        # 128 blocks per item, a ragged last tile
B_PANELS = 16 * TILE - 100       # the s8_e2 class (SC = 8, EM = 2: four Gram panels) at 16 blocks per item: the oracle's cost per
                                 # probe grows with B, the device's work at the seam does not
B_TILE = 63                      # one tile: one block per item


# ---- the formulas, restated from the header comments --------------------------------------------------------------------------

def padded_bins(B):
    return max(TILE, (B + TILE - 1) // TILE * TILE)


def source_class(own):
    S = len(own)
    return (2 if S <= 2 else 4 if S <= 4 else 8), max(1, max(len(o) for o in own))


def slots(own, call):
    """-> the result slots per item of every launch pass of a source-wise call (one pass, or one per Gram panel)"""
    SC, EM = source_class(own)
    W = 1 + EM
    if call == 'value':
        return [1]
    if call == 'gof':
        return [2]
    if call == 'grad':
        return [1 + SC * W]
    NL = 1 + SC * W + (SC * (EM * (EM - 1) // 2) if call == 'hess' else 0)
    assert call in ('hess', 'fisher')
    PS = SC if SC * W <= 16 else 2 if EM == 2 else 1
    out = []
    for p in range(SC // PS):
        a0, a1 = p * PS * W, (p + 1) * PS * W
        out.append((NL if p == 0 else 0) + a1 * (a1 + 1) // 2 - a0 * (a0 + 1) // 2)
    return out


def per_call(B, nsl):
    """FacBatch::run: the items of one run_item_chunks call"""
    nbx = min(padded_bins(B) // TILE, FAC_BLOCKS)
    return max(1, IN_FLIGHT // (nbx * nsl))


def factored_levels(n_live, B, nsl_list):
    """FacBatch::run over every pass: sub-batches of per_call items (outer), chunks of 65 535 items inside each (inner)
    -> (seams {level: [...]}, the most pieces of one pass {outer: sub-batches, inner: chunks of one sub-batch}, pieces in all)"""
    outer, inner, pieces = set(), set(), 0
    most = dict(outer=0, inner=0)
    for nsl in nsl_list:
        step = per_call(B, nsl)
        most['outer'] = max(most['outer'], (n_live + step - 1) // step)
        for j0 in range(0, n_live, step):
            nj = min(step, n_live - j0)
            most['inner'] = max(most['inner'], (nj + ITEM_CHUNK - 1) // ITEM_CHUNK)
            if j0:
                outer.add(j0)
            for i0 in range(0, nj, ITEM_CHUNK):
                if i0:
                    inner.add(j0 + i0)
                pieces += 1
    return dict(outer=sorted(outer), inner=sorted(inner)), most, pieces


def chunk_level(n_live, chunk):
    """a loop `for (i0 = 0; i0 < n; i0 += chunk)` -> (seams, pieces)"""
    return list(range(chunk, n_live, chunk)), (n_live + chunk - 1) // chunk


def expect_chunk(n_live, per_item):
    """bi_expected_counts (per_item = R B) and bi_sourcewise_expected_counts (per_item = R Bp)"""
    return max(1, min(n_live, LAUNCH_ITEMS, IN_FLIGHT // per_item))


def coarse_chunk_one_row(n_live, R, Lx, C):
    """coarse_chunk for a binning of ONE fine axis: a single fine row, so coarse_geometry gives nsplit = 1 on every device (a
    share keeps at least 4 TY fine rows) and CR = 1"""
    return max(1, min(n_live, LAUNCH_ITEMS, IN_FLIGHT // max(R * Lx, R * C)))


def list_chunk(n, C):
    """the non-empty-bin list form of bi_coarse_counts"""
    return max(1, min(n, LAUNCH_ITEMS, IN_FLIGHT // C))


def live_of(P, dead):
    return np.setdiff1d(np.arange(P), np.asarray(dead, dtype=np.int64))


def probes_of(P, dead, seams):
    """point indices: two live items on either side of every seam, the first and last point, the dead points' neighbours"""
    live = live_of(P, dead)
    want = {0, P - 1}
    for s in seams:
        want.update(int(live[i]) for i in (s - 2, s - 1, s, s + 1))
    for p in dead:
        want.update((p - 1, p + 1))
    return np.array(sorted(want - set(dead)), dtype=np.int64)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

class SeamCase:
    """name, entry (the C entry point), family ('sourcewise' or 'grid'), model_key (which model of `model_of`), P items,
    dead (point indices, () where the call takes none), levels {label: seams}, level_pieces {label: the pieces of that level},
    pieces (the expected last_point_pieces), probes (point indices), and what the entry point needs beyond that (`extra`)."""

    def __init__(self, name, entry, family, model_key, P, levels, level_pieces, pieces, dead=(OUTSIDE, UNPHYSICAL), **extra):
        self.name, self.entry, self.family, self.model_key, self.P = name, entry, family, model_key, P
        self.dead = tuple(dead)
        self.levels = {k: list(v) for k, v in levels.items()}
        self.level_pieces = dict(level_pieces)
        self.pieces = pieces
        self.extra = extra
        self.n_live = P - len(self.dead)
        self.seams = sorted({s for v in self.levels.values() for s in v})
        self.probes = probes_of(P, self.dead, self.seams)

    def __repr__(self):
        return self.name

    def points(self):
        """-> (z [P, d], rs [P, S]) inside the anchor box, but for the dead points; the same arrays on every call"""
        model = model_of(self.model_key)
        rng = np.random.default_rng(SEED + sum(self.name.encode()))
        g = model['anchor_z']
        S = len(model['own']) if self.family == 'sourcewise' else model['mus'].shape[-1]
        lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
        z = lo + (hi - lo) * rng.uniform(0.03, 0.97, (self.P, len(g)))
        rs = rng.uniform(0.5, 1.6, (self.P, S))
        if self.dead:
            z[OUTSIDE, 0] = lo[0] - 1.0
            rs[UNPHYSICAL, 0] = -1.0
        return z, rs

    def status(self):
        st = np.zeros(self.P, dtype=np.int32)
        if self.dead:
            st[OUTSIDE], st[UNPHYSICAL] = ST_OUT_OF_BOUNDS, ST_UNPHYSICAL
        return st


_MODELS = {}


def model_of(key):
    """The models, built once: source-wise 'rows' (B_ROWS bins), 'tile' (B_TILE), 'panels' (s8_e2, B_PANELS); grid 'g63' (d = 1,
    S = 2, B = 63) and 'g600' (d = 1, S = 3, B = 600)"""
    if key not in _MODELS:
        rng = np.random.default_rng(SEED + sum(key.encode()))
        if key == 'rows':
            m = fo.random_model(rng, N_ANCHOR, OWN, B_ROWS, zero_quarter=(1,))
        elif key == 'tile':
            m = fo.random_model(rng, N_ANCHOR, OWN, B_TILE, zero_quarter=(1,))
        elif key == 'panels':
            m = fo.random_model(rng, (2, 2, 2, 2), toy_cases.CLASS_OWN['s8_e2'], B_PANELS, zero_quarter=(1,))
        elif key == 'g63':
            m = synthetic_model(rng, 1, 2, 63)
        elif key == 'g600':
            m = synthetic_model(rng, 1, 3, 600)
        else:
            raise KeyError(key)
        _MODELS[key] = m
    return _MODELS[key]


MODEL_BINS = dict(rows=B_ROWS, tile=B_TILE, panels=B_PANELS, g63=63, g600=600)
MODEL_OWN = dict(rows=OWN, tile=OWN, panels=toy_cases.CLASS_OWN['s8_e2'])
REBIN7 = [0, 7, 14, 21, 28, 35, 42, 49, 56, 63]          # the one axis of 63 fine bins in 9 cells


def _factored(name, entry, key, call, P, crossed):
    """a call through FacBatch::run; crossed: the levels the case claims ('outer', 'inner')"""
    B, own = MODEL_BINS[key], MODEL_OWN[key]
    levels, most, pieces = factored_levels(P - 2, B, slots(own, call))
    assert sorted(k for k, v in levels.items() if v) == sorted(crossed), (name, levels)
    return SeamCase(name, entry, 'sourcewise', key, P, {k: levels[k] for k in crossed}, {k: most[k] for k in crossed}, pieces, call=call,
                    passes=slots(own, call))


def _chunked(name, entry, family, key, P, chunk_of, dead=(OUTSIDE, UNPHYSICAL), **extra):
    """a call with one explicit chunk loop; chunk_of(n_live) -> the chunk"""
    n = P - len(dead)
    seams, pieces = chunk_level(n, chunk_of(n))
    return SeamCase(name, entry, family, key, P, dict(chunk=seams), dict(chunk=pieces), pieces, dead=dead, chunk=chunk_of(n), **extra)


def _build():
    Bp_rows, Bp_tile = padded_bins(B_ROWS), padded_bins(B_TILE)
    out = [
        # -- FacBatch::run: the memory cap (outer), rows of 128 blocks
        _factored('sw_hess_mem', 'bi_eval_sourcewise_hess', 'rows', 'hess', 689 + 8, ['outer']),
        _factored('sw_fisher_mem', 'bi_eval_sourcewise_fisher', 'rows', 'fisher', 720 + 8, ['outer']),
        _factored('sw_grad_mem', 'bi_eval_factored', 'rows', 'grad', 5041 + 8, ['outer']),
        _factored('sw_real_grad_mem', 'bi_eval_sourcewise_real', 'rows', 'grad', 5041 + 8, ['outer']),
        _factored('sw_gof_mem', 'bi_eval_sourcewise_gof', 'rows', 'gof', 32768 + 8, ['outer']),
        # value only: the inner seam at 65 535 and the outer one at 65 536, one item apart
        _factored('sw_value_both', 'bi_eval_factored', 'rows', 'value', 65541, ['outer', 'inner']),
        _factored('sw_real_value_both', 'bi_eval_sourcewise_real', 'rows', 'value', 65541, ['outer', 'inner']),
        # four Gram panels of 54, 57, 93 and 129 slots: four seam positions in one call
        _factored('sw_hess_panels', 'bi_eval_sourcewise_hess', 'panels', 'hess', 10000, ['outer']),
        # -- FacBatch::run: the launch limit (inner), one block per item
        _factored('sw_hess_launch', 'bi_eval_sourcewise_hess', 'tile', 'hess', ITEM_CHUNK + 6, ['inner']),
        _factored('sw_fisher_launch', 'bi_eval_sourcewise_fisher', 'tile', 'fisher', ITEM_CHUNK + 6, ['inner']),
        _factored('sw_gof_launch', 'bi_eval_sourcewise_gof', 'tile', 'gof', ITEM_CHUNK + 6, ['inner']),
        _factored('sw_real_grad_launch', 'bi_eval_sourcewise_real', 'tile', 'grad', ITEM_CHUNK + 6, ['inner']),
        # -- the source-wise calls that write bins or cells
        _chunked('sw_expect_mem', 'bi_sourcewise_expected_counts', 'sourcewise', 'rows', 128 + 8, lambda n: expect_chunk(n, Bp_rows), R=1),
        _chunked('sw_coarse_launch', 'bi_sourcewise_expected_coarse', 'sourcewise', 'tile', LAUNCH_ITEMS + 8,
                 lambda n: coarse_chunk_one_row(n, 1, 63, 9), shape=(63,), groups=[REBIN7], R=1),
        _chunked('sw_coarse_counts_launch', 'bi_sourcewise_coarse_counts', 'sourcewise', 'tile', LAUNCH_ITEMS + 4,
                 lambda n: coarse_chunk_one_row(n, 1, 63, 9), dead=(), shape=(63,), groups=[REBIN7], T=6),
        _chunked('sw_asimov_launch', 'bi_sourcewise_set_asimov_counts', 'sourcewise', 'tile', LAUNCH_ITEMS + 4, lambda n: LAUNCH_ITEMS, dead=()),
        _chunked('sw_toys_launch', 'bi_sourcewise_generate_toys', 'sourcewise', 'tile', LAUNCH_ITEMS + 4, lambda n: LAUNCH_ITEMS, dead=()),
        # -- the grid model
        _chunked('grid_expect_launch', 'bi_expected_counts', 'grid', 'g63', LAUNCH_ITEMS + 8, lambda n: expect_chunk(n, 63), R=1),
        _chunked('grid_expect_mem', 'bi_expected_counts', 'grid', 'g600', 4660 + 8, lambda n: expect_chunk(n, 3 * 600), R=3),
        _chunked('grid_coarse_launch', 'bi_expected_coarse', 'grid', 'g63', LAUNCH_ITEMS + 8, lambda n: coarse_chunk_one_row(n, 1, 63, 9),
                 shape=(63,), groups=[REBIN7], R=1),
        _chunked('grid_coarse_mem', 'bi_expected_coarse', 'grid', 'g600', 13981 + 8, lambda n: coarse_chunk_one_row(n, 1, 600, 600),
                 shape=(600,), groups=[list(range(601))], R=1),
        _chunked('grid_jacobian_launch', 'bi_expected_coarse_jacobian', 'grid', 'g63', LAUNCH_ITEMS + 8,
                 lambda n: coarse_chunk_one_row(n, 4, 63, 9), shape=(63,), groups=[REBIN7], R=4),
        _chunked('grid_coarse_counts_launch', 'bi_coarse_counts', 'grid', 'g63', LAUNCH_ITEMS + 4, lambda n: coarse_chunk_one_row(n, 1, 63, 9),
                 dead=(), shape=(63,), groups=[REBIN7], T=3, form='dense'),
        _chunked('grid_coarse_counts_list_mem', 'bi_coarse_counts', 'grid', 'g600', 13981 + 4, lambda n: list_chunk(n, 600), dead=(),
                 shape=(600,), groups=[list(range(601))], T=6, form='lists'),
        _chunked('grid_asimov_launch', 'bi_set_asimov_counts', 'grid', 'g63', ITEM_CHUNK + 4, lambda n: ITEM_CHUNK, dead=()),
    ]
    assert Bp_tile == TILE
    return out


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every entry point whose seam no other test file crosses
ENTRY_POINTS = ['bi_eval_factored', 'bi_eval_sourcewise_gof', 'bi_eval_sourcewise_real', 'bi_eval_sourcewise_hess', 'bi_eval_sourcewise_fisher',
                'bi_sourcewise_expected_counts', 'bi_sourcewise_expected_coarse', 'bi_sourcewise_coarse_counts', 'bi_sourcewise_set_asimov_counts',
                'bi_sourcewise_generate_toys', 'bi_expected_counts', 'bi_expected_coarse', 'bi_expected_coarse_jacobian', 'bi_coarse_counts',
                'bi_set_asimov_counts']
