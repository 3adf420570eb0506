"""The cases of tests/batch_seam_cases.py cross the seams they claim: checked on the CPU from the formulas restated there, so that
a case that silently stops crossing its seam (a constant of the host code moved, a size edited) fails here and not only on the
device, where test_batch_seams_gpu.py compares `last_point_pieces` with the same figures."""
import numpy as np
import pytest

import batch_seam_cases as bsc

CASES = bsc.CASES


def test_the_figures_of_the_restated_formulas():
    """the slots and seam positions of the two source classes, worked out by hand from bi_common.h and bi_factored.h"""
    assert bsc.source_class(bsc.OWN) == (4, 2) and bsc.source_class(bsc.MODEL_OWN['panels']) == (8, 2)
    assert bsc.slots(bsc.OWN, 'hess') == [95] and bsc.slots(bsc.OWN, 'fisher') == [91] and bsc.slots(bsc.OWN, 'grad') == [13]
    assert bsc.slots(bsc.MODEL_OWN['panels'], 'hess') == [54, 57, 93, 129]
    assert bsc.padded_bins(bsc.B_ROWS) == 128 * 512 and bsc.B_ROWS % 512 != 0
    assert [bsc.per_call(bsc.B_ROWS, n) for n in (95, 91, 13, 2, 1)] == [689, 720, 5041, 32768, 65536]
    assert [bsc.per_call(bsc.B_PANELS, n) for n in (54, 57, 93, 129)] == [9709, 9198, 5637, 4064]
    assert bsc.per_call(bsc.B_TILE, 95) > bsc.ITEM_CHUNK            # one block per item: only the launch limit cuts
    assert bsc.expect_chunk(10 ** 6, 3 * 600) == 4660 and bsc.expect_chunk(10 ** 6, 63) == bsc.LAUNCH_ITEMS
    assert bsc.expect_chunk(10 ** 6, bsc.padded_bins(bsc.B_ROWS)) == 128
    assert bsc.coarse_chunk_one_row(10 ** 6, 1, 600, 600) == 13981 == bsc.list_chunk(10 ** 6, 600)
    assert bsc.coarse_chunk_one_row(10 ** 6, 4, 63, 9) == bsc.LAUNCH_ITEMS


def test_every_entry_point_has_a_case():
    assert sorted({c.entry for c in CASES}) == sorted(bsc.ENTRY_POINTS)
    crossed = {}
    for c in CASES:
        crossed.setdefault(c.entry, set()).update(c.levels)
    for entry in ('bi_eval_factored', 'bi_eval_sourcewise_gof', 'bi_eval_sourcewise_real', 'bi_eval_sourcewise_hess', 'bi_eval_sourcewise_fisher'):
        assert crossed[entry] == {'outer', 'inner'}, entry         # both levels of FacBatch::run
    both = bsc.BY_NAME['sw_value_both']
    assert both.levels == dict(outer=[65536], inner=[65535]) and both.P == 65541


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_the_case_crosses_its_seams(case):
    live = bsc.live_of(case.P, case.dead)
    assert len(live) == case.n_live and case.seams
    number = {int(p): i for i, p in enumerate(live)}                # point index -> live number
    probes = set(int(p) for p in case.probes)
    assert probes <= set(number), 'a probe is a dead point'
    for label, seams in case.levels.items():
        assert seams, label
        for s in seams:
            # P lies beyond the seam: two live items on either side of it, and they are probes
            assert 2 <= s and s + 2 <= case.n_live, (label, s)
            for i in (s - 2, s - 1, s, s + 1):
                assert int(live[i]) in probes, (label, s, i)
        assert case.level_pieces[label] >= 2, label
    # the dead points precede the first seam, so live number and point index differ on both sides of every seam
    for p in case.dead:
        assert p < live[case.seams[0] - 2]
        assert {p - 1, p + 1} - set(case.dead) <= probes
    if case.dead:
        assert all(live[s] == s + len(case.dead) for s in case.seams)
        assert list(case.status()[list(case.dead)]) == [bsc.ST_OUT_OF_BOUNDS, bsc.ST_UNPHYSICAL] and case.status().sum() == 3
    assert {0, case.P - 1} <= probes
    assert case.pieces >= 2 and case.pieces >= max(case.level_pieces.values())
    if 'passes' in case.extra:          # FacBatch::run: every pass ends a piece, every seam of a pass begins one
        per_pass = [bsc.factored_levels(case.n_live, bsc.MODEL_BINS[case.model_key], [nsl]) for nsl in case.extra['passes']]
        assert case.pieces == sum(1 + len(lv['outer']) + len(lv['inner']) for lv, _, _ in per_pass)
        assert case.pieces == sum(p for _, _, p in per_pass)
    else:
        assert case.pieces == len(case.seams) + 1 and case.seams == [case.extra['chunk'] * k for k in range(1, case.pieces)]


@pytest.mark.parametrize('case', [c for c in CASES if c.dead and c.P < 20000], ids=repr)
def test_the_points_are_inside_the_box_but_for_the_dead_ones(case):
    model = bsc.model_of(case.model_key)
    z, rs = case.points()
    lo, hi = np.array([a[0] for a in model['anchor_z']]), np.array([a[-1] for a in model['anchor_z']])
    inside = np.all((z >= lo) & (z <= hi), axis=1)
    assert list(np.flatnonzero(~inside)) == [bsc.OUTSIDE]
    assert list(np.flatnonzero((rs < 0).any(axis=1))) == [bsc.UNPHYSICAL]
    again = case.points()
    assert np.array_equal(again[0], z) and np.array_equal(again[1], rs)
