"""The case table of the value-geometry tests (tests/value_geometry_cases.py) on the CPU: at every shape a plain float64 numpy
evaluation of the likelihood value stays within the exact oracle's bound (so a correct float64 kernel can), and the bound
rejects every mutant of that evaluation -- a bin dropped or counted twice, a tile dropped, the padding lanes counted, two
tiles exchanged between two points, the empty-bin branch taken at n = 1.  A shape at which a one-bin mutant slipped under
C 2^-52 cond would have to leave the table.  Run with -s for the reference's own worst |err| / (2^-52 cond)."""
import numpy as np
import pytest

import derivative_oracle as do
import value_geometry_cases as vg

WORST = {}
CASES = vg.every_case()


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    if WORST:
        print('\nplain numpy evaluation, worst |err| / (2^-52 cond) (C = %d): %.3g over all shapes' % (do.C_POISSON, max(WORST.values())))
        for k in sorted(WORST):
            print('  %-24s %.3g' % (k, WORST[k]))


def poisson_oracle(c, z, r):
    """The plain binned value of every model of the table (a Beeston-Barlow model's templates serve as an ordinary model here)."""
    o = do.derivatives(c.model, z, r, counts=c.counts[0], hessian=False)
    return o['ll'], o['ll_cond']


@pytest.mark.parametrize('name,make', CASES, ids=[n for n, _ in CASES])
def test_plain_evaluation_stays_inside_the_bound_and_every_mutant_fails(name, make):
    c = make()
    zs, rs = vg.standard_points(c)
    want = [poisson_oracle(c, zs[p], rs[p]) for p in range(len(rs))]
    worst = 0.0
    for p in range(len(rs)):
        got = vg.numpy_value(c, zs[p], rs[p])
        worst = max(worst, do.check_entries(got, want[p][0], want[p][1], do.C_POISSON, '%s point %d' % (name, p)))
    WORST[name] = worst                 # (the device's margin under C is judged against this figure)
    # points 0 (lower cell) and 2 (upper cell; without a shape axis: other rates)
    mutants = vg.mutant_values(c, zs[0], rs[0], zs[2], rs[2])
    assert set(mutants) == set(vg.MUTANTS)
    for mname, results in mutants.items():
        ratios = [float(do.ratio(v, want[(0, 2)[i]][0], want[(0, 2)[i]][1])) for i, v in results]
        assert max(ratios) > do.C_POISSON, '%s: the mutant "%s" stays inside the bound (ratio %.3g)' % (name, mname, max(ratios))


def test_the_table_holds_the_shapes_the_kernels_branch_on():
    tiles = sorted({make().n_tiles for _, make in CASES})
    for t in vg.TILE_COUNTS:
        assert t in tiles
    for t, f in vg.TILE_SHAPES:
        c = vg.tile_case(t, f)
        assert c.n_tiles == t and (c.B - 1) % vg.TILE + 1 == f
        n = c.counts[0]
        assert n.max() <= 255 and ((n == 0).any() or c.B == 1)
        if c.B > 400:
            assert (n[300:390] == 0).all() and n[vg.N_ONE_BIN] == 1
    assert vg.single_big_case().n_tiles > 1024 and vg.seam_case().n_tiles == 1
