"""The case table of the scan-geometry tests (tests/scan_geometry_cases.py) on the CPU.  At every case a plain float64
evaluation and float64 emulations of the two reassociations the matrix-core scan kernels make -- n log of the product of a
64-bin strip's expectations in count order (dense rows and compacted rows), and the logarithm of the product mu^n over a lane's
four bins with -sum mu taken as sum_k coef_k rowsum_k -- stay within the exact oracle's bound at C_POISSON, so a correct kernel
can; the bound rejects every mutant of the count-order emulation at every case that can express it; and no prototype's sign
of an expectation is undecided.  Run with -s for the worst |err| / (2^-52 cond) per emulation."""
import numpy as np
import pytest

import derivative_oracle as do
import scan_geometry_cases as sg

CASES = sg.every_case()
# (cases whose interesting prototypes give nan / -inf: those patterns are asserted exactly on the device, not through the bound)
BOUND_CASES = [(n, m) for n, m in CASES if n not in ('negative dense', 'negative sparse', 'exact zero expectation')]
WORST = {}
REJECTED = {m: [] for m in sg.MUTANTS}
SKIPPED = {m: [] for m in sg.MUTANTS}


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    if WORST:
        print('\nemulations, worst |err| / (2^-52 cond) over all cases (C = %d):' % do.C_POISSON)
        for k in sg.EMULATIONS:
            hits = {n: v for (e, n), v in WORST.items() if e == k}
            if hits:
                worst = max(hits, key=hits.get)
                print('  %-32s %.3g (%s)' % (k, hits[worst], worst))
        for m in sg.MUTANTS:
            print('  mutant %-44s rejected at %d cases, not expressible at %d' % (m, len(REJECTED[m]), len(SKIPPED[m])))


def prototypes_checked(c):
    """Every prototype of the small pools; of each cell's pool the first few where the rows are long or wide."""
    heavy = c.B * c.NS > 20000
    return [int(i) for pool in c.pool for i in (pool[:4] if heavy else pool)]


@pytest.mark.parametrize('name,make', CASES, ids=[n for n, _ in CASES])
def test_emulations_stay_inside_the_bound(name, make):
    c = make()
    for i in prototypes_checked(c):
        for ds in range(c.T):
            want, cond = c.oracle(i, ds)
            if c.sign_class(i) == 'negative' or not np.isfinite(want):
                continue                                   # nan / -inf are asserted exactly on the device, not through the bound
            for which in sg.EMULATIONS:
                got = sg.emulate(c, which, i, ds)
                q = do.check_entries(got, want, cond, do.C_POISSON, '%s prototype %d dataset %d, %s' % (name, i, ds, which))
                WORST[(which, name)] = max(WORST.get((which, name), 0.0), q)


@pytest.mark.parametrize('name,make', BOUND_CASES, ids=[n for n, _ in BOUND_CASES])
def test_every_expressible_mutant_is_rejected(name, make):
    c = make()
    for mname, results in sg.mutant_values(c).items():
        if results is None:
            SKIPPED[mname].append(name)
            continue
        ratios = []
        for i, v in results:
            want, cond = c.oracle(i)
            ratios.append(float(do.ratio(v, want, cond)))
        assert max(ratios) > do.C_POISSON, '%s: the mutant "%s" stays inside the bound (ratio %.3g)' % (name, mname, max(ratios))
        REJECTED[mname].append(name)


def test_every_mutant_is_rejected_somewhere():
    for name, make in BOUND_CASES:
        c = make()
        for mname, results in sg.mutant_values(c).items():
            if results is not None and name not in REJECTED[mname]:
                i, v = results[0]
                if float(do.ratio(v, *c.oracle(i))) > do.C_POISSON:
                    REJECTED[mname].append(name)
    missing = [m for m in sg.MUTANTS if not REJECTED[m]]
    assert not missing, 'no case of the table expresses and rejects %s' % missing


@pytest.mark.parametrize('name,make', CASES, ids=[n for n, _ in CASES])
def test_no_prototype_has_an_undecided_sign(name, make):
    c = make()
    classes = [c.sign_class(int(i)) for pool in c.pool for i in pool]
    assert 'undecided' not in classes, '%s: prototypes %s' % (name, [i for i, k in enumerate(classes) if k == 'undecided'])
    if c.allow_negative.any():
        assert 'negative' in classes and 'positive' in classes
        # the certainly-negative prototypes are exactly those given the large negative rate
        assert [k == 'negative' for k in classes] == list(c.neg_rate)
    else:
        assert set(classes) == {'positive'}


def test_the_table_holds_the_shapes_the_kernels_branch_on():
    names = [n for n, _ in CASES]
    assert len(names) == len(set(names))
    for B in sg.FALLBACK_BINS + sg.BINS:
        assert sg.bins_case(B).B == B
    tiles = {(-(-B // sg.TILE), (B - 1) % sg.TILE + 1) for B in sg.BINS}
    assert {(t, f) for t in (1, 2, 5) for f in (sg.TILE, 1, sg.TILE - 1)} <= tiles | {(1, 1)}
    # every KG = 1 .. 8, with and without padding streams
    assert {(NS + 3) // 4 for NS in sg.STREAMS} == set(range(1, 9))
    assert {NS % 4 == 0 for NS in sg.STREAMS} == {True, False}
    for NS in sg.STREAMS:
        c = sg.stream_case(NS)
        assert c.S * 2 ** c.d == NS and all(len(p) % 2 == 1 for p in c.pool) and len(c.pz) <= 40
    # the strip classes of the dense variants, in count order
    cls = lambda c: set(sg.Strips(c, 0).cls)
    assert cls(sg.dense_case('poisson')) == {'U', 'M'}
    assert cls(sg.dense_case('runs')) == {'U', 'M', 'Z'}
    assert set(sg.Strips(sg.dense_case('all_mixed'), 0).cls[:-1]) == {'M'}
    one = sg.Strips(sg.dense_case('one_count'), 0).cls
    assert list(one).count('M') == 1 and one[-1] == 'M'
    assert set(sg.Strips(sg.dense_case('one_count', 2560), 0).cls) == {'U'}
    runs = sg.dense_case('runs').counts[0]
    assert (runs == 1).sum() == 1 and (runs == 1e6).sum() == 1 and (runs == 0).sum() == 130
    for kind in sg.SPARSE_DATA:
        for nnz in sg.SPARSE_NNZ:
            c = sg.sparse_case(kind, nnz)
            n = c.counts[0]
            assert (n > 0).sum() == nnz and 8 * nnz <= c.B and n.max() <= (2 if kind == 'ones_twos' else 12)
    # per-cell point counts: every quad remainder of the item count, last items with 1, 15 and 16 live slots
    items = [-(-n // 16) for n in sg.CELL_POINTS]
    assert {k % 4 for k in items} == {0, 1, 2, 3} and {n % 16 for n in sg.CELL_POINTS} >= {0, 1, 15}
    assert any(n % 16 == 1 and (n // 16) % 4 == 2 for n in sg.CELL_POINTS)
