"""Inputs and helpers of the source-wise toy / goodness-of-fit / expected-counts tests (test_sourcewise_toys_host.py on the CPU,
test_sourcewise_toys_gpu.py on the device): the smallest shapes at which the kernels can go wrong.  No test lives here.

    small models     factored_oracle.random_model at B = 63 (less than one tile), 1001 and 1027 (a ragged last tile; an odd B: the
                     last bin pair has one bin), and a B = 1 model
    class models     the nine (source slots, own axes) classes of test_factored_gpu.py at B = 1027: every kernel instantiation
    zero_both_sides  built by hand: EVERY source is zero in the same bins (mu_b = 0 exactly there), rates scaled so that mu_b lies
                     on both sides of 10 (both Poisson branches of the generator)

Every input comes with three truth points (z [3, d], rs [3, S]) inside the box, the last on its upper edge."""
import numpy as np

import factored_oracle as fo

SEED = 0x5EED50C1
N_TOYS = (3, 0, 5)                      # toys per truth of the H = 3 calls: a truth without toys in the middle
TOY_OFFSETS = (0, 2 ** 32 - 2)          # the second: dataset numbers cross 2^32 inside the call
LAUNCH_TOYS = 32770                     # a generator launch takes 32 768 toys: two more cross into a second one
LAUNCH_BOUNDARY_TOYS = (0, 1, 32766, 32767, 32768, 32769)
N_ANCHOR, OWN = (3, 2, 4), ((0,), (1, 2), ())
_TRIPLES = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
CLASS_OWN = {'e3x8': [_TRIPLES[s % 4] for s in range(8)], 'mixed': [(), (2,), (0, 3), (0, 1, 2)],
             'mixed_padded': [(), (2,), (0, 3), (0, 1, 2), (1, 3)],
             's2_e1': [(1,), ()], 's2_e2': [(0, 3), (2,)], 's2_e3': [(0, 1, 2), (3,)], 's4_e1': [(0,), (3,), ()],
             's8_e1': [(s % 4,) if s != 5 else () for s in range(8)],
             's8_e2': [[(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (2,), ()][s] for s in range(8)]}
CLASS_CASES = sorted(CLASS_OWN)
SMALL_CASES = ['B63', 'B1001', 'B1027', 'B1']
ALL_CASES = SMALL_CASES + CLASS_CASES + ['zero_both_sides']
ZERO_BINS = np.arange(0, 203, 5)        # the bins of `zero_both_sides` that no source fills


def box_points(model, rng, n):
    """n points inside the cells, the last on the upper edge of the box -> (z [n, d], rs [n, S])"""
    g = model['anchor_z']
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    z = lo + (hi - lo) * rng.uniform(0.03, 0.97, (n, len(g)))
    z[n - 1] = hi
    return z, rng.uniform(0.5, 1.6, (n, len(model['own'])))


def make_case(name):
    """-> (model, z [3, d], rs [3, S]) of one named input; the same arrays on every call"""
    rng = np.random.default_rng(sum(name.encode()) + 7000)
    if name == 'B1':
        model = fo.random_model(rng, N_ANCHOR, OWN, 1)
    elif name in SMALL_CASES:
        model = fo.random_model(rng, N_ANCHOR, OWN, int(name[1:]), zero_quarter=(1,))
    elif name in CLASS_OWN:
        model = fo.random_model(rng, (2, 2, 2, 2), CLASS_OWN[name], 1027, zero_quarter=(1,))
    elif name == 'zero_both_sides':
        model = fo.random_model(rng, N_ANCHOR, OWN, 203)
        for s in range(len(OWN)):
            p = model['ps'][s]
            p[..., ZERO_BINS] = 0.0
            p /= p.sum(axis=-1, keepdims=True)
    else:
        raise KeyError(name)
    z, rs = box_points(model, rng, 3)
    if name == 'zero_both_sides':
        live = np.setdiff1d(np.arange(203), ZERO_BINS)
        for h in range(3):                                      # the rates scaled: half of the live bins on either side of 10
            rs[h] *= 10.0 / np.median(fo.expectation(model, z[h], rs[h])[live])
    return model, z, rs


def exact_expectation(model, z, rs):
    """-> (mu [B], per source [S, B]) in long double: factored_columns' column 0 (the float64 coefficients every route starts
    from) times the template rows, summed in extended precision.  All terms are non-negative: cond = the value."""
    coef, rows = fo.factored_columns(model, z, rs)
    S, B = len(model['own']), fo.n_bins(model)
    per = np.zeros((S, B), dtype=np.longdouble)
    for k, (s, idx) in enumerate(rows):
        per[s] += np.longdouble(coef.v[0][k]) * np.asarray(model['ps'][s], dtype=float)[idx].astype(np.longdouble)
    return per.sum(axis=0), per


def truth_of_toy(n_toys):
    return np.repeat(np.arange(len(n_toys)), n_toys)


def upload(model, counts=None):
    """A SourceWiseContext holding `model` (anchors in any order) and, when given, counts [B] or [T, B]"""
    from blueice_amd.source_wise import SourceWiseContext
    ctx = SourceWiseContext(0)
    B = fo.n_bins(model)
    ctx.begin_model(model['anchor_z'], len(model['own']), B, model['own'])
    for s in range(len(model['own'])):
        rows = np.asarray(model['ps'][s]).reshape(-1, B)
        mus = np.asarray(model['mus'][s]).reshape(-1)
        for k in np.random.default_rng(s).permutation(len(rows)):
            ctx.set_anchor(s, int(k), rows[k], mus[k])
    ctx.end_model()
    if counts is not None:
        ctx.set_counts(counts)
    return ctx
