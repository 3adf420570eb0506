"""The inputs of the event-toy tests of source-wise models (bi_sourcewise_simulate_event_toys), shared by the host and the GPU
tests.  Test infrastructure only: NumPy, toy_oracle and factored_oracle; nothing is imported from blueice_amd.

Shapes: toy_replay_cases.SIM_EDGES at k = 1, 2, 3 analysis dimensions (B = 16, 80, 400) and one 1-D row of B = 1025 bins (odd,
three tiles).  Sources own [(0,), (1, 2), (), (0, 1, 2)] on anchors (3, 2, 3); factored_oracle.random_model's templates (source 1
exactly zero in a quarter of the bins) divided by the bin volumes, so that the rows are densities.  The rates at the truth are
(3, 400, 0, 5000): inversion, PTRS twice and an empty source, about 5.4 k events per toy (eleven tiles).  The class cases put
every kernel class of sourcewise_walk_cases.FAMILIES['load_forms'] + ['s4_e2'] on the 1-D B = 16 row with the rates
(3, 400, 0, 60) repeated over the sources.

The oracle of toy D at a truth is toy_oracle.simulate_events(dens, edges, rates, toy_seed(seed, D)) with dens the factored
specification in NumPy, sum_c w_c p_s,c per source.  The device's fma chain differs from it by a few ulp per bin, about 2^-51 of
the total in the running sums: far inside the oracle's 2^-42 bisection band."""
import numpy as np

import factored_oracle as fo
import sourcewise_toy_cases as toy_cases
import sourcewise_walk_cases as wc
import toy_oracle as to
import toy_replay_cases as trc

SEED = trc.SEED
TILE = 512
N_ANCHOR, OWN = (3, 2, 3), [(0,), (1, 2), (), (0, 1, 2)]
RATES = (3.0, 400.0, 0.0, 5000.0)
CLASS_RATES = (3.0, 400.0, 0.0, 60.0)
SHAPES = {'k1': trc.SIM_EDGES[:1], 'k2': trc.SIM_EDGES[:2], 'k3': trc.SIM_EDGES[:3], 'k1_B1025': [np.linspace(-4.0, 4.0, 1026)]}
CLASSES = list(wc.FAMILIES['load_forms']) + ['s4_e2']
CLASS_OWN = dict(toy_cases.CLASS_OWN, s4_e2=[(0, 1), (2,), (), (1, 3)])     # (test_sourcewise_sampler_gpu.OWN_4_2)
NAMES = list(SHAPES) + ['class_' + c for c in CLASSES]
OFFSETS = (0, 2 ** 32 - 2)                  # toy_offset of the replayed calls: the second crosses the low word of the toy number
T_REPLAY = 3


def toy_seed(seed, D):
    """include/blueice_hip.h, bi_simulate_event_toys: the seed of toy D of the seed's ensemble"""
    m = (1 << 64) - 1
    x = (int(seed) + (int(D) + 1) * 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _cell(g, z):
    n = len(g)
    k = n - 2 if z == g[n - 1] else min(max(int(np.searchsorted(g, z, side='right')) - 1, 0), n - 2)
    return k, (z - g[k]) / (g[k + 1] - g[k])


def corners(model, s, z):
    """-> [(w_c, own anchor index tuple)] of source s at z: the corner's bit of the first own axis most significant, w_c the
    product of t or 1 - t in own-axis order from 1.0 (include/blueice_hip.h, bi_eval_factored)"""
    own = model['own'][s]
    cells = [_cell(np.asarray(model['anchor_z'][i], dtype=float), float(z[i])) for i in own]
    out = []
    for c in range(1 << len(own)):
        w, idx = 1.0, []
        for j, (k, t) in enumerate(cells):
            up = (c >> (len(own) - 1 - j)) & 1
            idx.append(k + up)
            w = w * (t if up else 1 - t)
        out.append((w, tuple(idx)))
    return out


def mus_at(model, z):
    """M_s(z) [S]: left to right from 0.0"""
    out = np.zeros(len(model['own']))
    for s in range(len(model['own'])):
        v = 0.0
        for w, idx in corners(model, s, z):
            v = v + float(np.asarray(model['mus'][s])[idx]) * w
        out[s] = v
    return out


def densities_at(model, z):
    """dens [S, B] = sum_c w_c p_s,c: the factored specification in NumPy"""
    return np.array([sum(w * np.asarray(model['ps'][s], dtype=float)[idx] for w, idx in corners(model, s, z))
                     for s in range(len(model['own']))])


def rates_at(model, z, rs):
    """r_s = M_s(z) rs_s, as the library forms it"""
    return mus_at(model, z) * np.asarray(rs, dtype=float)


def scale_for(model, z, rates):
    """rate scales that put the rates at z at `rates` (to a rounding; the oracle is given rates_at's)"""
    return np.asarray(rates, dtype=float) / mus_at(model, z)


def make_case(name, n_truths=1):
    """-> dict(name, edges, model, z [H, d], rs [H, S]); the same arrays on every call.  The rows of the model are densities over
    `edges`; truth h has the case's rates scaled by 1, 0.8, 1.25, ..."""
    rng = np.random.default_rng(sum(name.encode()) + 9100)
    if name.startswith('class_'):
        edges, n_anchor, own = SHAPES['k1'], (2, 2, 2, 2), [tuple(o) for o in CLASS_OWN[name[6:]]]
        target = np.array([CLASS_RATES[s % 4] for s in range(len(own))])
    else:
        edges, n_anchor, own, target = SHAPES[name], N_ANCHOR, OWN, np.array(RATES)
    edges = [np.asarray(e, dtype=float) for e in edges]
    vol = to.bin_volumes(edges)
    model = fo.random_model(rng, n_anchor, own, len(vol), zero_quarter=(1,))
    model['ps'] = [p / vol for p in model['ps']]
    g = model['anchor_z']
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    z = lo + (hi - lo) * rng.uniform(0.05, 0.95, (n_truths, len(g)))
    factor = np.array([1.0, 0.8, 1.25, 0.9, 1.1])[np.arange(n_truths) % 5]
    rs = np.array([scale_for(model, z[h], target * factor[h]) for h in range(n_truths)])
    return dict(name=name, edges=edges, model=model, z=z, rs=rs)


def oracle_toy(case, h, seed, D, dens=None):
    """the Replay of toy D of the seed's ensemble at truth h"""
    dens = densities_at(case['model'], case['z'][h]) if dens is None else dens
    return to.simulate_events(dens, case['edges'], rates_at(case['model'], case['z'][h], case['rs'][h]), toy_seed(seed, D))


def check_oracle_alone(name):
    """the undecided share of the oracle's own draws on the replayed toys of a case stays within toy_oracle.CAP -> [(draws,
    undecided)]"""
    case = make_case(name)
    dens = densities_at(case['model'], case['z'][0])
    out = []
    for off in OFFSETS:
        for t in range(T_REPLAY):
            rep = oracle_toy(case, 0, SEED, off + t, dens)
            assert rep.undecided <= to.CAP * rep.draws, (name, off + t, rep.undecided, rep.draws)
            out.append((rep.draws, rep.undecided))
    return out


# the layout test: one source of rate TILE at truth 0 (set lengths on both sides of a tile), nothing at truth 1
LAYOUT_RATES = (float(TILE), 0.0, 0.0, 0.0)
LAYOUT_TOYS = 12


def layout_counts(case):
    """the oracle's events per source of the layout test's toys at truth 0: [LAYOUT_TOYS, S]"""
    rates = rates_at(case['model'], case['z'][0], scale_for(case['model'], case['z'][0], LAYOUT_RATES))
    out = np.zeros((LAYOUT_TOYS, len(rates)))
    for t in range(LAYOUT_TOYS):
        for s, r in enumerate(rates):
            if r > 0.0:
                n, und = to.event_count(float(r), toy_seed(SEED, t) ^ to.SIM_COUNT_KEY, [s])
                assert not und[0]
                out[t, s] = n[0]
    return out
