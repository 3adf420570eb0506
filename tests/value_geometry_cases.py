"""The models, points and batches of the value-geometry tests: shared by tests/test_value_geometry_gpu.py (which runs them on
the device at every launch geometry) and tests/test_value_geometry_cases.py (which shows on the CPU that a plain float64
evaluation stays inside the oracle's bound at every shape of the table and that the bound rejects every mutant).

Models: S = 2 sources on one shape axis of 3 anchors (-1, 0, 1: two grid cells), or no axis where noted; Poisson data with
every count <= 255 (the narrow form of the counts is eligible), a few empty bins, one run of empty bins, one bin with n = 1.
Oracle results are computed once per (model, dataset, point) and shared (`Case.oracle`)."""
import numpy as np
from scipy.special import gammaln

import derivative_oracle as do
from oracle import blueice_oracle as orc

TILE = 512                       # kTile: bins per tile of k_morph_reduce / k_morph_single

# tile counts around the chunked walk's thresholds (n_tiles >= 64 chunks: 128 for 2 chunks, 192 for 3; 129, 193 and 196 leave the
# last chunk ragged), the last tile full, holding one bin, holding 511
TILE_COUNTS = (1, 2, 9, 127, 128, 129, 191, 192, 193, 196)
LAST_FILL = (TILE, 1, TILE - 1)
TILE_SHAPES = [(t, f) for t in TILE_COUNTS for f in LAST_FILL]


def bins_of(n_tiles, fill):
    return (n_tiles - 1) * TILE + fill


N_ONE_BIN = 3                    # the bin that holds n = 1 (where the model has that many bins)


class Case:
    """One model of the table with its data: .m (SyntheticModel), .model (dense dict for the oracle), .counts [T, B]."""

    def __init__(self, B, n_anchor=(3,), S=2, T=1, bb_source=-1, seed=77):
        from blueice_amd.synthetic import SyntheticModel
        self.m = m = SyntheticModel(S, n_anchor, (B,), seed=seed, bb_source=bb_source)
        self.B, self.T = B, T
        self.model = m.dense_model()
        self.counts = np.stack([edited_counts(m.counts(dense=True, dataset=t), t) for t in range(T)])
        assert self.counts.max() <= 255 and self.counts.min() >= 0
        self._oracle = {}

    @property
    def n_tiles(self):
        return (self.B + TILE - 1) // TILE

    def upload(self, ctx):
        self.m.upload(ctx)
        ctx.upload_counts(self.counts)

    def oracle(self, z, r, ds=0):
        """-> (ll, ll_cond) of the exact oracle at one point (cached)."""
        key = (tuple(np.atleast_1d(z).tolist()), tuple(np.asarray(r).tolist()), int(ds))
        if key not in self._oracle:
            if self.m.bb_source >= 0:
                o = do.bb_gradient(self.model, z, r, self.counts[ds], self.m.bb_source)
            else:
                o = do.derivatives(self.model, z, r, counts=self.counts[ds], hessian=False)
            self._oracle[key] = (o['ll'], o['ll_cond'])
        return self._oracle[key]

    def oracle_many(self, zs, rs, ds=None):
        out = [self.oracle(zs[p] if self.m.d else np.zeros(0), rs[p], 0 if ds is None else ds[p]) for p in range(len(rs))]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def edited_counts(n, t=0):
    """A few empty bins, one run of empty bins and one bin with n = 1, wherever the row is long enough for them."""
    n = np.minimum(n, 255.0)
    B = len(n)
    if B > N_ONE_BIN:
        n[N_ONE_BIN] = 1.0
    for b in (0, 7 + t, 64, 255, 511, 512, B - 1, B - 2):
        if 0 <= b < B and b != N_ONE_BIN and B > 1:
            n[b] = 0.0
    if B > 400:
        n[300:390] = 0.0                                   # the run: more than a wave's 128 bins would see at once in two columns
    return n


_CASES = {}


def case(B, **kw):
    key = (B,) + tuple(sorted(kw.items()))
    if key not in _CASES:
        _CASES[key] = Case(B, **kw)
    return _CASES[key]


def tile_case(n_tiles, fill):
    return case(bins_of(n_tiles, fill))


def standard_points(c, seed=5):
    """Two random interior points of the lower cell and one of the upper, one on the middle anchor, the top corner -> (z [5, d],
    r [5, S]); without a shape axis five sets of rates."""
    m = c.m
    rng = np.random.default_rng([seed, c.B])
    r = rng.uniform(0.6, 1.4, (5, m.S))
    if not m.d:
        return np.zeros((5, 0)), r
    g = m.anchor_z[0]
    z = np.array([rng.uniform(g[0] + 0.05, g[1] - 0.05), rng.uniform(g[0] + 0.05, g[1] - 0.05), rng.uniform(g[1] + 0.05, g[2] - 0.05),
                  g[1], g[-1]])
    return z[:, None], r


# ---- the plain float64 evaluation and its mutants (CPU test) ----------------------------------------------------------------

def per_bin(c, z, r, ds=0):
    """-> (mu [B], n [B]) in plain float64 numpy: mu_b = sum over corners and sources of w_c u_s(z) rs_s P_cs(b)."""
    model = c.model
    S = c.m.S
    ps = np.asarray(model['ps'], dtype=float)
    mus = np.asarray(model['mus'], dtype=float)
    if c.m.d:
        k, t = orc.find_cell(model['anchor_z'][0], float(np.atleast_1d(z)[0]))
        corners = [(1.0 - t, ps[k], mus[k]), (t, ps[k + 1], mus[k + 1])]
    else:
        corners = [(1.0, ps, mus)]
    u = sum(w * mu_c for w, _, mu_c in corners) * np.asarray(r, dtype=float)
    mu = np.zeros(c.B)
    for w, p, _ in corners:
        for s in range(S):
            mu = mu + (w * u[s]) * p[s].reshape(-1)
    return mu, c.counts[ds]


def terms_of(mu, n):
    with np.errstate(all='ignore'):
        return np.where(n > 0, n * np.log(mu), 0.0) - mu - gammaln(n + 1.0)


def numpy_value(c, z, r, ds=0):
    mu, n = per_bin(c, z, r, ds)
    return float(np.sum(terms_of(mu, n)))


MUTANTS = ('bin dropped', 'bin twice', 'tile dropped', 'padding lanes', 'tiles swapped', 'empty branch at n = 1')


def mutant_values(c, z0, r0, z1, r1, ds=0):
    """-> {mutant: [(point index, value), ...]}: the values a kernel with that fault would return for points 0 and / or 1."""
    mu0, n = per_bin(c, z0, r0, ds)
    mu1, _ = per_bin(c, z1, r1, ds)
    t0, t1 = terms_of(mu0, n), terms_of(mu1, n)
    B = c.B
    live = np.flatnonzero(n > 1)                           # a bin with counts (not one of the emptied ones, not the n = 1 bin)
    j = int(live[len(live) // 2]) if len(live) else 0
    out = {}
    out['bin dropped'] = [(0, float(np.sum(np.delete(t0, j))))]
    out['bin twice'] = [(0, float(np.sum(np.append(t0, t0[j]))))]
    # the last whole tile (the only one, whole or not, where the model has a single tile)
    lo = (B // TILE - 1) * TILE if B >= TILE else 0
    out['tile dropped'] = [(0, float(np.sum(np.delete(t0, np.s_[lo:min(B, lo + TILE)]))))]
    # the lanes past the last bin (n = 0 there) evaluated with the last bin's mu; a full last tile: one lane past its end
    n_pad = (-B) % TILE or 1
    out['padding lanes'] = [(0, float(np.sum(np.append(t0, np.full(n_pad, -mu0[B - 1])))))]
    # tile 0 of the two points exchanged between their sums
    a, b = t0.copy(), t1.copy()
    a[:TILE], b[:TILE] = t1[:TILE], t0[:TILE]
    out['tiles swapped'] = [(0, float(np.sum(a))), (1, float(np.sum(b)))]
    # the bin with n = 1 (bin 0 of a one-bin model, whatever its count) takes the n = 0 branch: its n log mu is lost
    k = N_ONE_BIN if B > N_ONE_BIN else 0
    e = t0.copy()
    e[k] = -mu0[k] - gammaln(n[k] + 1.0)
    out['empty branch at n = 1'] = [(0, float(np.sum(e)))]
    return out


# ---- further shapes of the table ---------------------------------------------------------------------------------------------

SEAM_POINTS = 65537              # launches of 65 535 work items: the second launch holds two
SEAM_PROTOTYPES = 64
SINGLE_BIG_BINS = 1024 * TILE + 509          # 1025 tiles: one more block than the collector's first trip takes
BB_TILES = (1, 9, 129)
BB_SCAN_ITEMS = 4 * 65535 + 1    # 16-point items of one group: one more than k_scan_bb's gridDim.z covers


def seam_case():
    return case(TILE, n_anchor=())


def single_big_case():
    return case(SINGLE_BIG_BINS, n_anchor=(), S=1)


def bb_case(n_tiles):
    return case(bins_of(n_tiles, TILE - 1 if n_tiles > 1 else 300), bb_source=0)


def bb_scan_case():
    return case(16, n_anchor=(), bb_source=0)


def group_case():
    return case(2 * TILE + 1, T=2)


def every_case():
    """(name, maker) of every model of the table; maker() builds it (the Beeston-Barlow ones are held to do.bb_gradient)."""
    out = [('tiles %d fill %d' % tf, lambda tf=tf: tile_case(*tf)) for tf in TILE_SHAPES]
    out += [('seam', seam_case), ('groups', group_case), ('single big', single_big_case)]
    out += [('bb tiles %d' % t, lambda t=t: bb_case(t)) for t in BB_TILES] + [('bb scan', bb_scan_case)]
    return out


def prototypes(c, n, seed=9):
    """n points for batches of repeated points: random interior ones (both cells), so that n oracle evaluations cover a batch."""
    rng = np.random.default_rng([seed, c.B, n])
    r = rng.uniform(0.6, 1.4, (n, c.m.S))
    if not c.m.d:
        return np.zeros((n, 0)), r
    g = c.m.anchor_z[0]
    return rng.uniform(g[0], g[-1], (n, 1)), r
