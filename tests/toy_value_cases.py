"""The table, the batch oracle and the mutants of the toy-MC evaluation tests: shared by tests/test_toy_value_gpu.py (which holds
every route of bi_eval_datasets and bi_eval_datasets_points to the exact oracle, every dataset of every call) and
tests/test_toy_value_cases.py (which shows on the CPU that the table holds the edges it promises, that `values` is the oracle of
tests/derivative_oracle.py, and that the bound rejects every mutant).

`values(model, z, rs, counts [T, B]) -> (ll [T], cond [T])`: mu_b and log mu_b once per point as running-error pairs
(derivative_oracle's Cell, coefficient_columns, tmatmul and T.log over blocks of BLOCK bins), then per dataset

    ll_t = sum_{b: n_tb > 0} n_tb log mu_b - sum_b mu_b - sum_b lgamma(n_tb + 1)

with math.fsum, and cond_t by the running-error rule `derivative_oracle.derivatives` applies to the same expression (per bin
n log mu - mu - lgamma(n + 1), left to right).  A dataset with n > 0 where mu = 0 has ll = -inf (cond = inf: compared with ==,
not through the bound).

`edge_table(anchor_z, variant)`: one model (d = 1, S = 2, B = 4 * 8192 + 1 bins: 5 tiles of the single-point lists, the last one
bin wide, 9 tiles of 4096 of the multi-point lists) and T = 600 uploaded datasets in which every edge of the tile-major lists and
of the walk over them is placed on purpose (ROW NAMES below).  Every mu_b is 0 or at most 1 / 2, so that an entry dropped or
counted twice moves the value by at least log 2.

Imports only `oracle/`, `derivative_oracle`, numpy and scipy.special.  Test infrastructure only."""
import math

import numpy as np
from scipy.special import gammaln

import derivative_oracle as do
from oracle import blueice_oracle as orc

TILE1, TILE_MULTI = 8192, 4096           # bins per tile of the single-point and of the multi-point lists
B_EDGE = 4 * TILE1 + 1
T_EDGE = 600
ZERO_BINS = (0, TILE1 - 1, TILE1, 3 * TILE_MULTI, B_EDGE - 1 - TILE1)       # mu = 0 exactly: 0, 8191, 8192, 12288, 24576
RUN_LO, RUN_HI = 2 * TILE1, 2 * TILE1 + TILE_MULTI                          # crafted runs: one tile of either tiling
SLOTS = (48, 64, 96, 128)                # entry slots a run is given up front, by kernel variant
RUN_LENGTHS = tuple(sorted(set((1, 3, 4, 5, 7, 8, 9, 15, 16, 17) + tuple(s + k for s in SLOTS for k in (-1, 0, 1, 17))
                               + tuple(2 * s + 1 for s in SLOTS))))
ONE_ENTRY_BINS = (1, TILE1 - 2, TILE1 + 1, TILE_MULTI - 2, TILE_MULTI + 1, B_EDGE - 1)
VARIANT_COUNTS = {None: None, 'count8': 8.0, 'count32767': 32767.0, 'count32768': 32768.0}

# the two single-point test points (different halves of the cell [0, 1]; the second with a rate of exactly zero) and the points
# of the multi-point calls on the three-anchor model (both cells, the middle anchor, rates only)
POINTS_1 = ((0.3, (1.3, 0.8)), (0.8, (0.0, 1.1)))
ANCHORS_3 = (0.0, 1.0, 2.0)


def multi_points(P):
    """-> (z [P, 1], rs [P, 2]) on ANCHORS_3: both cells in turn, the middle anchor (point 3) and the top corner (point 6)."""
    z = np.array([0.3, 1.6, 0.8, 1.0, 1.25, 0.05, 2.0, 0.5, 1.9])[:P]
    rs = np.random.default_rng(P).uniform(0.6, 1.5, (P, 2))
    return z[:, None], rs


def rate_points(P, z=0.4):
    """-> P points that differ in their rates only (one cell: one work item of the log mu kernel), a rate of exactly 0 among them."""
    rs = np.column_stack([np.linspace(0.0, 1.5, P), np.linspace(1.4, 0.7, P)])
    return np.full((P, 1), z), rs


def build_model(anchor_z=(0.0, 1.0), B=B_EDGE, zero_bins=ZERO_BINS, lo=0.002, hi=0.012, seed=2024):
    """S = 2 sources on one shape axis (or none: anchor_z = ()); expected counts per (anchor, source, bin) uniform in
    [lo, hi), exactly 0 at `zero_bins` for every anchor and source.  The first anchors of a longer grid are those of a shorter."""
    rng = np.random.default_rng(seed)
    A = max(1, len(anchor_z))
    f = np.stack([rng.uniform(lo, hi, (2, B)) for _ in range(A)])
    f[:, :, list(zero_bins)] = 0.0
    mus = f.sum(axis=2)
    ps = f / mus[:, :, None]
    if len(anchor_z) == 0:
        return dict(anchor_z=[], ps=ps[0], mus=mus[0])
    return dict(anchor_z=[np.asarray(anchor_z, dtype=float)], ps=ps, mus=mus)


# ---- the batch oracle ---------------------------------------------------------------------------------------------------------

def log_mu(model, z, rs):
    """-> (mu, log mu) as running-error pairs (T of [B]), evaluated as `derivative_oracle.derivatives` evaluates them."""
    d = len(model['anchor_z'])
    rs = np.asarray(rs, dtype=float)
    S = len(rs)
    cell = do.Cell(model['anchor_z'], np.asarray(z, dtype=float).reshape(d))
    coef, _, _, _ = do.coefficient_columns(cell, model['mus'], rs, second=False)
    B = do.n_bins(model)
    mv, ma, lv, la = np.empty(B), np.empty(B), np.empty(B), np.empty(B)
    for b0 in range(0, B, do.BLOCK):
        b1 = min(B, b0 + do.BLOCK)
        mu = do.tmatmul(coef, do.T(do._rows(model, cell, b0, b1, S)))[0]
        lg = mu.log()
        mv[b0:b1], ma[b0:b1], lv[b0:b1], la[b0:b1] = mu.v, mu.a, lg.v, lg.a
    return do.T(mv, ma), do.T(lv, la)


def values(model, z, rs, counts):
    """-> (ll [T], cond [T]) of the binned Poisson likelihood of every dataset (counts [T, B]) at one point."""
    counts = np.asarray(counts)                                       # (any dtype: the tables keep theirs as uint16)
    counts = counts.reshape(-1, counts.shape[-1])
    n_sets, B = counts.shape
    assert B == do.n_bins(model)
    mu, lg = log_mu(model, z, rs)
    # every bin's -mu, and the weight an EMPTY bin adds (a_mu + |-mu| + |-mu - 0|), per block of bins
    base_parts, base_cond = [], 0.0
    for b0 in range(0, B, do.BLOCK):
        b1 = min(B, b0 + do.BLOCK)
        base_parts.append(-math.fsum(mu.v[b0:b1].tolist()))
        base_cond += float((mu.a[b0:b1] + 2.0 * np.abs(mu.v[b0:b1])).sum())
    tt, bb = np.nonzero(counts > 0)
    n = counts[tt, bb].astype(float)
    with np.errstate(all='ignore'):
        nlog = n * lg.v[bb]
        a_nlog = n * lg.a[bb] + np.abs(nlog)
        lgam = gammaln(n + 1.0)
        v1 = nlog - mu.v[bb]
        v2 = v1 - lgam
        # (the bin's own weight in place of the empty bin's 2 mu; a_mu is in base_cond already)
        extra = a_nlog + np.abs(v1) + np.abs(v2) - 2.0 * np.abs(mu.v[bb])
    seg = np.searchsorted(tt, np.arange(n_sets + 1))
    nlog_l, lgam_l = nlog.tolist(), (-lgam).tolist()
    ll, cond = np.empty(n_sets), np.empty(n_sets)
    for t in range(n_sets):
        a, b = int(seg[t]), int(seg[t + 1])
        ll[t] = math.fsum(nlog_l[a:b] + lgam_l[a:b] + base_parts)
        cond[t] = base_cond + float(extra[a:b].sum())
    cond[~np.isfinite(ll) | ~np.isfinite(cond)] = np.inf
    return ll, cond


def check(got, want, cond, what=''):
    """The comparison of the GPU tests: rows the oracle gives as -inf with ==, every other row through the bound -> worst ratio."""
    got, want, cond = (np.asarray(x, dtype=float) for x in (got, want, cond))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), '%s: rows expected at -inf: got %r' % (what, got[~fin])
    return do.check_entries(got[fin], want[fin], cond[fin], do.C_POISSON, what)


# ---- the table ------------------------------------------------------------------------------------------------------------------

class Table:
    """.model (dense dict for the oracle), .counts [T, B], .rows {name: dataset}, .runs {dataset: run length}, .cell (dataset, bin)
    of the entry the count variants change, .fillers [datasets]"""

    def __init__(self, model, counts, rows, runs, cell, fillers):
        self.model, self.counts, self.rows, self.runs, self.cell, self.fillers = model, counts, rows, runs, cell, fillers
        self.T, self.B = counts.shape
        self._oracle = {}

    def oracle(self, z, rs):
        """values() of the whole table at one point, computed once."""
        key = (tuple(float(x) for x in np.asarray(z if z is not None else [], dtype=float).reshape(-1)), tuple(float(x) for x in rs))
        if key not in self._oracle:
            self._oracle[key] = values(self.model, key[0], key[1], self.counts)
        return self._oracle[key]

    def upload(self, ctx):
        m = self.model
        ctx.upload_model(m['anchor_z'], m['ps'], m['mus'])
        ctx.set_param('sparse', 1)
        ctx.upload_counts(self.counts)


def run_lengths(counts, tile):
    """-> [T, n_tiles]: the entries of every (dataset, tile) run of the tile-major lists."""
    B = counts.shape[1]
    return np.add.reduceat((counts > 0).astype(np.int64), np.arange(0, B, tile), axis=1)


ROW_NAMES = (('empty',) + tuple('one@%d' % b for b in ONE_ENTRY_BINS) + ('all7', 'minus_inf', 'tile_end_4096', 'tile_end_8192')
             + tuple('run%d' % k for k in RUN_LENGTHS))
_BASE = {}


def _base_counts():
    if 'counts' in _BASE:
        return _BASE['counts'], _BASE['rows'], _BASE['runs'], _BASE['fillers']
    rng = np.random.default_rng(600)
    T, B = T_EDGE, B_EDGE
    counts = np.zeros((T, B), dtype=np.uint16)                        # (39 MB a table instead of 157: they live as long as the session)
    live = np.setdiff1d(np.arange(B), ZERO_BINS)
    # the named rows evenly over the datasets: the first and the last dataset are named ones, every slice of 200 holds some
    where = np.round(np.arange(len(ROW_NAMES)) * (T - 1) / (len(ROW_NAMES) - 1)).astype(int)
    rows = {name: int(t) for name, t in zip(ROW_NAMES, where)}
    runs = {}

    def fill(t, k, lo=1, hi=8):
        hit = rng.choice(live, size=k, replace=False)
        counts[t, hit] = rng.integers(lo, hi, size=k)

    def run(t, k, must=()):
        pool = np.setdiff1d(np.arange(RUN_LO, RUN_HI), must)
        hit = np.concatenate([rng.choice(pool, size=k - len(must), replace=False), np.asarray(must, dtype=int)])
        counts[t, hit] = rng.integers(1, 8, size=k)

    for b in ONE_ENTRY_BINS:
        counts[rows['one@%d' % b], b] = rng.integers(1, 8)
    fill(rows['all7'], 250, 7, 8)
    fill(rows['minus_inf'], 250)
    counts[rows['minus_inf'], TILE1] = 1.0                            # n = 1 where mu = 0
    run(rows['tile_end_4096'], 5, must=(RUN_HI - 1,))                 # the run's last entry in the last bin of the 4096 tile
    run(rows['tile_end_8192'], 4)
    counts[rows['tile_end_8192'], 3 * TILE1 - 1] = 3.0                # ... and of the 8192 tile (bin 24575)
    for k in RUN_LENGTHS:
        run(rows['run%d' % k], k)
        runs[rows['run%d' % k]] = k
    named = set(rows.values())
    fillers = [t for t in range(T) if t not in named]
    for t in fillers:
        fill(t, int(rng.integers(100, 401)))
    counts.setflags(write=False)
    _BASE.update(counts=counts, rows=rows, runs=runs, fillers=fillers)
    return counts, rows, runs, fillers


def edge_table(anchor_z=(0.0, 1.0), variant=None):
    """The table (see the module docstring).  `variant`: None, or 'count8' / 'count32767' / 'count32768': one entry of one filler
    dataset holds that count (four-byte entries; their largest count; a count that fits neither width)."""
    key = (tuple(anchor_z), variant)
    if key not in _BASE:
        counts, rows, runs, fillers = _base_counts()
        t = fillers[len(fillers) // 2]
        cell = (t, int(np.flatnonzero(counts[t])[7]))
        if VARIANT_COUNTS[variant] is not None:
            if ('counts', variant) not in _BASE:                      # (one copy per variant, whatever the anchors)
                changed = counts.copy()
                changed[cell] = VARIANT_COUNTS[variant]
                changed.setflags(write=False)
                _BASE[('counts', variant)] = changed
            counts = _BASE[('counts', variant)]
        _BASE[key] = Table(build_model(anchor_z), counts, rows, runs, cell, fillers)
    return _BASE[key]


def seam_table(T=16390, B=600, seed=7):
    """d = 0, S = 2, B = 600 and T dense datasets (past the 16 384-dataset chunk of the dense row kernel, no multiple of its 8
    datasets per block): Poisson draws of about 60 events, the first dataset empty."""
    key = ('seam', T, B, seed)
    if key not in _BASE:
        model = build_model((), B=B, zero_bins=(5,), lo=0.02, hi=0.08, seed=seed)
        rng = np.random.default_rng(seed + 1)
        mu = (model['mus'][:, None] * model['ps']).sum(axis=0)
        counts = rng.poisson(mu, size=(T, B)).astype(np.uint16)
        counts[0] = 0
        counts[T - 1, 17] = 41                                    # (a count no list entry format limits here)
        counts.setflags(write=False)
        _BASE[key] = Table(model, counts, {'empty': 0}, {}, None, [])
    return _BASE[key]


# ---- the plain float64 evaluation and its mutants --------------------------------------------------------------------------------

def plain_log_mu(model, z, rs):
    """-> (mu [B], log mu [B]) in plain float64 numpy: mu_b = sum over corners and sources of w_c u_s(z) rs_s P_cs(b)."""
    ps = np.asarray(model['ps'], dtype=float)
    mus = np.asarray(model['mus'], dtype=float)
    if len(model['anchor_z']):
        k, t = orc.find_cell(model['anchor_z'][0], float(np.asarray(z).reshape(-1)[0]))
        corners = [(1.0 - t, ps[k], mus[k]), (t, ps[k + 1], mus[k + 1])]
    else:
        corners = [(1.0, ps, mus)]
    u = sum(w * mu_c for w, _, mu_c in corners) * np.asarray(rs, dtype=float)
    mu = np.zeros(ps.shape[-1])
    for w, p, _ in corners:
        for s in range(len(u)):
            mu = mu + (w * u[s]) * p[s]
    with np.errstate(all='ignore'):
        return mu, np.log(mu)


class Plain:
    """The pieces a kernel puts together: the entries (dataset, bin, count), log mu, sum mu, sum lgamma per dataset."""

    def __init__(self, model, z, rs, counts):
        self.T, self.B = counts.shape
        self.mu, self.lv = plain_log_mu(model, z, rs)
        self.summu = float(np.sum(self.mu))
        self.tt, self.bb = np.nonzero(counts > 0)
        self.n = counts[self.tt, self.bb].astype(float)
        self.seg = np.searchsorted(self.tt, np.arange(self.T + 1))
        self.lg = np.array([float(np.sum(gammaln(self.n[a:b] + 1.0))) for a, b in zip(self.seg[:-1], self.seg[1:])])

    def partials(self, tile=TILE1, n=None, lv=None, keep=None):
        """-> [T, n_tiles]: sum of n log mu per (dataset, tile) run (pairwise np.sum per run)."""
        n = self.n if n is None else n
        lv = self.lv if lv is None else lv
        with np.errstate(all='ignore'):
            term = n * lv[self.bb]
        n_tl = (self.B + tile - 1) // tile
        out = np.zeros((self.T, n_tl))
        key = self.tt * n_tl + self.bb // tile
        if keep is not None:
            term, key = term[keep], key[keep]
        cut = np.flatnonzero(np.diff(key)) + 1
        for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(key)]])):
            if b > a:
                out[key[a] // n_tl, key[a] % n_tl] = np.sum(term[a:b])
        return out

    def finish(self, part, summu=None, lg=None):
        return np.sum(part, axis=1) - (self.summu if summu is None else summu) - (self.lg if lg is None else lg)

    def value(self):
        return self.finish(self.partials())


def numpy_values(model, z, rs, counts):
    return Plain(model, z, rs, counts).value()


def _entry(p, t, which):
    """index into the entry arrays of entry `which` (negative: from the end) of dataset t"""
    a, b = int(p.seg[t]), int(p.seg[t + 1])
    return (b + which) if which < 0 else (a + which)


def _drop(tab, p, other):
    keep = np.ones(len(p.n), bool)
    keep[_entry(p, tab.cell[0], 3)] = False
    return p.finish(p.partials(keep=keep))


def _twice(tab, p, other):
    n = p.n.copy()
    n[_entry(p, tab.cell[0], 3)] *= 2.0
    return p.finish(p.partials(n=n))


def _count_and_7(tab, p, other):
    return p.finish(p.partials(n=np.where(p.n > 7, np.mod(p.n, 8.0), p.n)))


def _padding_counted(tab, p, other):
    # the padding entries of a run of 5 (three, of the eight of a 16-byte group) read as count 1 at bin 0 of the tile
    t = tab.rows['run5']
    part = p.partials()
    part[t, RUN_LO // TILE1] += 3.0 * p.lv[RUN_LO // TILE1 * TILE1]
    return p.finish(part)


def _tail_entry_dropped(tab, p, other):
    keep = np.ones(len(p.n), bool)
    keep[_entry(p, tab.rows['run%d' % (SLOTS[0] + 1)], -1)] = False
    return p.finish(p.partials(keep=keep))


def _tile_omitted(tab, p, other):
    part = p.partials()
    part[:, RUN_LO // TILE1] = 0.0
    return p.finish(part)


def _lgsum_of_neighbour(tab, p, other):
    return p.finish(p.partials(), lg=np.roll(p.lg, -1))


def _runs_exchanged(tab, p, other):
    part = p.partials()
    t = tab.rows['run17']
    part[[t, t + 1], RUN_LO // TILE1] = part[[t + 1, t], RUN_LO // TILE1]
    return p.finish(part)


def _summu_of_other_point(tab, p, other):
    return p.finish(p.partials(), summu=other.summu)


# name -> f(table, Plain at the point, Plain at another point) -> ll [T] as a kernel with that fault would return it.  Run them on
# the 'count8' variant of the table: it holds every edge of the base table and the count the `& 7` mutant needs.
MUTANTS = {
    'one entry dropped': _drop,
    'one entry counted twice': _twice,
    'count read through & 7': _count_and_7,
    'padding entry counted at bin 0 of its tile': _padding_counted,
    'last entry beyond the up-front slots dropped': _tail_entry_dropped,
    "one tile's partial omitted": _tile_omitted,
    'lgsum of the neighbouring dataset': _lgsum_of_neighbour,
    'runs of two neighbouring datasets exchanged': _runs_exchanged,
    'sum mu of another point': _summu_of_other_point,
}
