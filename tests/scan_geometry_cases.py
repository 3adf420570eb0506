"""The models, data, prototype points and batches of the scan-geometry tests: shared by tests/test_scan_geometry_gpu.py (which
runs them through the matrix-core scan routes at every launch geometry) and tests/test_scan_geometry_cases.py (which shows on the
CPU that float64 emulations of the kernels' reassociations stay inside the oracle's bound at every case, and that the bound
rejects every mutant).

Models are SyntheticModel's templates as explicit arrays (so that single entries can be edited): S sources on one shape axis of
3 anchors (two cells), no axis (one cell) or a 3 x 3 grid (four cells); NS = 2^d S streams.  Every batch draws its points from
a small pool of PROTOTYPE points per cell whose oracle value is computed once (`ScanCase.oracle`); the pools' sizes are odd, so
neighbouring 16-point items and the four items of a quad never hold the same values."""
import numpy as np
from scipy.special import gammaln

import derivative_oracle as do
from oracle import blueice_oracle as orc

TILE = 512
STRIP = 64                       # bins per strip of k_scan_sorted and k_scan_valid (k_scan_mfma<2>: 32)
POOL = {1: 37, 2: 19, 4: 9}      # prototypes per cell, by the number of cells: odd (coprime to 16 and to 4), <= 38 per case

# ---- the table's axes --------------------------------------------------------------------------------------------------------
FALLBACK_BINS = (1, 63)          # B < 64: the count-sorted copy is refused
BINS = (64, 65, 511, 512, 513, 1023, 1024, 2049, 2559, 2560)      # 1, 2 and 5 tiles: last tile full, one bin, 511 bins
# NS -> (n_anchor, S): every KG = 1 .. 8 with and without padding streams
STREAMS = {1: ((), 1), 3: ((), 3), 4: ((3,), 2), 5: ((), 5), 8: ((3,), 4), 9: ((), 9), 12: ((3,), 6), 13: ((), 13), 16: ((3, 3), 4),
           17: ((), 17), 20: ((3,), 10), 22: ((3,), 11), 24: ((3, 3), 6), 25: ((), 25), 28: ((3,), 14), 29: ((), 29), 32: ((3,), 16)}
_SHAPES = dict(STREAMS)
_SHAPES[2] = ((), 2)           # (the exact-zero model: two sources, no axis)
_SHAPES[33] = ((), 33)         # (one stream more than the scan kernels take: fallback)
DENSE_DATA = ('poisson', 'runs', 'all_mixed', 'one_count')
SPARSE_DATA = ('ones_twos', 'upto12')
SPARSE_NNZ = (1, 63, 64, 65, 512, 513)
# points per cell: every quad remainder of the item count, a last item with one live slot (16 k + 1 with k % 4 = 2: k = 6)
CELL_POINTS = (1, 15, 16, 17, 48, 63, 64, 65, 97)


def make_counts(kind, B, rng, nnz=None):
    if kind == 'poisson':                                  # several events per bin, none empty: count-order strips are uniform
        return np.maximum(rng.poisson(4.0, B), 1).astype(float)
    if kind == 'runs':                                     # runs of empty bins (> 64 and < 64), single bins of n = 1 and a large n
        n = np.maximum(rng.poisson(4.0, B), 2).astype(float)
        n[B // 5:B // 5 + 90] = 0.0
        n[B // 2:B // 2 + 40] = 0.0
        n[3 % B] = 1.0
        n[(B // 3) % B] = 1e6
        return n
    if kind == 'all_mixed':                                # 32 bins per count: every 64-bin strip in count order holds two counts
        return 1.0 + (rng.permutation(B) // 32).astype(float)
    if kind == 'one_count':                                # one count throughout: the only mixed strip is the one next to the padding
        return np.full(B, 3.0)
    n = np.zeros(B)
    hot = rng.choice(B, nnz, replace=False)
    n[hot] = rng.integers(1, 3 if kind == 'ones_twos' else 13, nnz)
    return n


class ScanCase:
    """One model with its data: .model (dense dict for the oracle and the upload), .counts [T, B], the prototype pools
    .pool[cell] (indices into .pz / .pr) and .neg_rate (prototypes whose allowed-negative source has a rate below zero)."""

    def __init__(self, name, B, NS=4, data='poisson', nnz=None, T=1, negative=False, rate_scale=1.0, edit=None, seed=91,
                 n_proto=None):
        from blueice_amd.synthetic import SyntheticModel
        n_anchor, S = _SHAPES[NS]
        self.name, self.B, self.NS, self.S, self.T, self.data, self.nnz = name, B, NS, S, T, data, nnz
        m = SyntheticModel(S, n_anchor, (B,), seed=seed)
        self.d = m.d
        self.model = m.dense_model()
        self.model['anchor_z'] = [np.asarray(g, dtype=float) for g in m.anchor_z]
        rng = np.random.default_rng([seed, B, NS, T])
        self.counts = np.stack([make_counts(data, B, rng, nnz) for _ in range(T)])
        self.allow_negative = np.zeros(S, dtype=np.int32)
        self.n_cells = 2 ** self.d
        per_cell = n_proto or POOL[self.n_cells]
        zs, self.pool = [], []
        for c in range(self.n_cells):
            lo = [(-1.0, 0.0)[(c >> i) & 1] for i in range(self.d)]
            zs.append(np.array(lo)[None, :] + rng.uniform(0.03, 0.97, (per_cell, self.d)))
            self.pool.append(np.arange(c * per_cell, (c + 1) * per_cell))
        self.pz = np.concatenate(zs)
        self.pr = rng.uniform(0.6, 1.4, (len(self.pz), S)) * rate_scale
        self.neg_rate = np.zeros(len(self.pz), bool)
        if negative:                                       # the last source may go negative: every third prototype far below zero
            assert S >= 2
            self.allow_negative[S - 1] = 1                 # (expectations certainly negative), another third just below (all
            k = np.arange(len(self.pz)) % 3                # expectations certainly positive)
            # (the total rate stays above zero: a batch point whose summed rates are negative is rejected as unphysical before any
            #  kernel sees it; 1300 p_0 - 800 p_1 is negative wherever p_1 > 1.625 p_0)
            self.pr[k == 0, S - 1] = -0.4 * rate_scale
            self.pr[k == 0, 0] = 1.3 * rate_scale
            self.pr[k == 1, S - 1] = -0.002 * rate_scale
            self.neg_rate = k == 0
        if edit:
            edit(self)
        self._oracle, self._mu = {}, {}

    def upload(self, ctx):
        ctx.upload_model(self.model['anchor_z'], self.model['ps'], self.model['mus'])
        if self.allow_negative.any():
            ctx.set_allow_negative(self.allow_negative)
        ctx.upload_counts(self.counts)

    def oracle(self, i, ds=0):
        """-> (ll, ll_cond) of the exact oracle at prototype i (cached)."""
        if (i, ds) not in self._oracle:
            with np.errstate(all='ignore'):
                o = do.derivatives(self.model, self.pz[i], self.pr[i], counts=self.counts[ds], hessian=False)
            self._oracle[(i, ds)] = (o['ll'], o['ll_cond'])
        return self._oracle[(i, ds)]

    def mu_pairs(self, i):
        """-> (mu [B], weight [B]) of the oracle's running-error arithmetic at prototype i."""
        if i not in self._mu:
            cell = do.Cell(self.model['anchor_z'], self.pz[i])
            coef, _, _, _ = do.coefficient_columns(cell, self.model['mus'], self.pr[i], second=False)
            with np.errstate(all='ignore'):
                mu = do.tmatmul(coef, do.T(do._rows(self.model, cell, 0, self.B, self.S)))[0]
            self._mu[i] = (mu.v, mu.a)
        return self._mu[i]

    def sign_class(self, i):
        """'negative' (some mu_b certainly below zero), 'positive' (all certainly >= 0; an exact 0 counts) or 'undecided'."""
        v, a = self.mu_pairs(i)
        certain = np.abs(v) > do.C_POISSON * do.EPS * a
        if (certain & (v < 0)).any():
            return 'negative'
        return 'positive' if (certain | (v == 0)).all() else 'undecided'

    def expected(self, protos, ds=None):
        """-> (want, cond, kind) per point: kind 'bound' (held to the oracle's bound), 'nan' or '-inf' (asserted exactly)."""
        ds = np.zeros(len(protos), int) if ds is None else ds
        want, cond, kind = np.empty(len(protos)), np.empty(len(protos)), []
        memo = {}
        # scipy's poisson.logpmf: a nan count gives nan, a negative or non-integer one -inf, whatever the expectation
        n = self.counts
        bad = np.where(np.isnan(n).any(axis=1), 'nan', np.where(((n < 0) | (n != np.floor(n))).any(axis=1), '-inf', ''))
        for j, (i, t) in enumerate(zip(protos, ds)):
            if (i, t) not in memo and bad[t]:
                memo[(i, t)] = (np.nan, np.nan, str(bad[t]))
            if (i, t) not in memo:
                ll, c = self.oracle(int(i), int(t))
                if self.sign_class(int(i)) == 'negative' or np.isnan(ll):
                    k = 'nan'
                elif ll == -np.inf:
                    k = '-inf'
                else:
                    k = 'bound'
                memo[(i, t)] = (ll, c, k)
            want[j], cond[j], k = memo[(i, t)]
            kind.append(k)
        return want, cond, np.array(kind)


_CASES = {}


def case(name, B, **kw):
    key = (name, B) + tuple(sorted((k, v) for k, v in kw.items() if k != 'edit'))
    if key not in _CASES:
        _CASES[key] = ScanCase(name, B, **kw)
    return _CASES[key]


def bins_case(B, data='poisson'):
    """Dense data, or -- for the split scan -- mostly empty data (at most an eighth of the bins hold events)."""
    if data == 'poisson':
        return case('bins %d' % B, B)
    return case('bins %d sparse' % B, B, data='upto12', nnz=max(1, B // 9))


def stream_case(NS, data='poisson'):
    if data == 'poisson':
        return case('NS %d' % NS, 577, NS=NS, n_proto=5 if NS > 8 else None)
    return case('NS %d sparse' % NS, 1100, NS=NS, data='upto12', nnz=130, n_proto=5 if NS > 8 else None)


def dense_case(kind, B=2559):
    return case('dense %s' % kind, B, data=kind)


def sparse_case(kind, nnz):
    return case('sparse %s nnz %d' % (kind, nnz), max(600, 8 * nnz + 40), data=kind, nnz=nnz)


def two_dataset_case():
    return case('two datasets', 1100, data='upto12', nnz=130, T=2)


def negative_case(data='poisson'):
    if data == 'poisson':
        return case('negative dense', 1023, negative=True)
    return case('negative sparse', 2600, data='upto12', nnz=300, negative=True)


def five_tile_case(data):
    """5 tiles of bins: dense data (the count-sorted copy, the bin-order rows, or with sparse = 2 their compacted copy: 40 strips of
    64 bins), or mostly empty data for the split scan, whose validity pass walks all 5 tiles."""
    if data == 'poisson':
        return case('five tiles', 2559)
    return case('five tiles sparse', 2560, data='upto12', nnz=300)


def scaled_case(factor):
    return case('rates x %g' % factor, 1023, rate_scale=factor)


def _subnormal_row(c):
    # one entry of one template row so small that the learnt scale 2^-s (s ~ 150 for rates x 1e45) would make it subnormal
    c.model['ps'][(0,) * c.d + (0, 700)] = 1e-300


def subnormal_row_case():
    return case('rates x 1e45, one entry 1e-300', 1023, rate_scale=1e45, edit=_subnormal_row, seed=92)


def _zero_expectation(c):
    # no shape axis, two sources: source 0 has an exact zero in bin 5 (which holds data) and every third prototype gives source 1
    # the rate 0, so that mu_5 is exactly 0 there
    c.model['ps'][0, 5] = 0.0
    c.counts[0, 5] = 4.0
    c.pr[::3, 1] = 0.0


def zero_expectation_case():
    return case('exact zero expectation', 1023, NS=2, edit=_zero_expectation, seed=93)


def _nan_entry(c):
    c.model['ps'][0, 1, 100] = np.nan                      # anchor 0 (the lower cell's rows only), source 1, bin 100


INVALID_COUNTS = {'non-integer count': 2.5, 'negative count': -1.0, 'nan count': np.nan}


def invalid_counts_case(kind, data='poisson'):
    """The model, data and prototypes of bins_case(1023) (dense) or the mostly empty data of the NS 4 stream case, with ONE bin that
    holds data given a count scipy's poisson.logpmf answers with -inf (negative, non-integer) or nan (nan) at every point (not
    part of every_case: no point has a finite value to emulate)."""
    def edit(c):
        c.counts[0, np.flatnonzero(c.counts[0] > 0)[7]] = INVALID_COUNTS[kind]
    if data == 'poisson':
        return case(kind, 1023, edit=edit)
    return case(kind + ', sparse', 1100, data='upto12', nnz=130, edit=edit)


def fallback_cases():
    """Models no scan route takes (not part of every_case: the CPU emulations are of the scan kernels): B = 63, 33 streams, and a nan
    template entry (the lower cell's prototypes then give nan, the upper cell's are held to the bound)."""
    return [bins_case(63), case('NS 33', 577, NS=33, n_proto=5), case('nan template entry', 577, edit=_nan_entry, seed=94)]


def every_case():
    """(name, maker) of every model of the table."""
    out = [('bins %d' % B, lambda B=B: bins_case(B)) for B in FALLBACK_BINS + BINS]
    out += [('bins %d sparse' % B, lambda B=B: bins_case(B, 'upto12')) for B in BINS]
    out += [('NS %d' % NS, lambda NS=NS: stream_case(NS)) for NS in STREAMS]
    out += [('NS %d sparse' % NS, lambda NS=NS: stream_case(NS, 'upto12')) for NS in STREAMS]
    out += [('dense %s' % k, lambda k=k: dense_case(k)) for k in DENSE_DATA]
    out += [('dense one_count 2560', lambda: dense_case('one_count', 2560))]
    out += [('sparse %s nnz %d' % (k, z), lambda k=k, z=z: sparse_case(k, z)) for k in SPARSE_DATA for z in SPARSE_NNZ]
    out += [('two datasets', two_dataset_case), ('negative dense', negative_case), ('negative sparse', lambda: negative_case('upto12')),
            ('five tiles sparse', lambda: five_tile_case('upto12')), ('rates x 1e45', lambda: scaled_case(1e45)),
            ('rates x 1e-135', lambda: scaled_case(1e-135)), ('subnormal row entry', subnormal_row_case),
            ('exact zero expectation', zero_expectation_case)]
    return out


# ---- batches -----------------------------------------------------------------------------------------------------------------

def batch(c, cell_points, ds_of_cell=None, seed=3, shuffle=True):
    """cell_points[k] points in cell k (cells of a second dataset: further entries with ds_of_cell), point j of an entry taking
    prototype pool[j % len(pool)] -> (z, r, ds, proto) in shuffled batch order."""
    protos, ds = [], []
    for k, n in enumerate(cell_points):
        cell = k % c.n_cells
        pool = c.pool[cell]
        protos.append(pool[(np.arange(n) + 5 * k) % len(pool)])
        ds.append(np.full(n, 0 if ds_of_cell is None else ds_of_cell[k]))
    protos, ds = np.concatenate(protos), np.concatenate(ds)
    if shuffle:
        order = np.random.default_rng([seed, len(protos)]).permutation(len(protos))
        protos, ds = protos[order], ds[order]
    return (c.pz[protos] if c.d else None), c.pr[protos], ds, protos


# ---- float64 emulations of the kernels' evaluation orders (CPU test) --------------------------------------------------------------

def streams(c, i):
    """-> (coef [NS], rows [NS, B]) of prototype i in plain float64: stream = corner x source, mu = coef @ rows."""
    model, S = c.model, c.S
    corners = [((), 1.0)]
    for ax, g in enumerate(model['anchor_z']):
        k, t = orc.find_cell(g, float(c.pz[i][ax]))
        corners = [(idx + (k + up,), w * (t if up else 1.0 - t)) for idx, w in corners for up in (0, 1)]
    u = sum(w * np.asarray(model['mus'][idx], dtype=float) for idx, w in corners) * c.pr[i]
    coef = np.concatenate([w * u for _, w in corners])
    rows = np.concatenate([np.asarray(model['ps'][idx], dtype=float).reshape(S, -1) for idx, _ in corners])
    return coef, rows


def plain_value(c, i, ds=0):
    coef, rows = streams(c, i)
    mu, n = coef @ rows, c.counts[ds]
    with np.errstate(all='ignore'):
        return float(np.sum(np.where(n > 0, n * np.log(mu), 0.0) - mu - gammaln(n + 1.0)))


def _padded(x, fill=0.0):
    out = np.full(max(TILE, -(-len(x) // TILE) * TILE), fill)
    out[:len(x)] = x
    return out


def _log_of_product(mu):
    """log of the product along the last axis, multiplied pairwise in a tree; the exponents are taken out first and added back
    inside the logarithm (what the kernel's power-of-two scale does), so that no partial product leaves the double range."""
    m, e = np.frexp(mu)
    while m.shape[-1] > 1:
        m = m[..., 0::2] * m[..., 1::2]
    return np.log(m[..., 0]) + e.sum(axis=-1) * np.log(2.0)


class Strips:
    """The terms sum n log mu of one prototype, strip by strip, as k_scan_sorted forms them: rows in count order (ties by bin;
    `compacted`: the non-empty bins only), padded with empty bins to whole tiles; a strip of one positive count n gives n log of
    the product of its 64 expectations ('U'), a strip of empty bins nothing ('Z'), any other its bins one by one ('M').
    value = const + sum(terms): const holds -sum_b mu_b as sum_k coef_k rowsum_k and -sum lgamma(n + 1) (linear_outside)."""

    def __init__(self, c, i, ds=0, compacted=False, extra_mu=None):
        coef, rows = streams(c, i)
        n = c.counts[ds]
        mu = coef @ rows
        if extra_mu is not None:
            mu = mu + extra_mu(coef, rows)
        self.const = -float(coef @ rows.sum(axis=1)) - float(np.sum(gammaln(n + 1.0)))
        keep = np.flatnonzero(n > 0) if compacted else np.arange(len(n))
        order = keep[np.argsort(n[keep], kind='stable')]
        self.n = _padded(n[order]).reshape(-1, STRIP)
        self.mu = _padded(mu[order], 1.0).reshape(-1, STRIP)
        first = self.n[:, :1]
        one = (self.n == first).all(axis=1)
        self.cls = np.where(one & (first[:, 0] > 0), 'U', np.where(one, 'Z', 'M'))
        self.count = first[:, 0]
        with np.errstate(all='ignore'):
            self.logprod = _log_of_product(self.mu)
            per_bin = np.where(self.n > 0, self.n * np.log(self.mu), 0.0).sum(axis=1)
        self.terms = np.where(self.cls == 'U', self.count * self.logprod, np.where(self.cls == 'Z', 0.0, per_bin))

    def value(self, terms=None):
        return self.const + float(np.sum(self.terms if terms is None else terms))


def sorted_value(c, i, ds=0, compacted=False):
    return Strips(c, i, ds, compacted).value()


def prod_value(c, i, ds=0):
    """k_scan_mfma<2, KG, MASK, 1> on the compacted rows in bin order: a 16-bin block whose counts are all 1 or 2 gives, per lane
    (bins kq, 4 + kq, 8 + kq, 12 + kq), one logarithm of the product of mu^n; other blocks their bins one by one."""
    coef, rows = streams(c, i)
    n_all = c.counts[ds]
    mu_all = coef @ rows
    keep = np.flatnonzero(n_all > 0)
    n = _padded(n_all[keep]).reshape(-1, 4, 4)             # [block, r, kq]
    mu = _padded(mu_all[keep], 1.0).reshape(-1, 4, 4)
    small = ((n == 1) | (n == 2)).all(axis=(1, 2))
    with np.errstate(all='ignore'):
        f = np.where(n == 2, mu * mu, mu)
        lane = np.log((f[:, 0] * f[:, 1]) * (f[:, 2] * f[:, 3])).sum(axis=1)
        per_bin = np.where(n > 0, n * np.log(mu), 0.0).sum(axis=(1, 2))
    total = float(np.sum(np.where(small, lane, per_bin)))
    return total - float(coef @ rows.sum(axis=1)) - float(np.sum(gammaln(n_all + 1.0)))


EMULATIONS = ('plain', 'count-order strips', 'compacted count-order strips', 'product form of four bins')


def emulate(c, which, i, ds=0):
    if which == 'plain':
        return plain_value(c, i, ds)
    if which == 'count-order strips':
        return sorted_value(c, i, ds)
    if which == 'compacted count-order strips':
        return sorted_value(c, i, ds, compacted=True)
    return prod_value(c, i, ds)


# ---- mutants of the count-order emulation ------------------------------------------------------------------------------------

MUTANTS = ('strip dropped', 'strip twice', "one wave's share of a mixed strip dropped", 'last item of a ragged quad dropped',
           'padding slot of the last item counted', 'first item of a chunk twice', "uniform strip with its neighbour's count",
           'two results of a quad swapped', 'padding stream read as live')
MUTANT_LAYOUT = (16 * 18 + 1, 33)     # points in cells 0 and 1 (the CPU test's batch): 19 items (a ragged quad, a last item with one
CHUNK = 16                            # live slot, more than one chunk of 16 items) and 3 items


def mutant_values(c, n0=MUTANT_LAYOUT[0], nslots=4):
    """-> {mutant: [(prototype, value), ...] or None where this case cannot express it}: the values a k_scan_sorted with that
    fault would return for points of cell 0, which holds n0 points (point j = prototype pool[j % len(pool)])."""
    pool = c.pool[0]
    proto = lambda j: int(pool[j % len(pool)])
    n_items = -(-n0 // 16)
    st = {}

    def strips(j):
        if proto(j) not in st:
            st[proto(j)] = Strips(c, proto(j))
        return st[proto(j)]

    s0 = strips(0)
    uni, mixed = np.flatnonzero(s0.cls == 'U'), np.flatnonzero((s0.cls == 'M') & (s0.terms != 0))
    data = np.concatenate([uni, mixed])
    out = dict.fromkeys(MUTANTS)
    if len(data):
        k = data[len(data) // 2]
        out['strip dropped'] = [(proto(0), s0.value() - s0.terms[k])]
        out['strip twice'] = [(proto(0), s0.value() + s0.terms[k])]
    if len(mixed) and n_items > 1 % nslots:                  # wave 1 of nslots: items 1, 1 + nslots, ... of every mixed strip
        s = strips(16)
        out["one wave's share of a mixed strip dropped"] = [(proto(16), s.value() - s.terms[mixed].sum())]
    if len(uni) and n_items % 4:                             # the last live item of the last quad: its product-form terms are lost
        j = 16 * (n_items - 1)
        s = strips(j)
        out['last item of a ragged quad dropped'] = [(proto(j), s.value() - s.terms[uni].sum())]
    if len(data) and n0 % 16:                                # a padding slot (a copy of the last live point) added to that point
        s = strips(n0 - 1)
        out['padding slot of the last item counted'] = [(proto(n0 - 1), s.value() + s.terms.sum())]
    if len(data) and n_items > CHUNK:
        s = strips(16 * CHUNK)
        out['first item of a chunk twice'] = [(proto(16 * CHUNK), s.value() + s.terms.sum())]
    # (two uniform strips of different counts are never adjacent unless a run ends on a strip's edge: the neighbour is the next
    #  uniform strip with another count, the mixed strip between them apart -- a count kept from the strip worked before)
    pairs = [(k, m) for k, m in zip(uni[:-1], uni[1:]) if s0.count[k] != s0.count[m]]
    if pairs:
        k, m = pairs[len(pairs) // 2]
        t = s0.terms.copy()
        t[k] = s0.count[m] * s0.logprod[k]
        out["uniform strip with its neighbour's count"] = [(proto(0), s0.value(t))]
    if len(data) and n_items > 1 and proto(0) != proto(16):
        out['two results of a quad swapped'] = [(proto(0), strips(16).value()), (proto(16), s0.value())]
    if c.NS % 4:                                             # the padding streams of the last 4-stream group: the row and coefficient
        pad = 4 - c.NS % 4                                   # the kernel steers their reads to (stream NS - 1), not zeroed
        out['padding stream read as live'] = [(proto(0), Strips(c, proto(0), extra_mu=lambda coef, rows: pad * coef[-1] * rows[-1]).value())]
    # a fault whose every result is, bit for bit, the unmutated emulation's cannot be expressed in float64 at this case (rates x 1e45:
    # every n log mu term lies below the last bit of -sum mu ~ 1e48)
    for name, results in out.items():
        if results is not None and name != 'two results of a quad swapped' and all(v == st[i].value() for i, v in results if i in st):
            out[name] = None
    return out
