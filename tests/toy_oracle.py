"""An exact oracle of the three toy-generator streams, written from the text of include/blueice_hip.h (bi_generate_toys
streams A and B, bi_simulate_events) in NumPy -- nothing is imported from blueice_amd -- and the comparison functions that
replay a device result draw for draw.  Test infrastructure only.

Every comparison the device makes in rounded arithmetic carries a BAND; a draw with a comparison inside its band is
UNDECIDED: counted, never compared.  At most CAP of the draws of a case may be undecided.
  inversion (mu < 10)   the exact answer is the Poisson quantile, the smallest n with u <= CDF(n; mu), CDF in long double
                        (64-bit mantissa) with a compensated sum.  Band: |u - CDF step| < 2^-44 absolute -- the device loop
                        runs at most ~60 terms for mu < 10, each with at most 2n + 2 roundings (the exp included): <= ~2^-46
                        in all; the band is four times that.
  PTRS (mu >= 10)       replayed attempt by attempt.  Bands: the argument of floor within 2^-40 relative of an integer (the
                        multiply-adds may be fused), V against vr within 2^-44, the logarithmic test within
                        1e-10 max(1, |right side|) (device log and lgamma are not correctly rounded).  us >= 0.07, us < 0.013
                        and V > us compare values that are exact functions of the uniforms: no band.
  bisection             target = u M against the exact running sums: within 2^-42 M of a boundary (the device prefix sum
                        has a fixed tree order of a few hundred additions; 2^-42 is 2048 eps).
  positions             a device coordinate within 2 ulp of e_i + u (e_{i+1} - e_i) and inside [e_i, e_{i+1}]."""
import numpy as np
from scipy.special import gammaln

LD = np.longdouble
M32 = np.uint64(0xFFFFFFFF)
EV_TAG = 0x45564E54
SIM_TAG = 0x53494D45
SIM_COUNT_KEY = 0x9E3779B97F4A7C15
EVENT_COUNT_BIN = (1 << 40) + 7
SIM_MAX_RATE = 2.0 ** 30
CAP = 1e-5
BAND_CDF = 2.0 ** -44
BAND_FLOOR = 2.0 ** -40
BAND_VR = 2.0 ** -44
BAND_LOG = 1e-10
BAND_BISECT = 2.0 ** -42
_U64 = np.uint64


def _w(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox_v(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (broadcast against each other) -> (r0, r1, r2, r3)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(_w(c0), _w(c1), _w(c2), _w(c3), _w(k0), _w(k1))
    a0, a1 = _U64(0xD2511F53), _U64(0xCD9E8D57)
    s = _U64(32)
    for _ in range(10):
        a, b = a0 * c0, a1 * c2                                  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (b >> s) ^ c1 ^ k0, b & M32, (a >> s) ^ c3 ^ k1, a & M32
        k0, k1 = (k0 + _U64(0x9E3779B9)) & M32, (k1 + _U64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def u53(hi, lo):
    return ((hi >> _U64(5)).astype(np.float64) * 67108864.0 + (lo >> _U64(6)).astype(np.float64)) * 2.0 ** -53


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def _dataset_words(D, mutant=None):
    D = np.asarray(D, dtype=np.uint64)
    hi = (D >> _U64(32)) & _U64(0xFFFF)
    if mutant == 'trunc32':
        hi = hi * _U64(0)
    return D & M32, hi


# ---- the two samplers ---------------------------------------------------------------------------------------------------

def poisson_quantile(lam, u):
    """The exact draw of poisson_small: smallest n with u <= CDF(n; lam) -> (n float64, undecided bool)."""
    lam, u = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(u, dtype=np.float64))
    shape = lam.shape
    lam, u = lam.ravel().astype(LD), u.ravel().astype(LD)
    p = np.exp(-lam)
    F, c = p.copy(), np.zeros_like(p)
    prev = np.full_like(p, -1)
    n = np.zeros(len(p))
    idx = np.nonzero(u > F)[0]
    it = 0
    while len(idx) and it < 1000:
        it += 1
        p[idx] = p[idx] * lam[idx] / LD(it)
        prev[idx] = F[idx]
        y = p[idx] - c[idx]                                       # Kahan: F + c carries the sum beyond the 64-bit mantissa
        t = F[idx] + y
        c[idx] = (t - F[idx]) - y
        F[idx] = t
        n[idx] = it
        idx = idx[u[idx] > F[idx]]
    und = (F - u < BAND_CDF) | (u - prev < BAND_CDF)
    und[idx] = True
    return n.reshape(shape), und.reshape(shape)


def poisson_small_f64(lam, u):
    """The device loop itself, in plain binary64 (one rounding per operation)."""
    lam, u = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(u, dtype=np.float64))
    lam, u = lam.ravel(), u.ravel()
    p = np.exp(-lam)
    F = p.copy()
    n = np.zeros(len(p))
    idx = np.nonzero(u > F)[0]
    it = 0
    while len(idx) and it < 1000:
        it += 1
        p[idx] = p[idx] * (lam[idx] / float(it))
        F[idx] = F[idx] + p[idx]
        n[idx] = it
        idx = idx[u[idx] > F[idx]]
    return n


def poisson_ptrs(lam, seed, D, b, mutant=None):
    """poisson_ptrs(lam, D, b) for arrays of draws -> (k float64, undecided bool)."""
    lam, D, b = np.broadcast_arrays(np.asarray(lam, dtype=np.float64), np.asarray(D, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    shape = lam.shape
    lam, D, b = lam.ravel(), D.ravel(), b.ravel()
    k0, k1 = _key(seed)
    dlo, dhi = _dataset_words(D, mutant)
    slam, loglam = np.sqrt(lam), np.log(lam)
    bb = 0.931 + 2.53 * slam
    aa = -0.059 + 0.02483 * bb
    invalpha = 1.1239 + 1.1328 / (bb - 3.4)
    vr = 0.9277 - 3.6224 / (bb - 2.0)
    shift = 0.5 if mutant == 'shift05' else 0.43
    us_cut = 0.13 if mutant == 'us13' else 0.013
    out = np.floor(lam)
    und = np.zeros(len(lam), bool)
    act = np.arange(len(lam))
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for attempt in range(4096):
            if not len(act):
                break
            a = attempt if mutant == 'attempt0' else attempt + 1
            r0, r1, r2, r3 = philox_v(b[act], b[act] >> _U64(32), dlo[act], dhi[act] | _U64(a << 16), k0, k1)
            U, V = u53(r0, r1) - 0.5, u53(r2, r3)
            us = 0.5 - np.abs(U)
            x = (2.0 * aa[act] / us + bb[act]) * U + lam[act] + shift
            k = np.floor(x)
            near = np.abs(x - np.rint(x)) <= BAND_FLOOR * np.abs(x)
            squeeze = us >= 0.07
            in_band = near | (squeeze & (np.abs(V - vr[act]) <= BAND_VR))
            acc = squeeze & (V <= vr[act])
            rej = ~acc & ((k < 0.0) | ((us < us_cut) & (V > us)))
            test = ~acc & ~rej
            lhs = np.log(V) + np.log(invalpha[act]) - np.log(aa[act] / (us * us) + bb[act])
            rhs = -lam[act] + k * loglam[act] - gammaln(k + 1.0)
            in_band |= test & (np.abs(lhs - rhs) <= BAND_LOG * np.maximum(1.0, np.abs(rhs)))
            acc |= test & (lhs <= rhs)
            done = acc | in_band
            out[act[acc]] = k[acc]
            und[act[in_band]] = True
            act = act[~done]
    return out.reshape(shape), und.reshape(shape)


def event_count(M, seed, D, mutant=None):
    """N of stream B (and N_s of bi_simulate_events): -> (N float64, undecided), one per dataset number."""
    D = np.atleast_1d(np.asarray(D, dtype=np.uint64))
    if M >= 10.0:
        return poisson_ptrs(np.full(len(D), M), seed, D, np.full(len(D), EVENT_COUNT_BIN, dtype=np.uint64), mutant)
    k0, k1 = _key(seed)
    dlo, dhi = _dataset_words(D, mutant)
    r0, r1, _, _ = philox_v(0xFFFFFFFF, EV_TAG, dlo, dhi, k0, k1)
    return poisson_quantile(np.full(len(D), M), u53(r0, r1))


# ---- stream A: one draw per bin -----------------------------------------------------------------------------------------

class Replay:
    """What the oracle expects of a call: counts [n_toys, B], and which draws are undecided."""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def share(self):
        return self.undecided / max(self.draws, 1)


def per_bin_toys(mu, seed, datasets, mutant=None):
    mu = np.asarray(mu, dtype=np.float64)
    B = len(mu)
    datasets = np.atleast_1d(np.asarray(datasets, dtype=np.uint64))
    k0, k1 = _key(seed)
    counts = np.zeros((len(datasets), B))
    und = np.zeros((len(datasets), B), bool)
    small = (mu > 0.0) & (mu < 10.0)
    large = mu >= 10.0
    q = np.arange((B + 1) // 2, dtype=np.uint64)
    bins = np.arange(B, dtype=np.uint64)
    for i, D in enumerate(datasets):
        dlo, dhi = _dataset_words(D, mutant)
        r0, r1, r2, r3 = philox_v(q, q >> _U64(32), dlo, dhi, k0, k1)
        u = np.empty(2 * len(q))
        u[0::2] = u53(r0, r1)
        u[1::2] = u53(r0, r1) if mutant == 'odd01' else u53(r2, r3)
        u = u[:B]
        if small.any():
            counts[i, small], und[i, small] = poisson_quantile(mu[small], u[small])
        if large.any():
            counts[i, large], und[i, large] = poisson_ptrs(mu[large], seed, np.full(int(large.sum()), D, dtype=np.uint64), bins[large], mutant)
    return Replay(path=0, counts=counts, und_bins=und, und_toy=und.any(axis=1), draws=int((small | large).sum()) * len(datasets),
                  undecided=int(und.sum()), mu=mu)


# ---- stream B: event by event -------------------------------------------------------------------------------------------

def exact_running_sums(mu):
    """Running sums of mu in long double, left to right (exact for the dyadic expectations of the tests)."""
    return np.cumsum(np.asarray(mu, dtype=np.float64).astype(LD))


def find_bins(F, total, u, mutant=None):
    """first b with F[b] > u total, clamped -> (bin, undecided)"""
    target = np.asarray(u, dtype=np.float64).astype(LD) * LD(total)
    b = np.searchsorted(F, target, side='left' if mutant == 'bisect_lt' else 'right')
    b = np.minimum(b, len(F) - 1)
    band = LD(BAND_BISECT) * LD(total)
    below = np.where(b > 0, F[np.maximum(b - 1, 0)], LD(-1) - band)
    und = (np.abs(F[b] - target) < band) | (np.abs(target - below) < band)
    return b.astype(np.int64), und


def sort_size(N):
    n2 = 1024
    while n2 < N:
        n2 <<= 1
    return n2


def encode_runs(bins, B, mutant=None):
    """The toy's counts from its events' bins: sort, run-length encode.  The mutants restate the device's layout: 512 threads
    own contiguous segments of the n2 sorted keys (pads 0xFFFFFFFF behind the events)."""
    N = len(bins)
    counts = np.bincount(bins, minlength=B).astype(np.float64)
    if mutant == 'rle_drop' and N:
        keys = np.sort(bins)
        seg = sort_size(N) // 512
        heads = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0]
        length = np.diff(np.r_[heads, N])
        length = np.minimum(length, (heads // seg + 1) * seg - heads)           # the run ends with its thread's segment
        counts = np.zeros(B)
        counts[keys[heads]] = length
    if mutant == 'pad_count':
        key_bits = 1
        while (1 << key_bits) < B:
            key_bits += 1
        pad = 0xFFFFFFFF & ((1 << key_bits) - 1)
        if pad < B:
            counts[pad] += sort_size(N) - N
    return counts


def event_toys(mu, seed, datasets, mutant=None, forced_u=None):
    """forced_u: {event number: uniform} replaces the stream's uniform of those events (crafted ties, CPU tests only)."""
    mu = np.asarray(mu, dtype=np.float64)
    B = len(mu)
    datasets = np.atleast_1d(np.asarray(datasets, dtype=np.uint64))
    k0, k1 = _key(seed)
    F = exact_running_sums(mu)
    M = float(F[-1])
    N, und_N = event_count(M, seed, datasets, mutant)
    counts = np.zeros((len(datasets), B))
    decided = np.zeros((len(datasets), B))
    n_und = np.zeros(len(datasets), dtype=np.int64)
    for i, D in enumerate(datasets):
        n = int(N[i])
        e = np.arange(n, dtype=np.uint64)
        dlo, dhi = _dataset_words(D, mutant)
        r0, r1, _, _ = philox_v(e, EV_TAG, dlo, dhi, k0, k1)
        u = u53(r0, r1)
        for ev, val in (forced_u or {}).items():
            if ev < n:
                u[ev] = val
        b, und = find_bins(F, M, u, mutant)
        counts[i] = encode_runs(b, B, mutant)
        decided[i] = np.bincount(b[~und], minlength=B)
        n_und[i] = int(und.sum())
    return Replay(path=1, counts=counts, decided=decided, N=N, und_N=und_N, und_toy=und_N | (n_und > 0), M=M,
                  draws=len(datasets) + int(N.sum()), undecided=int(und_N.sum() + n_und.sum()), mu=mu)


# ---- the comparison -----------------------------------------------------------------------------------------------------

def compare_toys(dev, rep, what=''):
    """dev [n_toys, B]: the device's dense counts of the toys `rep` describes -> (draws, undecided, mismatches).  Asserts: no
    mismatch among decided draws; the non-empty-bin lists of every toy without an undecided draw equal the oracle's; no
    event in a bin of zero expectation (undecided draws included); at most CAP of the draws undecided."""
    dev = np.asarray(dev, dtype=np.float64)
    assert dev.shape == rep.counts.shape, (what, dev.shape, rep.counts.shape)
    lines = []
    mismatches = 0
    dead = rep.mu == 0.0
    if rep.path == 1:
        dead = dead.copy()
        dead[-1] = False                                            # (the clamp may put an event into the last bin)
    bad = np.argwhere(dev[:, dead] != 0)
    if len(bad):
        mismatches += len(bad)
        lines.append("events where mu = 0: toy %d, bin %d" % (bad[0][0], np.nonzero(dead)[0][bad[0][1]]))
    if rep.path == 0:
        wrong = ~rep.und_bins & ~(dev == rep.counts)
        mismatches += int(wrong.sum())
        for t, b in np.argwhere(wrong)[:5]:
            lines.append("toy %d bin %d (mu = %r): device %r, oracle %r" % (t, b, rep.mu[b], dev[t, b], rep.counts[t, b]))
    else:
        for t in range(len(dev)):
            if not rep.und_N[t] and dev[t].sum() != rep.N[t]:
                mismatches += 1
                lines.append("toy %d: device holds %r events, oracle N = %r" % (t, dev[t].sum(), rep.N[t]))
            short = np.nonzero(dev[t] < rep.decided[t])[0]
            if len(short):
                mismatches += len(short)
                lines.append("toy %d bin %d: device %r < %r decided events" % (t, short[0], dev[t, short[0]], rep.decided[t, short[0]]))
    for t in np.nonzero(~rep.und_toy)[0]:
        (db,), (ob,) = np.nonzero(dev[t]), np.nonzero(rep.counts[t])
        if not (np.array_equal(db, ob) and np.array_equal(dev[t, db], rep.counts[t, ob])):
            diff = np.nonzero(dev[t] != rep.counts[t])[0]
            if rep.path == 1:
                mismatches += len(diff)
            lines.append("toy %d: non-empty-bin lists differ, first at bin %d: device %r, oracle %r" %
                         (t, diff[0], dev[t, diff[0]], rep.counts[t, diff[0]]))
    assert mismatches == 0 and not lines, "%s: %d mismatches among %d draws (%d undecided)\n  %s" % (
        what, mismatches, rep.draws, rep.undecided, "\n  ".join(lines[:12]))
    assert rep.undecided <= CAP * rep.draws, "%s: undecided share %g (%d of %d) above the cap %g" % (
        what, rep.share, rep.undecided, rep.draws, CAP)
    return rep.draws, rep.undecided, mismatches


# ---- bi_simulate_events -------------------------------------------------------------------------------------------------

def bin_volumes(edges):
    vol = np.ones([len(e) - 1 for e in edges])
    for ax, e in enumerate(edges):
        shape = [1] * len(edges)
        shape[ax] = len(e) - 1
        vol = vol * np.diff(e).reshape(shape)                       # in axis order from 1
    return vol.ravel()


def simulate_events(dens, edges, rates, seed, mutant=None):
    """dens [S, B]: the morphed densities; rates [S] -> Replay: n [S], source [N], bin [N], coords [k, N], undecided [N]."""
    dens = np.asarray(dens, dtype=np.float64)
    S, B = dens.shape
    edges = [np.asarray(e, dtype=np.float64) for e in edges]
    nb = [len(e) - 1 for e in edges]
    k = len(edges)
    stride = [int(np.prod(nb[i + 1:], dtype=np.int64)) for i in range(k)]
    v = dens * bin_volumes(edges)
    pmf = np.where(v > 0.0, v, 0.0)
    k0, k1 = _key(seed)
    n = np.zeros(S)
    und_n = np.zeros(S, bool)
    for s in range(S):
        assert 0.0 <= rates[s] < SIM_MAX_RATE
        if rates[s] > 0.0:
            a, b = event_count(float(rates[s]), int(seed) ^ SIM_COUNT_KEY, [s])
            n[s], und_n[s] = a[0], b[0]
    source, bins, coords, und = [], [], [], []
    for s in range(S):
        j = np.arange(int(n[s]), dtype=np.uint64)
        F = np.cumsum(pmf[s].astype(LD))
        r0, r1, _, _ = philox_v(j, j >> _U64(32), s, SIM_TAG, k0, k1)
        b, ub = find_bins(F, F[-1], u53(r0, r1))
        rem = b.copy()
        x = np.empty((k, len(j)))
        idx = []
        for ax in range(k):
            idx.append(rem // stride[ax])
            rem = rem - idx[-1] * stride[ax]
        if mutant == 'axes_swapped':
            idx = [np.minimum(i, nb[ax] - 1) for ax, i in enumerate(idx[::-1])]
        for ax in range(k):
            r0, r1, _, _ = philox_v(j, j >> _U64(32), s | (ax << 24), SIM_TAG + 1, k0, k1)
            e = edges[ax]
            x[ax] = e[idx[ax]] + u53(r0, r1) * (e[idx[ax] + 1] - e[idx[ax]])
        source.append(np.full(len(j), s, dtype=np.int32))
        bins.append(b)
        coords.append(x)
        und.append(ub)
    N = int(n.sum())
    return Replay(n=n, und_n=und_n, source=np.concatenate(source), bin=np.concatenate(bins), coords=np.concatenate(coords, axis=1),
                  und=np.concatenate(und), draws=S + N * (1 + k), undecided=int(und_n.sum()) + int(np.concatenate(und).sum()) * (1 + k),
                  edges=edges, stride=stride)


def compare_events(dev_n, dev_coords, dev_source, rep, what=''):
    """-> (draws, undecided, mismatches); the events are compared in drawn order (source by source, event j of source s at
    first_s + j).  Asserts as compare_toys does; a position must lie within 2 ulp of the oracle's and inside its bin."""
    dev_n = np.asarray(dev_n)
    assert rep.undecided <= CAP * rep.draws, \
        "%s: undecided share %g (%d of %d) above the cap %g" % (what, rep.share, rep.undecided, rep.draws, CAP)
    lines = []
    ok_n = rep.und_n | (dev_n == rep.n)
    mismatches = int((~ok_n).sum())
    if mismatches:
        lines.append("events per source: device %r, oracle %r" % (list(dev_n), list(rep.n)))
    if not rep.und_n.any() and not mismatches:
        if not np.array_equal(dev_source, rep.source):
            mismatches += int(np.sum(dev_source != rep.source))
            lines.append("source of the events differs, first at event %d" % np.nonzero(dev_source != rep.source)[0][0])
        else:
            k = len(rep.edges)
            rem = rep.bin.copy()
            for ax in range(k):
                i = rem // rep.stride[ax]
                rem = rem - i * rep.stride[ax]
                e = rep.edges[ax]
                x, want = dev_coords[ax], rep.coords[ax]
                tol = 2 * np.spacing(np.abs(want))
                wrong = ~rep.und & ~((np.abs(x - want) <= tol) & (x >= e[i]) & (x <= e[i + 1]))
                mismatches += int(wrong.sum())
                for ev in np.nonzero(wrong)[0][:3]:
                    lines.append("event %d (source %d, bin %d) axis %d: device %r, oracle %r in [%r, %r]" %
                                 (ev, rep.source[ev], rep.bin[ev], ax, x[ev], want[ev], e[i[ev]], e[i[ev] + 1]))
    assert mismatches == 0, "%s: %d mismatches among %d draws (%d undecided)\n  %s" % (what, mismatches, rep.draws, rep.undecided,
                                                                                     "\n  ".join(lines[:12]))
    return rep.draws, rep.undecided, mismatches
