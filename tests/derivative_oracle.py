"""An exact derivative oracle for tests: value, gradient and Hessian over theta = (z [d], rate_scale [S]) of the binned
Poisson and the extended unbinned likelihood, the value and gradient of the Beeston-Barlow likelihood, and for every output
entry a condition number `cond` that bounds how far a correct float64 implementation may land from the exact result:

    |device - oracle| <= C * 2**-52 * cond        (check_entries)

Every quantity is carried as a pair (value, weight) through running-error arithmetic (class T): a sum's weight is the sum of
its summands' weights, a product's the product rule over the absolute values, and every operation adds the magnitude of its
own result.  That is the expression evaluated with every summand replaced by its absolute value, extended to quotients, logs
and square roots, so `cond` grows with exactly the cancellation a kernel has to live with (n / mu - 1 weighs like
n / mu + 1; the Gram term like sum n |d_q mu d_r mu| / mu^2; the Beeston-Barlow root like (|b| + sqrt(disc)) / |A|).

Inside a grid cell the interpolation is multilinear: mu_b = sum over the cell's corners c and the sources s of
w_c(z) u_s(z) rs_s P_cs(b), with u_s(z) the interpolated rate and w_c the product of the per-axis weights t or 1 - t.  Every
derivative of mu_b is one more coefficient per (c, s) over the same rows, from the derivatives of w_c and u_s.  The cell
convention is `oracle.blueice_oracle.find_cell`'s: g[k] <= z < g[k+1], the last cell closed; single-anchor axes have zero
derivative.  Per-bin terms are summed with math.fsum per block of bins (no [F, F, B] array; ~300 k bins stay small), so
the oracle's own rounding does not grow with B.

Imports only `oracle/` and numpy / scipy.special.  Test infrastructure only."""
import math

import numpy as np
from scipy.special import gammaln

from oracle import blueice_oracle as orc

EPS = 2.0 ** -52
C_POISSON = 256          # binned Poisson and extended unbinned likelihoods
C_BB = 256               # Beeston-Barlow: the root's cancellation is inside cond (see bb_gradient), not in C
BLOCK = 32768            # bins per block


class T:
    """A float64 array with its running-error weight: |exact - computed| <~ EPS * a for any correct evaluation order."""
    __slots__ = ('v', 'a')

    def __init__(self, v, a=None):
        self.v = np.asarray(v, dtype=float)
        self.a = np.abs(self.v) if a is None else np.asarray(a, dtype=float)

    @staticmethod
    def of(x):
        return x if isinstance(x, T) else T(x, np.zeros(np.shape(x)))      # exact inputs

    def __add__(self, o):
        o = T.of(o)
        v = self.v + o.v
        return T(v, self.a + o.a + np.abs(v))
    __radd__ = __add__

    def __neg__(self):
        return T(-self.v, self.a)

    def __sub__(self, o):
        return self + (-T.of(o))

    def __rsub__(self, o):
        return T.of(o) - self

    def __mul__(self, o):
        o = T.of(o)
        v = self.v * o.v
        return T(v, self.a * np.abs(o.v) + np.abs(self.v) * o.a + np.abs(v))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = T.of(o)
        with np.errstate(all='ignore'):
            v = self.v / o.v
            a = self.a / np.abs(o.v) + np.abs(v) * o.a / np.abs(o.v) + np.abs(v)
        return T(v, a)

    def __rtruediv__(self, o):
        return T.of(o) / self

    def __pow__(self, k):
        assert k == 2
        return self * self

    def __getitem__(self, k):
        return T(self.v[k], self.a[k])

    def sqrt(self):
        with np.errstate(all='ignore'):
            s = np.sqrt(self.v)
            return T(s, np.where(s > 0, self.a / (2 * s), 0.0) + s)

    def log(self):
        with np.errstate(all='ignore'):
            lv = np.log(self.v)
            return T(lv, self.a / np.abs(self.v) + np.abs(lv))

    def where(self, mask, other):
        other = T.of(other)
        return T(np.where(mask, self.v, other.v), np.where(mask, self.a, other.a))


def tsum(xs):
    """Sum of a list of T (same shape)."""
    out = xs[0]
    for x in xs[1:]:
        out = out + x
    return out


def tmatmul(c, r):
    """[K, N] x [N, b]: the products' weights plus one rounding of every partial sum (bounded by the summands' sum)."""
    v = c.v @ r.v
    absprod = np.abs(c.v) @ np.abs(r.v)
    return T(v, c.a @ np.abs(r.v) + np.abs(c.v) @ r.a + absprod * c.v.shape[-1] ** 0.5 + np.abs(v))


class Acc:
    """Per-entry sums over bin blocks: the values with math.fsum (one rounding per block), the weights plainly."""

    def __init__(self, shape):
        self.parts = np.empty(shape, dtype=object)
        for idx in np.ndindex(shape):
            self.parts[idx] = []
        self.a = np.zeros(shape)

    def add(self, x):
        """x: T of shape shape + (b,)."""
        for idx in np.ndindex(self.a.shape):
            self.parts[idx].append(math.fsum(x.v[idx].tolist()))
        self.a += x.a.sum(axis=-1)

    def add_scalar(self, x):
        for idx in np.ndindex(self.a.shape):
            self.parts[idx].append(float(x.v[idx]))
        self.a += x.a

    def result(self):
        v = np.zeros(self.a.shape)
        for idx in np.ndindex(self.a.shape):
            v[idx] = math.fsum(self.parts[idx])
        return v, self.a


# ---- the cell, its corners and the coefficient columns ------------------------------------------------------------

class Cell:
    """The grid cell of z and the corner weights' derivatives.  `anchor_z` [d arrays]; `cell_shift` {axis: -1} moves the
    point to the cell below on that axis (a wrong cell at an anchor, for the tests of the bound)."""

    def __init__(self, anchor_z, z, cell_shift=None):
        z = np.asarray(z, dtype=float)
        self.d = d = len(anchor_z)
        self.eff = [i for i in range(d) if len(anchor_z[i]) > 1]
        self.k, self.t, self.h = [], [], []
        for i, g in enumerate(anchor_z):
            g = np.asarray(g, dtype=float)
            if len(g) == 1:
                self.k.append(0), self.t.append(None), self.h.append(None)
                continue
            k, _ = orc.find_cell(g, z[i])
            k += (cell_shift or {}).get(i, 0)
            lo, hi = T.of(g[k]), T.of(g[k + 1])
            width = hi - lo
            self.k.append(k)
            self.t.append((T.of(z[i]) - lo) / width)
            self.h.append(width)
        de = len(self.eff)
        self.nc = 1 << de
        # corner c: bit j of c = upper anchor on effective axis j
        self.index = []
        for c in range(self.nc):
            idx = list(self.k)
            for j, i in enumerate(self.eff):
                idx[i] = self.k[i] + ((c >> j) & 1)
            self.index.append(tuple(idx))

        def factor(c, j, deriv):
            up = (c >> j) & 1
            i = self.eff[j]
            if deriv:
                return (1.0 if up else -1.0) / self.h[i]
            return self.t[i] if up else 1.0 - self.t[i]

        def prod(c, derivs):
            out = T.of(1.0)
            for j in range(de):
                out = out * factor(c, j, j in derivs)
            return out

        # weights, first derivatives [corner][axis d], second [corner][(i, j)] for i < j (effective axes only; d_ii w = 0)
        self.w = [prod(c, ()) for c in range(self.nc)]
        zero = T.of(0.0)
        self.dw = [[zero] * d for _ in range(self.nc)]
        self.d2w = [dict() for _ in range(self.nc)]
        for c in range(self.nc):
            for j, i in enumerate(self.eff):
                self.dw[c][i] = prod(c, (j,))
                for jj in range(j + 1, de):
                    self.d2w[c][(i, self.eff[jj])] = prod(c, (j, jj))


def interp_derivs(cell, values):
    """values [A.., *rest] -> interpolated f, df [d] and d2f {(i, j), i < j} as T over `rest` (u_s: the rates per source)."""
    d = cell.d
    rows = [T.of(np.asarray(values[idx], dtype=float)) for idx in cell.index]
    f = tsum([cell.w[c] * rows[c] for c in range(cell.nc)])
    df = [tsum([cell.dw[c][i] * rows[c] for c in range(cell.nc)]) for i in range(d)]
    d2f = {}
    for i in range(d):
        for j in range(i + 1, d):
            if (i, j) in cell.d2w[0]:
                d2f[(i, j)] = tsum([cell.d2w[c][(i, j)] * rows[c] for c in range(cell.nc)])
            else:
                d2f[(i, j)] = T.of(np.zeros_like(f.v))
    return f, df, d2f


def pairs(F):
    return [(q, r) for q in range(F) for r in range(q, F)]


def coefficient_columns(cell, mus, rs, second=True):
    """-> (coef T [K, nc * S], rates r T [S], dr [F] of T [S], d2r {(q, r)} of T [S]).  Row k = corner * S + s; column 0
    mu, columns 1..F the first derivatives (axes then rates), then the pairs q <= r of `pairs(F)` when `second`."""
    d = cell.d
    rs = np.asarray(rs, dtype=float)
    S = len(rs)
    F = d + S
    u, du, d2u = interp_derivs(cell, mus)
    zeroS = T.of(np.zeros(S))
    Rs = T.of(rs)
    r = u * Rs
    dr = [du[i] * Rs for i in range(d)] + [T(np.where(np.arange(S) == t, u.v, 0.0), np.where(np.arange(S) == t, u.a, 0.0))
                                           for t in range(S)]
    d2r = {}
    for q, p in pairs(F):
        if q < d and p < d:
            d2r[(q, p)] = d2u[(q, p)] * Rs if q != p else zeroS
        elif q < d:
            t = p - d
            d2r[(q, p)] = T(np.where(np.arange(S) == t, du[q].v, 0.0), np.where(np.arange(S) == t, du[q].a, 0.0))
        else:
            d2r[(q, p)] = zeroS
    cols = []
    sel = lambda x, s: T(x.v[s], x.a[s])
    for c in range(cell.nc):
        w, dw, d2w = cell.w[c], cell.dw[c], cell.d2w[c]
        for s in range(S):
            col = [w * sel(r, s)]
            first = [dw[i] * sel(r, s) + w * sel(dr[i], s) for i in range(d)]       # d_i (w r_s)
            first += [w * sel(dr[d + t], s) for t in range(S)]
            col += first
            if second:
                for q, p in pairs(F):
                    if q < d and p < d:
                        v = dw[q] * sel(dr[p], s) + dw[p] * sel(dr[q], s)
                        if q != p:
                            v = v + (d2w[(q, p)] * sel(r, s) if (q, p) in d2w else 0.0) + w * sel(d2r[(q, p)], s)
                    elif q < d:
                        v = dw[q] * sel(dr[p], s) + w * sel(d2r[(q, p)], s)
                    else:
                        v = T.of(0.0)
                    col.append(v)
            cols.append(col)
    K = len(cols[0])
    coef = T(np.array([[cols[k][j].v for k in range(len(cols))] for j in range(K)], dtype=float),
             np.array([[cols[k][j].a for k in range(len(cols))] for j in range(K)], dtype=float))
    return coef, r, dr, d2r


def _rows(model, cell, b0, b1, S):
    """[nc * S, b] template rows of the cell's corners over bins b0:b1 (model['ps'] [A.., S, *bins])."""
    ps = model['ps']
    out = np.empty((cell.nc * S, b1 - b0))
    for c, idx in enumerate(cell.index):
        out[c * S:(c + 1) * S] = np.asarray(ps[idx], dtype=float).reshape(S, -1)[:, b0:b1]
    return out


def n_bins(model):
    d = len(model['anchor_z'])
    return int(np.prod(np.shape(model['ps'])[d + 1:], dtype=np.int64))


# ---- binned Poisson and extended unbinned ---------------------------------------------------------------------------

def derivatives(model, z, rs, counts=None, unbinned=False, outlier=1e-12, hessian=True, mutate=None):
    """-> dict(ll, grad [F], hess [F, F] (if `hessian`) and their conds ll_cond, grad_cond, hess_cond).

    Binned (counts [*bins]): ll = sum_b n log mu - mu - lgamma(n + 1), g = sum d mu (n / mu - 1), H = sum d2 mu (n / mu - 1)
    - n d mu d mu / mu^2 (bins with n = 0 have no 1 / mu).  Unbinned (model['ps'] [A.., S, N_events]): ll = -sum_s r_s + sum_e
    log lambda_e with nan pdf terms dropped per (event, source), and events whose lambda is not > 0 on the outlier clamp (a
    constant).  `mutate` (tests of the bound only): {'coef': (row, col, rel)} scales one corner's coefficient; {'drop_bin': b}
    leaves bin b out; {'gram_flip': (q, r)} flips the sign of one Gram pair; {'cell_shift': {axis: -1}}."""
    mutate = mutate or {}
    d = len(model['anchor_z'])
    rs = np.asarray(rs, dtype=float)
    S = len(rs)
    F = d + S
    cell = Cell(model['anchor_z'], z, mutate.get('cell_shift'))
    coef, r, dr, d2r = coefficient_columns(cell, model['mus'], rs, second=hessian)
    if 'coef' in mutate:
        k, j, rel = mutate['coef']
        coef.v[j, k] *= 1.0 + rel
    P2 = pairs(F)
    B = n_bins(model)
    acc_ll, acc_g = Acc(()), Acc((F,))
    acc_h = Acc((len(P2),)) if hessian else None
    n_all = None if unbinned else np.asarray(counts, dtype=float).ravel()
    n_clamped = 0
    for b0 in range(0, B, BLOCK):
        b1 = min(B, b0 + BLOCK)
        rows = _rows(model, cell, b0, b1, S)
        keep = np.ones(b1 - b0, bool)
        if 'drop_bin' in mutate and b0 <= mutate['drop_bin'] < b1:
            keep[mutate['drop_bin'] - b0] = False
        if unbinned:
            # nan pdf terms are dropped per (event, source): a nan at any corner makes the interpolated term nan
            bad = np.zeros((S, b1 - b0), bool)
            for c in range(cell.nc):
                bad |= np.isnan(rows[c * S:(c + 1) * S])
            for c in range(cell.nc):
                rows[c * S:(c + 1) * S][bad] = 0.0
        X = tmatmul(coef, T(rows))
        mu = X[0]
        if unbinned:
            live = (mu.v > 0) if outlier != 0 else np.ones(b1 - b0, bool)
            n_clamped += int((~live & keep).sum())
            live &= keep
            X = X[:, live]
            mu = X[0]
            inv = 1.0 / mu
            lg = mu.log()
            acc_ll.add(lg)
            fw = inv                                    # d ll / d lambda
            nw = T.of(np.ones(len(inv.v)))              # Gram weight: 1 per event
        else:
            n = n_all[b0:b1][keep]
            X = X[:, keep]
            mu = X[0]
            pos = n > 0
            with np.errstate(all='ignore'):
                inv = (1.0 / mu).where(pos, 0.0)
                nlog = (T.of(n) * mu.log()).where(pos, 0.0)
            term = nlog - mu - T.of(gammaln(n + 1))
            acc_ll.add(term)
            fw = T.of(n) * inv - 1.0
            nw = T.of(n)
        dmu = X[1:1 + F]
        acc_g.add(dmu * T(fw.v[None], fw.a[None]))
        if hessian:
            d2 = X[1 + F:]
            fwb = T(fw.v[None], fw.a[None])
            # (d_q mu / mu) (d_r mu / mu) n: no 1 / mu^2, which overflows for the pdfs' far tails
            sl = dmu * T(inv.v[None], inv.a[None])
            qi = np.array([q for q, _ in P2])
            ri = np.array([p for _, p in P2])
            gram = sl[qi] * sl[ri] * T(nw.v[None], nw.a[None])
            if 'gram_flip' in mutate:
                j = P2.index(tuple(sorted(mutate['gram_flip'])))
                gram.v[j] = -gram.v[j]
            acc_h.add(d2 * fwb - gram)
    if unbinned:
        # -sum_s r_s and its derivatives; the clamped events' log(outlier) is a constant
        acc_ll.add_scalar(T(-np.array(math.fsum(r.v.tolist())), np.array(r.a.sum())))
        if n_clamped:
            acc_ll.add_scalar(T(np.array(n_clamped * math.log(outlier)), np.array(abs(n_clamped * math.log(outlier)))))
        acc_g.add_scalar(T(-np.array([math.fsum(x.v.tolist()) for x in dr]), np.array([x.a.sum() for x in dr])))
        if hessian:
            acc_h.add_scalar(T(-np.array([math.fsum(d2r[pq].v.tolist()) for pq in P2]), np.array([d2r[pq].a.sum() for pq in P2])))
    out = {}
    v, a = acc_ll.result()
    out['ll'], out['ll_cond'] = float(v), float(a)
    out['grad'], out['grad_cond'] = acc_g.result()
    if hessian:
        hv, ha = acc_h.result()
        H, Hc = np.zeros((F, F)), np.zeros((F, F))
        for j, (q, p) in enumerate(P2):
            H[q, p] = H[p, q] = hv[j]
            Hc[q, p] = Hc[p, q] = ha[j]
        out['hess'], out['hess_cond'] = H, Hc
    return out


# ---- Beeston-Barlow -------------------------------------------------------------------------------------------------

def bb_gradient(model, z, rs, counts, bb_source, mutate=None):
    """-> dict(ll, grad, ll_cond, grad_cond) of the binned likelihood with the Beeston-Barlow adjustment of source i.

    mu_b = U_b + A_b p_b, p_b = r_i P_b / a_b (U: the other sources, P: source i's template, a: its Monte-Carlo counts), A_b
    the second root of Q(A) = p (p + 1) A^2 + (U (p + 1) - p (a + n)) A - a U = 0, differentiated implicitly:
    dA = -(Q_p dp + Q_U dU + Q_a da) / Q_A.  Where U_b == 0 exactly the reference's special case A = (n + a) / (1 + p_cal)
    with the scalar p_cal = r_i / N, N = sum_b a_b (N moves with z too).

    The cond of A carries the root's cancellation: A is evaluated as the reference writes it, (-b + sqrt(disc)) / (2 p (p +
    1)), so its weight is (|b| + sqrt(disc) + disc's summands / sqrt(disc)) / (2 p (p + 1)) -- about |A| where b < 0 and up to
    |b| / |A| times that where the root is the small difference of two large terms (U >> a p).  With that inside cond the
    constant is the plain one, C_BB = C_POISSON."""
    mutate = mutate or {}
    d = len(model['anchor_z'])
    rs = np.asarray(rs, dtype=float)
    S = len(rs)
    F = d + S
    i = int(bb_source)
    cell = Cell(model['anchor_z'], z, mutate.get('cell_shift'))
    coef, r, dr, _ = coefficient_columns(cell, model['mus'], rs, second=False)     # U and its derivatives: sources != i
    for c in range(cell.nc):
        coef.v[:, c * S + i] = 0.0
        coef.a[:, c * S + i] = 0.0
    if 'coef' in mutate:
        k, j, rel = mutate['coef']
        coef.v[j, k] *= 1.0 + rel
    # P_i and a: interpolated rows of source i (weights only; the rates do not move them)
    wcol = T(np.array([[cell.w[c].v for c in range(cell.nc)]] + [[cell.dw[c][q].v for c in range(cell.nc)] for q in range(d)],
                      dtype=float),
             np.array([[cell.w[c].a for c in range(cell.nc)]] + [[cell.dw[c][q].a for c in range(cell.nc)] for q in range(d)],
                      dtype=float))
    B = n_bins(model)
    n_all = np.asarray(counts, dtype=float).ravel()

    def rows_i(key, b0, b1):
        out = np.empty((cell.nc, b1 - b0))
        for c, idx in enumerate(cell.index):
            out[c] = np.asarray(model[key][idx], dtype=float).reshape(S, -1)[i, b0:b1]
        return out

    # first pass: N = sum_b a_b and its shape derivatives
    accN = Acc((1 + d,))
    for b0 in range(0, B, BLOCK):
        b1 = min(B, b0 + BLOCK)
        accN.add(tmatmul(wcol, T(rows_i('n_model', b0, b1))))
    Nv, Na = accN.result()
    N = T(Nv[0], Na[0])
    dN = [T(Nv[1 + q], Na[1 + q]) for q in range(d)] + [T.of(0.0)] * S
    ri = r[i]
    dri = [dr[q][i] for q in range(F)]
    p_cal = ri / N
    dp_cal = [dri[q] / N - ri * dN[q] / (N * N) for q in range(F)]
    acc_ll, acc_g = Acc(()), Acc((F,))
    for b0 in range(0, B, BLOCK):
        b1 = min(B, b0 + BLOCK)
        n = T.of(n_all[b0:b1])
        X = tmatmul(coef, T(_rows(model, cell, b0, b1, S)))
        Pw = tmatmul(wcol, T(rows_i('ps', b0, b1)))
        aw = tmatmul(wcol, T(rows_i('n_model', b0, b1)))
        U, Pv, av = X[0], Pw[0], aw[0]
        dU = [X[1 + q] for q in range(F)]
        zero = T.of(np.zeros(b1 - b0))
        dP = [Pw[1 + q] for q in range(d)] + [zero] * S
        da = [aw[1 + q] for q in range(d)] + [zero] * S
        p = ri * Pv / av
        dp = [(dri[q] * Pv + ri * dP[q]) / av - p * da[q] / av for q in range(F)]
        # the physical root as the reference evaluates it (blueice_oracle.beeston_barlow_root2) and its implicit derivative
        disc = orc._bb_disc(av, p, U, n)
        bq = U * p + U - av * p - n * p
        A2 = (-bq + disc.sqrt()) / (2.0 * p * (p + 1.0))
        QA = 2.0 * p * (p + 1.0) * A2 + U * (p + 1.0) - p * (av + n)
        Qp = (2.0 * p + 1.0) * A2 * A2 + (U - (av + n)) * A2
        QU = (p + 1.0) * A2 - av
        Qa = -p * A2 - U
        dA2 = [-(Qp * dp[q] + QU * dU[q] + Qa * da[q]) / QA for q in range(F)]
        # the special case where the other sources expect exactly nothing
        zu = U.v == 0
        As = (n + av) / (1.0 + p_cal)
        dAs = [da[q] / (1.0 + p_cal) - (n + av) * dp_cal[q] / ((1.0 + p_cal) * (1.0 + p_cal)) for q in range(F)]
        A = A2.where(~zu, As)
        dA = [dA2[q].where(~zu, dAs[q]) for q in range(F)]
        mu = U + A * p
        dmu = [dU[q] + dA[q] * p + A * dp[q] for q in range(F)]
        keep = np.ones(b1 - b0, bool)
        if 'drop_bin' in mutate and b0 <= mutate['drop_bin'] < b1:
            keep[mutate['drop_bin'] - b0] = False
        nv = n.v
        pos = nv > 0
        inv = (1.0 / mu).where(pos, 0.0)
        nlog = (n * mu.log()).where(pos, 0.0)
        term = nlog - mu - T.of(gammaln(nv + 1))
        acc_ll.add(term[keep])
        fw = n * inv - 1.0
        g = [dmu[q] * fw for q in range(F)]
        acc_g.add(T(np.array([x.v[keep] for x in g]), np.array([x.a[keep] for x in g])))
    v, a = acc_ll.result()
    gv, ga = acc_g.result()
    return dict(ll=float(v), ll_cond=float(a), grad=gv, grad_cond=ga)


# ---- the check -------------------------------------------------------------------------------------------------------

def ratio(got, want, cond, floor=1e-300):
    """|got - want| / (2^-52 cond) per entry (0 where both are exactly equal)."""
    got, want, cond = (np.asarray(x, dtype=float) for x in (got, want, cond))
    err = np.abs(got - want)
    with np.errstate(all='ignore'):
        out = np.where(err == 0, 0.0, err / (EPS * cond + floor))
    return np.where(np.isnan(got) | np.isnan(want), np.inf, out)


def check_entries(got, want, cond, C=C_POISSON, what=''):
    """Assert |got - want| <= C 2^-52 cond for every entry; -> the worst ratio |got - want| / (2^-52 cond)."""
    q = ratio(got, want, cond)
    worst = float(q.max(initial=0.0))
    if not worst <= C:
        j = np.unravel_index(int(np.argmax(q)), q.shape) if np.ndim(q) else ()
        raise AssertionError('%s: |err| / (2^-52 cond) = %.3g > C = %d at entry %s (got %r, want %r, cond %.3g)'
                             % (what, worst, C, j, np.asarray(got)[j], np.asarray(want)[j], np.asarray(cond)[j]))
    return worst
