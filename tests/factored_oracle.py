"""The NumPy specification of the source-wise (factored) binned model, for tests: value and gradient over theta = (z [d],
rate_scale [S]) with `derivative_oracle`'s running-error weights, so that

    |device - oracle| <= C_POISSON * 2**-52 * cond        (derivative_oracle.check_entries)

means here what it means everywhere else.

A model is a dict
    anchor_z   d ascending arrays
    own        per source the ascending tuple of the axes it owns (possibly empty; every owned axis has >= 2 anchors)
    ps         per source an array [n_{own[0]}, ..., n_{own[-1]}, B] of template rows (C order over its own axes)
    mus        per source an array [n_{own[0]}, ..., n_{own[-1]}] of rates

Evaluation, as include/blueice_hip.h states it: per source the multilinear interpolation over ITS axes only, tau_s,b =
sum_c w_c p_s,c,b and M_s = sum_c w_c M_s,c; r_s = M_s rs_s; mu_b = sum_s r_s tau_s,b; ll = sum_b n log mu - mu - lgamma(n + 1),
bins with n = 0 contributing -mu.  Every derivative of mu_b is one more coefficient per (source, corner) row: the rows of all
sources side by side and the columns [1 + d + S, rows] go through `tmatmul` and `Acc` exactly as the grid model's do in
`derivative_oracle.derivatives`.

`expand(model)` is the same likelihood on the full tensor-product grid (interpolating a source over an axis it does not own
returns its value unchanged: the weights along that axis sum to one), in the form `derivative_oracle.derivatives` takes.

Imports only `derivative_oracle`, numpy and scipy.special.  Test infrastructure only."""
import numpy as np
from scipy.special import gammaln

from derivative_oracle import Acc, BLOCK, Cell, T, interp_derivs, tmatmul


def n_bins(model):
    return int(np.shape(model['ps'][0])[-1])


def expand(model):
    """-> {'anchor_z', 'ps' [n_0, .., n_{d-1}, S, B], 'mus' [n_0, .., n_{d-1}, S]} of the full grid"""
    anchor_z = [np.asarray(g, dtype=float) for g in model['anchor_z']]
    shape = tuple(len(g) for g in anchor_z)
    S, B = len(model['own']), n_bins(model)
    ps = np.empty(shape + (S, B))
    mus = np.empty(shape + (S,))
    for idx in np.ndindex(*shape):
        for s, own in enumerate(model['own']):
            sub = tuple(idx[i] for i in own)
            ps[idx + (s,)] = np.asarray(model['ps'][s], dtype=float)[sub]
            mus[idx + (s,)] = np.asarray(model['mus'][s], dtype=float)[sub]
    return dict(anchor_z=anchor_z, ps=ps, mus=mus)


def _zero():
    return T.of(0.0)


def factored_columns(model, z, rs):
    """-> (coef T [1 + d + S, NR], rows index list [(source, own anchor index tuple)]) : column 0 mu, columns 1 .. d the shape
    axes, then the rate scales; row order: sources ascending, the source's corners in its Cell's order."""
    d, S = len(model['anchor_z']), len(model['own'])
    z = np.asarray(z, dtype=float)
    rs = np.asarray(rs, dtype=float)
    cols, rows = [], []
    for s, own in enumerate(model['own']):
        cell = Cell([np.asarray(model['anchor_z'][i], dtype=float) for i in own], z[list(own)] if len(own) else np.zeros(0))
        u, du, _ = interp_derivs(cell, np.asarray(model['mus'][s], dtype=float))          # M_s(z) and its slopes over the own axes
        R = T.of(rs[s])
        r = u * R
        for c in range(cell.nc):
            w = cell.w[c]
            col = [_zero() for _ in range(1 + d + S)]
            col[0] = w * r
            for j, i in enumerate(own):
                col[1 + i] = cell.dw[c][j] * r + w * (du[j] * R)
            col[1 + d + s] = w * u
            cols.append(col)
            rows.append((s, cell.index[c]))
    K = 1 + d + S
    coef = T(np.array([[float(cols[k][j].v) for k in range(len(cols))] for j in range(K)]),
             np.array([[float(cols[k][j].a) for k in range(len(cols))] for j in range(K)]))
    return coef, rows


def factored_derivatives(model, z, rs, counts):
    """-> dict(ll, grad [d + S], ll_cond, grad_cond) of the source-wise model at (z, rs) against counts [B]"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    coef, rows = factored_columns(model, z, rs)
    B = n_bins(model)
    n_all = np.asarray(counts, dtype=float).ravel()
    acc_ll, acc_g = Acc(()), Acc((F,))
    for b0 in range(0, B, BLOCK):
        b1 = min(B, b0 + BLOCK)
        block = np.array([np.asarray(model['ps'][s], dtype=float)[idx][b0:b1] for s, idx in rows])
        X = tmatmul(coef, T(block))
        mu = X[0]
        n = n_all[b0:b1]
        pos = n > 0
        with np.errstate(all='ignore'):
            inv = (1.0 / mu).where(pos, 0.0)
            nlog = (T.of(n) * mu.log()).where(pos, 0.0)
        acc_ll.add(nlog - mu - T.of(gammaln(n + 1)))
        fw = T.of(n) * inv - 1.0
        acc_g.add(X[1:1 + F] * T(fw.v[None], fw.a[None]))
    v, a = acc_ll.result()
    gv, ga = acc_g.result()
    return dict(ll=float(v), ll_cond=float(a), grad=gv, grad_cond=ga)


# ---- random models of the tests ---------------------------------------------------------------------------------------

def random_model(rng, n_anchor, own, B, zero_quarter=()):
    """Anchors at unevenly spaced z, templates normalised over the bins, rates of a few hundred events; the sources listed in
    `zero_quarter` have a quarter of their bins zero at every anchor (the same bins: their tau is exactly 0 there)."""
    anchor_z = [np.sort(rng.uniform(-2.0, 2.0, n)) if n > 1 else np.zeros(1) for n in n_anchor]
    ps, mus = [], []
    for s, o in enumerate(own):
        shape = tuple(n_anchor[i] for i in o)
        p = rng.gamma(2.0, 1.0, size=shape + (B,))
        if s in zero_quarter:
            p[..., rng.permutation(B)[:max(1, B // 4)]] = 0.0
        p /= p.sum(axis=-1, keepdims=True)
        ps.append(p)
        mus.append(rng.uniform(150.0, 600.0, size=shape))
    return dict(anchor_z=anchor_z, own=[tuple(o) for o in own], ps=ps, mus=mus)


def expectation(model, z, rs):
    """mu [B] at (z, rs), plain float64 (for drawing counts)"""
    coef, rows = factored_columns(model, z, rs)
    block = np.array([np.asarray(model['ps'][s], dtype=float)[idx] for s, idx in rows])
    return coef.v[0] @ block
