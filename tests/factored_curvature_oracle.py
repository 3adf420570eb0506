"""The NumPy specification of the second-order layers of a source-wise (factored) binned model, for tests: value, gradient and
Hessian over theta = (z [d], rate_scale [S]) with `derivative_oracle`'s running-error weights (T, Acc, tmatmul, as
`factored_oracle.factored_derivatives` forms the gradient), so that

    |device - oracle| <= C_POISSON * 2**-52 * cond        (derivative_oracle.check_entries)

means here what it means everywhere else; and the expected (Fisher) information, its per-entry cond, the unbounded counts
and the total expectation in `fisher_oracle._sums`' form, so that `fisher_oracle.check` applies.

Source s is multilinear over its own axes O_s, so every derivative of mu_b = sum_s M_s(z) rs_s tau_s,b is one more coefficient
per (source, corner) row over the same rows (w, dw, d2w: the corner weight and its derivatives over the own axes; u, du, d2u:
M_s and its):
    mu                      w u rs
    d / d z_i               (dw_j u + w du_j) rs                                                    i = O_s[j]
    d / d rs_s              w u
    d2 / d z_i d z_k        (d2w_jk u + dw_j du_k + dw_k du_j + w d2u_jk) rs                         j < k
    d2 / d z_i d z_i        2 dw_j du_j rs                                                           (d_jj w = d_jj u = 0)
    d2 / d z_i d rs_s       dw_j u + w du_j
    d2 / d rs d rs          0
and H = sum_b d2 mu_b f_b - n_b (d_q mu_b / mu_b) (d_r mu_b / mu_b), f_b = n_b / mu_b - 1 (bins with n = 0 have no 1 / mu), exactly as
`derivative_oracle.derivatives` forms it for the grid model.  An axis nobody owns has zero rows and columns.

Imports only `derivative_oracle`, `factored_oracle`, `fisher_oracle`, numpy and scipy.special, and changes none of them.
Test infrastructure only."""
import numpy as np
from scipy.special import gammaln

import factored_oracle as fo
import fisher_oracle
from derivative_oracle import Acc, BLOCK, Cell, T, interp_derivs, pairs, tmatmul


def curvature_columns(model, z, rs, second=True):
    """-> (coef T [1 + F (+ len(pairs(F)))], NR], rows [(source, own anchor index tuple)]): column 0 mu, columns 1 .. F the
    first derivatives (axes, then rate scales), then the pairs q <= r of `pairs(F)`"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    P2 = pairs(F) if second else []
    where = {qr: 1 + F + j for j, qr in enumerate(P2)}
    z = np.asarray(z, dtype=float)
    rs = np.asarray(rs, dtype=float)
    cols, rows = [], []
    for s, own in enumerate(model['own']):
        cell = Cell([np.asarray(model['anchor_z'][i], dtype=float) for i in own], z[list(own)] if len(own) else np.zeros(0))
        u, du, d2u = interp_derivs(cell, np.asarray(model['mus'][s], dtype=float))
        R = T.of(rs[s])
        r = u * R
        for c in range(cell.nc):
            w, dw, d2w = cell.w[c], cell.dw[c], cell.d2w[c]
            col = [T.of(0.0) for _ in range(1 + F + len(P2))]
            col[0] = w * r
            col[1 + d + s] = w * u
            for j, i in enumerate(own):
                col[1 + i] = dw[j] * r + w * (du[j] * R)
                if not second:
                    continue
                col[where[(i, i)]] = (dw[j] * (du[j] * R)) * 2.0
                col[where[(i, d + s)]] = dw[j] * u + w * du[j]
                for jj in range(j + 1, len(own)):
                    k = own[jj]
                    col[where[(i, k)]] = d2w[(j, jj)] * r + dw[j] * (du[jj] * R) + dw[jj] * (du[j] * R) + w * (d2u[(j, jj)] * R)
            cols.append(col)
            rows.append((s, cell.index[c]))
    K = len(cols[0])
    coef = T(np.array([[float(cols[k][j].v) for k in range(len(cols))] for j in range(K)]),
             np.array([[float(cols[k][j].a) for k in range(len(cols))] for j in range(K)]))
    return coef, rows


def _block(model, rows, b0, b1):
    return np.array([np.asarray(model['ps'][s], dtype=float)[idx][b0:b1] for s, idx in rows])


def curvature(model, z, rs, counts):
    """-> dict(ll, grad [F], hess [F, F], ll_cond, grad_cond, hess_cond) of the source-wise model at (z, rs) against counts [B]"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    P2 = pairs(F)
    qi, ri = np.array([q for q, _ in P2]), np.array([p for _, p in P2])
    coef, rows = curvature_columns(model, z, rs)
    B = fo.n_bins(model)
    n_all = np.asarray(counts, dtype=float).ravel()
    acc_ll, acc_g, acc_h = Acc(()), Acc((F,)), Acc((len(P2),))
    for b0 in range(0, B, BLOCK):
        b1 = min(B, b0 + BLOCK)
        X = tmatmul(coef, T(_block(model, rows, b0, b1)))
        mu = X[0]
        n = n_all[b0:b1]
        pos = n > 0
        with np.errstate(all='ignore'):
            inv = (1.0 / mu).where(pos, 0.0)
            nlog = (T.of(n) * mu.log()).where(pos, 0.0)
        acc_ll.add(nlog - mu - T.of(gammaln(n + 1)))
        fw = T.of(n) * inv - 1.0
        fwb = T(fw.v[None], fw.a[None])
        dmu = X[1:1 + F]
        acc_g.add(dmu * fwb)
        # (d_q mu / mu) (d_r mu / mu) n: no 1 / mu^2 (derivative_oracle.derivatives)
        sl = dmu * T(inv.v[None], inv.a[None])
        acc_h.add(X[1 + F:] * fwb - sl[qi] * sl[ri] * T.of(n)[None])
    v, a = acc_ll.result()
    gv, ga = acc_g.result()
    hv, ha = acc_h.result()
    H, Hc = np.zeros((F, F)), np.zeros((F, F))
    for j, (q, p) in enumerate(P2):
        H[q, p] = H[p, q] = hv[j]
        Hc[q, p] = Hc[p, q] = ha[j]
    return dict(ll=float(v), ll_cond=float(a), grad=gv, grad_cond=ga, hess=H, hess_cond=Hc)


def _mu_dmu(model, z, rs):
    coef, rows = curvature_columns(model, z, rs, second=False)
    X = coef.v @ _block(model, rows, 0, fo.n_bins(model))
    return X[0], X[1:]


def information(model, z, rs):
    """-> dict(info [F, F], cond [F, F], unbounded [F] int, total, negative), fisher_oracle.information's form"""
    return fisher_oracle._sums(*_mu_dmu(model, z, rs), float)


def information_longdouble(model, z, rs):
    return fisher_oracle._sums(*_mu_dmu(model, z, rs), np.longdouble)


# ---- the fixture of the unbounded counts --------------------------------------------------------------------------------

def unbounded_fixture():
    """-> (model, z, rs, unbounded [6]): d = 3 (anchors 3, 2, 4; nobody owns axis 2), own = ((0,), (0, 1), ()), B = 63.
    Bins 0 .. 6 are zero for source 2 and, for sources 0 and 1, at every anchor of axis 0 but the last; bins 7 .. 10 are filled
    by source 2 only.  At z_0 exactly on anchor 1 of axis 0 (cell 1, t = 0) and rs_2 = 0 the expectation of those eleven bins is
    0; in the first seven it moves with z_0 (towards the last anchor), in the other four with rs_2; with nothing else."""
    rng = np.random.default_rng(77)
    model = fo.random_model(rng, (3, 2, 4), ((0,), (0, 1), ()), 63)
    model['ps'][2][..., :7] = 0.0
    model['ps'][0][:2, :7] = 0.0
    model['ps'][1][:2, :, :7] = 0.0
    model['ps'][0][..., 7:11] = 0.0
    model['ps'][1][..., 7:11] = 0.0
    g = model['anchor_z']
    z = np.array([g[0][1], 0.5 * (g[1][0] + g[1][1]), 0.5 * (g[2][1] + g[2][2])])
    rs = np.array([1.25, 0.75, 0.0])
    return model, z, rs, np.array([7, 0, 0, 0, 0, 4], dtype=np.int64)
