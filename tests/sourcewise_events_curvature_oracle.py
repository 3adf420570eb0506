"""The NumPy specification of the second-order layer of the extended unbinned likelihood of a source-wise model, for tests:
value, gradient and Hessian over theta = (z [d], rate_scale [S]) with `derivative_oracle`'s running-error weights, as
`factored_curvature_oracle.curvature` is for binned data and `sourcewise_events_oracle.events_derivatives` for the first order.

A model is `sourcewise_events_oracle`'s: ps[s] [n_{own[0]}, .., N] holds the pdf value of every event at every own anchor of
source s (finite or nan).  With lam_e = sum_s r_s tau_s,e (nan sources left out per event, the outlier clamp on lam_e)

    ll                    = sum_e log lam_e - sum_s r_s
    d ll / d theta_q      = sum_e (1 / lam_e) d_q lam_e - d_q sum_s r_s
    d2 ll / d theta_q d theta_r = sum_e [(1 / lam_e) d_qr lam_e - (d_q lam_e / lam_e) (d_r lam_e / lam_e)] - d_qr sum_s r_s

lam_e and its derivatives are `factored_curvature_oracle.curvature_columns`' coefficient columns times the event rows; a clamped
event contributes log(outlier) and nothing else; sum_s r_s and its derivatives come from the interpolated rates alone
(`interp_derivs`: a pdf integrates to one exactly), and have the second derivatives d_j M_s (z_i, rs_s) and rs_s d_jk M_s
(z_i, z_k) and no others.  No 1 / lam^2 is formed.  With outlier = 0 an event with lam_e = 0 gives ll = -inf and nan derivatives.

Imports only `derivative_oracle`, `factored_oracle`, `factored_curvature_oracle` and numpy, and changes none of them.
Test infrastructure only."""
import math

import numpy as np

import factored_curvature_oracle as fc
import factored_oracle as fo
from derivative_oracle import Acc, BLOCK, Cell, T, interp_derivs, pairs, tmatmul


def rate_curvature(model, z, rs):
    """-> (sum_s r_s as T, its first derivatives [F] as T, its second derivatives over pairs(F) as T)"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    P2 = pairs(F)
    where = {qr: j for j, qr in enumerate(P2)}
    z = np.asarray(z, dtype=float)
    rs = np.asarray(rs, dtype=float)
    total = T.of(0.0)
    dv, da = np.zeros(F), np.zeros(F)
    hv, ha = np.zeros(len(P2)), np.zeros(len(P2))
    for s, own in enumerate(model['own']):
        cell = Cell([np.asarray(model['anchor_z'][i], dtype=float) for i in own], z[list(own)] if len(own) else np.zeros(0))
        u, du, d2u = interp_derivs(cell, np.asarray(model['mus'][s], dtype=float))
        R = T.of(rs[s])
        total = total + u * R
        dv[d + s] += float(u.v)
        da[d + s] += float(u.a)
        for j, i in enumerate(own):
            t = du[j] * R
            dv[i] += float(t.v)
            da[i] += float(t.a)
            hv[where[(i, d + s)]] += float(du[j].v)
            ha[where[(i, d + s)]] += float(du[j].a)
            for jj in range(j + 1, len(own)):
                t2 = d2u[(j, jj)] * R
                hv[where[(i, own[jj])]] += float(t2.v)
                ha[where[(i, own[jj])]] += float(t2.a)
    return total, T(dv, da), T(hv, ha)


def events_curvature(model, z, rs, outlier=1e-12, n_events=None):
    """-> dict(ll, grad [F], hess [F, F], ll_cond, grad_cond, hess_cond, n_clamped) of the source-wise model at (z, rs) over its
    first n_events events (None: all)"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    P2 = pairs(F)
    qi, ri = np.array([q for q, _ in P2]), np.array([p for _, p in P2])
    coef, rows = fc.curvature_columns(model, z, rs)
    N = fo.n_bins(model) if n_events is None else int(n_events)
    src = np.array([s for s, _ in rows])
    acc_ll, acc_g, acc_h = Acc(()), Acc((F,)), Acc((len(P2),))
    n_clamped = 0
    minus_inf = False
    for b0 in range(0, N, BLOCK):
        b1 = min(N, b0 + BLOCK)
        block = np.array([np.asarray(model['ps'][s], dtype=float)[idx][b0:b1] for s, idx in rows])
        for s in range(S):                      # nan pdf terms are dropped per (event, source)
            mine = np.flatnonzero(src == s)
            bad = np.isnan(block[mine]).any(axis=0)
            block[np.ix_(mine, np.flatnonzero(bad))] = 0.0
        X = tmatmul(coef, T(block))
        lam = X[0]
        if outlier != 0:
            live = lam.v > 0
            n_clamped += int((~live).sum())
            X = X[:, live]
            lam = X[0]
        elif np.any(lam.v == 0):
            minus_inf = True
            break
        acc_ll.add(lam.log())
        inv = 1.0 / lam
        invb = T(inv.v[None], inv.a[None])
        dlam = X[1:1 + F]
        acc_g.add(dlam * invb)
        sl = dlam * invb                        # (d_q lam / lam) (d_r lam / lam): no 1 / lam^2 (derivative_oracle.derivatives)
        acc_h.add(X[1 + F:] * invb - sl[qi] * sl[ri])
    if minus_inf:
        return dict(ll=-np.inf, ll_cond=0.0, grad=np.full(F, np.nan), grad_cond=np.zeros(F), hess=np.full((F, F), np.nan),
                    hess_cond=np.zeros((F, F)), n_clamped=0)
    total, dtotal, d2total = rate_curvature(model, z, rs)
    acc_ll.add_scalar(-total)
    if n_clamped:
        acc_ll.add_scalar(T(np.array(n_clamped * math.log(outlier)), np.array(abs(n_clamped * math.log(outlier)))))
    acc_g.add_scalar(-dtotal)
    acc_h.add_scalar(-d2total)
    v, a = acc_ll.result()
    gv, ga = acc_g.result()
    hv, ha = acc_h.result()
    H, Hc = np.zeros((F, F)), np.zeros((F, F))
    for j, (q, p) in enumerate(P2):
        H[q, p] = H[p, q] = hv[j]
        Hc[q, p] = Hc[p, q] = ha[j]
    return dict(ll=float(v), ll_cond=float(a), grad=gv, grad_cond=ga, hess=H, hess_cond=Hc, n_clamped=n_clamped)
