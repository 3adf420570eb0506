"""A numpy Hessian of the likelihood for tests: value, gradient and Hessian over theta = (z [d], rate_scale [S]) of the binned
Poisson and the extended unbinned likelihood, from `oracle.blueice_oracle`'s interpolation on a golden fixture's tensors.

Inside a grid cell the interpolation is multilinear, so its derivatives are exact differences of interpolated values on the
cell's faces: d_i f = (f|z_i=hi - f|z_i=lo) / (hi - lo), d_ij f the mixed face difference, d_ii f = 0.  The cell is the one
the point is assigned to (g[k] <= z < g[k+1], the last one closed), as on the device.  Test infrastructure only."""
import numpy as np

from oracle import blueice_oracle as orc


def cell_of(grid, z):
    """-> (lo, hi) of the cell z is assigned to, or None for a single-anchor axis."""
    g = np.asarray(grid, dtype=float)
    if len(g) < 2:
        return None
    k, _ = orc.find_cell(g, z)
    return g[k], g[k + 1]


def _derivatives(anchor_z, values, z):
    """Interpolated tensor f(z) and its exact first / mixed second derivatives inside the cell of z:
    -> (f, d1 [d] list, d2 {(i, j): array} for i < j)."""
    z = np.asarray(z, dtype=float)
    d = len(anchor_z)
    cells = [cell_of(g, zi) for g, zi in zip(anchor_z, z)]

    def at(**fix):
        zz = z.copy()
        for i, v in fix.items():
            zz[int(i[1:])] = v
        return orc.interpolate(anchor_z, values, zz)

    f = orc.interpolate(anchor_z, values, z)
    d1 = []
    for i in range(d):
        if cells[i] is None:
            d1.append(np.zeros_like(f))
            continue
        lo, hi = cells[i]
        d1.append((at(**{'a%d' % i: hi}) - at(**{'a%d' % i: lo})) / (hi - lo))
    d2 = {}
    for i in range(d):
        for j in range(i + 1, d):
            if cells[i] is None or cells[j] is None:
                d2[(i, j)] = np.zeros_like(f)
                continue
            (li, hi_), (lj, hj) = cells[i], cells[j]
            v = (at(**{'a%d' % i: hi_, 'a%d' % j: hj}) - at(**{'a%d' % i: hi_, 'a%d' % j: lj})
                 - at(**{'a%d' % i: li, 'a%d' % j: hj}) + at(**{'a%d' % i: li, 'a%d' % j: lj}))
            d2[(i, j)] = v / ((hi_ - li) * (hj - lj))
    return f, d1, d2


def _mu_derivatives(model, z, rs):
    """Per-bin expectation terms: rows t_s = rs_s u_s P_s and the first / second derivatives of mu_b = sum_s t_s over theta.
    -> (mu [B], dmu [F, B], d2mu [F, F, B], rate terms r [S], dr [F, S], d2r [F, F, S])."""
    anchor_z = model['anchor_z']
    d = len(anchor_z)
    rs = np.asarray(rs, dtype=float)
    S = len(rs)
    u, du, d2u = _derivatives(anchor_z, model['mus'], z)                 # [S]
    ps, dp, d2p = _derivatives(anchor_z, model['ps'], z)                 # [S, *bins]
    ps = ps.reshape(S, -1)
    dp = [x.reshape(S, -1) for x in dp]
    d2p = {k: x.reshape(S, -1) for k, x in d2p.items()}
    F = d + S
    B = ps.shape[1]
    # theta derivatives of the per-source rate r_s = rs_s u_s and of the per-source row q_s = r_s P_s
    r = rs * u
    dr = np.zeros((F, S))
    d2r = np.zeros((F, F, S))
    for i in range(d):
        dr[i] = rs * du[i]
        for j in range(i + 1, d):
            d2r[i, j] = d2r[j, i] = rs * d2u[(i, j)]
        for t in range(S):
            d2r[i, d + t, t] = d2r[d + t, i, t] = du[i][t]
    for t in range(S):
        dr[d + t, t] = u[t]
    dP = np.zeros((F, S, B))
    d2P = np.zeros((F, F, S, B))
    for i in range(d):
        dP[i] = dp[i]
        for j in range(i + 1, d):
            d2P[i, j] = d2P[j, i] = d2p[(i, j)]
    mu = r @ ps
    dmu = np.einsum('fs,sb->fb', dr, ps) + np.einsum('s,fsb->fb', r, dP)
    d2mu = (np.einsum('fgs,sb->fgb', d2r, ps) + np.einsum('fs,gsb->fgb', dr, dP) + np.einsum('gs,fsb->fgb', dr, dP)
            + np.einsum('s,fgsb->fgb', r, d2P))
    return mu, dmu, d2mu, r, dr, d2r


def hessian_binned(model, counts, z, rs):
    """-> (ll, grad [d + S], H [d + S, d + S]) of the binned Poisson likelihood (no Beeston-Barlow)."""
    ll = orc.loglikelihood(model, counts, z, rs)
    mu, dmu, d2mu, _, _, _ = _mu_derivatives(model, z, rs)
    n = np.asarray(counts, dtype=float).ravel()
    with np.errstate(all='ignore'):
        inv = np.where(n > 0, 1.0 / mu, 0.0)
    f = n * inv - 1.0
    g = dmu @ f
    a = dmu * inv
    H = np.einsum('fgb,b->fg', d2mu, f) - np.einsum('fb,gb,b->fg', a, a, n)
    return ll, g, H


def hessian_unbinned(model, z, rs, outlier_likelihood=1e-12):
    """-> (ll, grad, H) of the extended unbinned likelihood with finite pdfs; events on the outlier clamp are constants."""
    ll = orc.loglikelihood_unbinned(model, z, rs, outlier_likelihood)
    lam, dlam, d2lam, r, dr, d2r = _mu_derivatives(model, z, rs)
    live = lam > 0 if outlier_likelihood != 0 else np.ones(len(lam), bool)
    with np.errstate(all='ignore'):
        inv = np.where(live, 1.0 / lam, 0.0)
    g = -dr.sum(axis=1) + dlam @ inv
    a = dlam * inv
    H = -d2r.sum(axis=2) + np.einsum('fgb,b->fg', d2lam, inv) - a @ a.T
    return ll, g, H


def second_differences(f, x, lo, hi, h):
    """Central second differences of f at x [F] with per-coordinate steps h [F] (Richardson-extrapolated from h and h/2),
    every displaced point inside [lo, hi] (the caller keeps x at least 2 h[i] away from the edges)."""
    x = np.asarray(x, dtype=float)
    F = len(x)

    def once(hh):
        H = np.zeros((F, F))
        f0 = f(x)
        for i in range(F):
            if hh[i] == 0:
                continue
            e = np.zeros(F)
            e[i] = hh[i]
            H[i, i] = (f(x + e) - 2 * f0 + f(x - e)) / hh[i] ** 2
            for j in range(i):
                if hh[j] == 0:
                    continue
                ej = np.zeros(F)
                ej[j] = hh[j]
                H[i, j] = H[j, i] = (f(x + e + ej) - f(x + e - ej) - f(x - e + ej) + f(x - e - ej)) / (4 * hh[i] * hh[j])
        return H

    h = np.asarray(h, dtype=float)
    return (4 * once(h / 2) - once(h)) / 3
