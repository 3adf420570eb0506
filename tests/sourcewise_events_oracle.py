"""The NumPy specification of the extended unbinned likelihood of a source-wise model, for tests: value and gradient over
theta = (z [d], rate_scale [S]) with `derivative_oracle`'s running-error weights, as `factored_oracle` is for binned data.

A model is `factored_oracle`'s dict with the EVENTS where the bins are: ps[s] [n_{own[0]}, .., N] holds the pdf value of every
event at every own anchor of source s (finite or nan).  As include/blueice_hip.h states it:

    tau_s,e = sum_c w_c p_s,c,e                 a source with a nan at any of its corners leaves the event (numpy.nansum)
    lam_e   = sum_s r_s tau_s,e                 r_s = M_s(z) rs_s
    clamped = outlier != 0 and not (lam_e > 0)  ->  the event contributes log(outlier), a constant
    ll      = sum_e log lam_e - sum_s r_s
    d ll / d theta_j = sum_e (1 / lam_e) d_j lam_e - d_j sum_s r_s

lam_e and d_j lam_e are `factored_oracle.factored_columns`' coefficient columns times the rows, as in the binned specification;
sum_s r_s and its derivatives come from the interpolated rates alone (a pdf integrates to one exactly: no column of ones is
interpolated).  With outlier = 0 an event with lam_e = 0 gives ll = -inf and a nan gradient.

`golden_model(f)` / `golden_point(kw)`: the per-source tensors and the calls of tests/golden/api_source_wise.npz in this form.

Imports only `derivative_oracle`, `factored_oracle` and numpy.  Test infrastructure only."""
import math

import numpy as np

import factored_oracle as fo
from derivative_oracle import Acc, BLOCK, Cell, T, interp_derivs, tmatmul


def rate_terms(model, z, rs):
    """-> (sum_s r_s as T, its derivatives [d + S] as T)"""
    d, S = len(model['anchor_z']), len(model['own'])
    z = np.asarray(z, dtype=float)
    rs = np.asarray(rs, dtype=float)
    total = T.of(0.0)
    dv, da = np.zeros(d + S), np.zeros(d + S)
    for s, own in enumerate(model['own']):
        cell = Cell([np.asarray(model['anchor_z'][i], dtype=float) for i in own], z[list(own)] if len(own) else np.zeros(0))
        u, du, _ = interp_derivs(cell, np.asarray(model['mus'][s], dtype=float))
        R = T.of(rs[s])
        total = total + u * R
        for j, i in enumerate(own):
            t = du[j] * R
            dv[i] += float(t.v)
            da[i] += float(t.a)
        dv[d + s] += float(u.v)
        da[d + s] += float(u.a)
    return total, T(dv, da)


def events_derivatives(model, z, rs, outlier=1e-12, n_events=None):
    """-> dict(ll, grad [d + S], ll_cond, grad_cond, n_clamped) of the source-wise model at (z, rs) over its first n_events
    events (None: all)"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    coef, rows = fo.factored_columns(model, z, rs)
    N = fo.n_bins(model) if n_events is None else int(n_events)
    src = np.array([s for s, _ in rows])
    acc_ll, acc_g = Acc(()), Acc((F,))
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
        acc_g.add(X[1:1 + F] * T(inv.v[None], inv.a[None]))
    if minus_inf:
        return dict(ll=-np.inf, ll_cond=0.0, grad=np.full(F, np.nan), grad_cond=np.zeros(F), n_clamped=0)
    total, dtotal = rate_terms(model, z, rs)
    acc_ll.add_scalar(-total)
    if n_clamped:
        acc_ll.add_scalar(T(np.array(n_clamped * math.log(outlier)), np.array(abs(n_clamped * math.log(outlier)))))
    acc_g.add_scalar(-dtotal)
    v, a = acc_ll.result()
    gv, ga = acc_g.result()
    return dict(ll=float(v), ll_cond=float(a), grad=gv, grad_cond=ga, n_clamped=n_clamped)


def plain_ll(model, z, rs, outlier=1e-12):
    """The same value with a plain NumPy interpolation per source, float64: what the reference's per-source interpolators compute"""
    z = np.asarray(z, dtype=float)
    terms, total = [], 0.0
    for s, own in enumerate(model['own']):
        p = np.asarray(model['ps'][s], dtype=float)
        m = np.asarray(model['mus'][s], dtype=float)
        for i in own:                           # one axis after the other, the first own axis first
            g = np.asarray(model['anchor_z'][i], dtype=float)
            k = len(g) - 2 if z[i] == g[-1] else min(max(int(np.searchsorted(g, z[i], side='right')) - 1, 0), len(g) - 2)
            t = (z[i] - g[k]) / (g[k + 1] - g[k])
            p = p[k] * (1 - t) + p[k + 1] * t
            m = m[k] * (1 - t) + m[k + 1] * t
        r = float(m) * float(rs[s])
        terms.append(r * p)
        total += r
    lam = np.nansum(np.array(terms), axis=0)
    if outlier != 0:
        lam = np.where(lam > 0, lam, outlier)
    with np.errstate(divide='ignore'):
        return float(np.sum(np.log(lam)) - total)


# ---- the reference's recorded case -----------------------------------------------------------------------------------

GOLDEN_SOURCES = ('a', 'b', 'c')
GOLDEN_DEFAULTS = dict(mu=0.0, sigma=1.0)


def golden_model(f):
    """tests/golden/api_source_wise.npz (np.load) -> the model: d = 2 (mu, sigma), own axes (0,), (1,), ()"""
    anchor_z = [None, None]
    own, ps, mus = [], [], []
    for i in range(3):
        dims = tuple(int(k) for k in f['sw_%d_dims' % i])
        for pos, k in enumerate(dims):
            anchor_z[k] = np.asarray(f['sw_%d_z_%d' % (i, pos)], dtype=float)
        own.append(dims)
        ps.append(np.asarray(f['sw_%d_ps' % i], dtype=float))
        mus.append(np.asarray(f['sw_%d_mus' % i], dtype=float))
    return dict(anchor_z=anchor_z, own=own, ps=ps, mus=mus)


def golden_point(kw):
    """a call of model_zoo.api_source_wise -> (z [2], rs [3])"""
    z = np.array([kw.get('mu', GOLDEN_DEFAULTS['mu']), kw.get('sigma', GOLDEN_DEFAULTS['sigma'])], dtype=float)
    rs = np.array([kw.get(n + '_rate_multiplier', 1.0) for n in GOLDEN_SOURCES], dtype=float)
    return z, rs


def carrier(model):
    """the same geometry and rates with one-bin rows [1.0]: what a context needs before pdf values scored elsewhere are uploaded"""
    return dict(anchor_z=model['anchor_z'], own=model['own'], mus=model['mus'],
                ps=[np.ones(np.shape(m) + (1,)) for m in model['mus']])


def upload_events(ctx, model, n_events, outlier=1e-12):
    """the rows of `model` (ps[s] [.., sum(n_events)], set after set) through SourceWiseContext.set_event_rows"""
    N = int(np.sum(n_events))
    flat = [np.asarray(p, dtype=float).reshape(np.asarray(m).size, N) for p, m in zip(model['ps'], model['mus'])]
    ctx.set_event_rows(n_events, lambda s, local: flat[s][local], outlier)
