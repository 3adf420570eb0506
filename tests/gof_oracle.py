"""Goodness-of-fit oracle: the per-bin expectation, half-deviance and Pearson chi2 of a binned likelihood in numpy, built on
the CPU oracle's morph (oracle/blueice_oracle.py: `interpolate`, `rates_at`) and written in the direct per-bin forms
    half-deviance   n > 0: mu - n - n log(mu / n)     n = 0: mu
    Pearson         n > 0: (n - mu)^2 / mu            n = 0: mu
(n = 0 and mu = 0: 0 in both; n > 0 and mu = 0: +inf in both).  Test infrastructure only: nothing in the package imports it."""
import numpy as np

from oracle import blueice_oracle as orc

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL = 1, 2


def per_bin(n, mu):
    """-> (half-deviance terms, Pearson terms) of counts n and expectations mu (arrays of one shape and dtype)"""
    n, mu = np.broadcast_arrays(np.asarray(n), np.asarray(mu))
    hit = n > 0
    with np.errstate(all='ignore'):
        ratio = np.where(hit, mu / np.where(hit, n, 1), 1)
        half = np.where(hit, mu - n - n * np.log(ratio), mu)
        pearson = np.where(hit, (n - mu) ** 2 / np.where(hit & (mu == 0), 1, mu), mu)
        pearson = np.where(hit & (mu == 0), np.inf, pearson)
    return half, pearson


def statistics(model, counts, z, rate_scale, dtype=float):
    """-> dict(mu_sources [S, B], mu [B], half_terms [B], pearson_terms [B], half_deviance, pearson) of one dataset `counts`
    at the point (z, rate_scale), no screening.  dtype=numpy.longdouble evaluates templates, sums and logarithms in extended
    precision (the corner weights stay the float64 ones every implementation starts from)."""
    z = np.asarray(z, dtype=float)
    wide = dict(model, ps=np.asarray(model['ps'], dtype=dtype), mus=np.asarray(model['mus'], dtype=dtype))
    rates = orc.rates_at(wide, z, rate_scale)
    ps = orc.interpolate(model['anchor_z'], wide['ps'], z).reshape(len(rates), -1)
    mu_sources = ps * rates[:, None]
    mu = np.zeros(ps.shape[1], dtype=dtype)
    for row in mu_sources:                       # source by source, as the reference adds them up
        mu = mu + row
    n = np.asarray(counts, dtype=dtype).ravel()
    half, pearson = per_bin(n, mu)
    return dict(mu_sources=mu_sources, mu=mu, half_terms=half, pearson_terms=pearson, half_deviance=half.sum(), pearson=pearson.sum())


def point(model, counts, z, rate_scale, allow_negative=None, dtype=float):
    """What bi_eval_gof returns for one (point, dataset): (half-deviance, Pearson, status).  The reference's early exits
    (outside the anchor box; unphysical rates: blueice/likelihood.py:345-347,397-415) give +inf in both with their status bit;
    a live point gives +inf in both where the likelihood is -inf and nan in both where it is nan."""
    z = np.asarray(z, dtype=float)
    if not orc.in_bounds(model['anchor_z'], z):
        return np.inf, np.inf, ST_OUT_OF_BOUNDS
    rates = orc.rates_at(model, z, rate_scale)
    if allow_negative is None or not any(allow_negative):
        physical = bool(np.all((rates >= 0) & (rates < np.inf)))
    else:
        physical = bool(any(rates < np.inf)) and not np.sum(rates) < 0 and \
            all((0 <= r) or a for r, a in zip(rates, allow_negative))
    if not physical:
        return np.inf, np.inf, ST_UNPHYSICAL
    s = statistics(model, counts, z, rate_scale, dtype)
    with np.errstate(all='ignore'):
        ll = np.sum(orc.poisson_logpmf(np.asarray(counts, dtype=float).ravel(), np.asarray(s['mu'], dtype=float)))
    if np.isnan(ll):
        return np.nan, np.nan, 0
    if ll == -np.inf:
        return np.inf, np.inf, 0
    return s['half_deviance'], s['pearson'], 0


def tensors_of(lf):
    """The anchor tensors of a prepared blueice_amd binned likelihood, as the oracle's model dict (bins flattened)."""
    S = len(lf.source_name_list)
    if not len(lf.shape_parameters):
        return dict(anchor_z=[], ps=np.asarray(lf.base_model.pmf_grids()[0], dtype=float).reshape(S, -1),
                    mus=np.asarray(lf.base_model.expected_events(), dtype=float), n_model=None)
    grid_shape = tuple(lf.morpher.grid_shape)
    ps, mus = None, np.empty(grid_shape + (S,))
    for _, multi, zs in lf.morpher.anchor_items():
        rows = np.asarray(lf.anchor_models[zs].pmf_grids()[0], dtype=float).reshape(S, -1)
        if ps is None:
            ps = np.empty(grid_shape + rows.shape)
        ps[multi] = rows
        mus[multi] = lf.anchor_models[zs].expected_events()
    return dict(anchor_z=[np.asarray(g, dtype=float) for g in lf.morpher.anchor_z_arrays], ps=ps, mus=mus, n_model=None)
