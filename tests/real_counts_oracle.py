"""Oracle of bi_eval_real: the half-deviance of real-valued counts n_b >= 0 against the expectation at (z, rate_scale), its
gradient over theta = (z [d], rate_scale [S]) and, for every gradient entry, its own condition
    half_deviance   sum_b  (mu_b - n_b) - n_b log(mu_b / n_b)        (n_b = 0: mu_b)
    grad_q          sum_b  d_q mu_b (1 - n_b / mu_b)                 (n_b = 0: d_q mu_b)
    grad_cond_q     sum_b  |d_q mu_b| |1 - n_b / mu_b|
in plain numpy: the value from `gof_oracle.statistics`, whose per-bin half-deviance holds for any real n, the morph
derivatives d_q mu_b from `derivative_oracle`'s coefficient columns (on an anchor: the cell the point is assigned to).  Sums
over bins are math.fsum.  Test infrastructure only: nothing in the package imports it."""
import math

import numpy as np

import derivative_oracle as dor
import gof_oracle
from oracle import blueice_oracle as orc

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL = gof_oracle.ST_OUT_OF_BOUNDS, gof_oracle.ST_UNPHYSICAL


def screen(model, z, rate_scale, allow_negative=None):
    """The reference's early exits (as `gof_oracle.point`) -> 0 or the status bit"""
    z = np.asarray(z, dtype=float)
    if not orc.in_bounds(model['anchor_z'], z):
        return ST_OUT_OF_BOUNDS
    rates = orc.rates_at(model, z, rate_scale)
    if allow_negative is None or not any(allow_negative):
        physical = bool(np.all((rates >= 0) & (rates < np.inf)))
    else:
        physical = bool(any(rates < np.inf)) and not np.sum(rates) < 0 and all((0 <= r) or a for r, a in zip(rates, allow_negative))
    return 0 if physical else ST_UNPHYSICAL


def expectation_derivatives(model, z, rate_scale):
    """-> d mu [d + S, B]: the first derivatives of the per-bin expectation (axes, then rate scales), no screening"""
    rs = np.asarray(rate_scale, dtype=float)
    cell = dor.Cell(model['anchor_z'], z)
    coef, _, _, _ = dor.coefficient_columns(cell, model['mus'], rs, second=False)
    rows = dor._rows(model, cell, 0, dor.n_bins(model), len(rs))
    return (coef.v @ rows)[1:]


def point(model, counts, z, rate_scale, allow_negative=None):
    """What bi_eval_real returns for one (point, dataset) -> dict(half_deviance, grad [d + S], grad_cond [d + S], status, mu [B]).
    Outside the box / unphysical rates: +inf with the status bit; a negative or nan expectation: nan; n > 0 where mu = 0:
    +inf; the gradient is nan wherever the value is not finite."""
    z, rs = np.asarray(z, dtype=float), np.asarray(rate_scale, dtype=float)
    F = len(z) + len(rs)
    nan_grad = np.full(F, np.nan)
    st = screen(model, z, rs, allow_negative)
    if st:
        return dict(half_deviance=np.inf, grad=nan_grad, grad_cond=nan_grad, status=st, mu=None)
    n = np.asarray(counts, dtype=float).ravel()
    s = gof_oracle.statistics(model, n, z, rs)
    mu = np.asarray(s['mu'], dtype=float)
    if np.any(~(mu >= 0)):
        return dict(half_deviance=np.nan, grad=nan_grad, grad_cond=nan_grad, status=0, mu=mu)
    if np.any((n > 0) & (mu == 0)):
        return dict(half_deviance=np.inf, grad=nan_grad, grad_cond=nan_grad, status=0, mu=mu)
    half = math.fsum(np.asarray(s['half_terms'], dtype=float).tolist())
    if not np.isfinite(half):
        return dict(half_deviance=half, grad=nan_grad, grad_cond=nan_grad, status=0, mu=mu)
    dmu = expectation_derivatives(model, z, rs)
    hit = n > 0
    with np.errstate(all='ignore'):
        f = np.where(hit, 1.0 - n / np.where(hit, mu, 1.0), 1.0)
    grad = np.array([math.fsum((row * f).tolist()) for row in dmu])
    cond = np.array([math.fsum((np.abs(row) * np.abs(f)).tolist()) for row in dmu])
    return dict(half_deviance=half, grad=grad, grad_cond=cond, status=0, mu=mu)


def expectation(model, z, rate_scale):
    """mu [B] at the point, no screening (the Asimov dataset of that truth)"""
    B = dor.n_bins(model)
    return np.asarray(gof_oracle.statistics(model, np.zeros(B), z, rate_scale)['mu'], dtype=float)
