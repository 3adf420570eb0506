"""The NumPy specification of the non-empty-bin form of a source-wise model's likelihood, for tests: value and gradient over
theta = (z [d], rate_scale [S]) with `derivative_oracle`'s running-error weights, as `factored_oracle` is for the dense form.

For the list Z = {b : n_b != 0} of a dataset (ascending bins), as include/blueice_hip.h states it:

    ll        = sum_{b in Z} n_b log mu_b  -  sum_s lambda_s  -  sum_b lgamma(n_b + 1),     lambda_s = r_s sum_c w_c R_{s,c}
    d ll / d theta_j = sum_{b in Z} (n_b / mu_b) d_j mu_b  -  d_j sum_s lambda_s

with R_{s,c} the total of anchor row (s, c) over ALL bins.  mu_b and d_j mu_b are `factored_oracle.factored_columns`'
coefficient columns times the rows, as in the dense specification; sum_s lambda_s and its derivatives are the SAME columns
times the vector of row totals (column 0 is w_c r_s, column j its derivative: the sum over the bins is linear in the rows).  The
identity with the dense form needs mu_b >= 0 everywhere, which the model's limits guarantee: templates >= 0, rates in [0, inf).

A listed bin with mu_b = 0, or a listed count that is negative or no integer, gives ll = -inf and a nan gradient.

Imports only `derivative_oracle`, `factored_oracle`, numpy and scipy.special.  Test infrastructure only."""
import math

import numpy as np
from scipy.special import gammaln

import factored_oracle as fo
from derivative_oracle import Acc, BLOCK, T, tmatmul


def row_totals(model, rows):
    """R [NR] as T: every row's total over all bins, one rounding (math.fsum is exact to it; the library sums in long double)"""
    return T(np.array([math.fsum(np.asarray(model['ps'][s], dtype=float)[idx].tolist()) for s, idx in rows]))


def listed_bins(counts):
    """Z: the bins with n != 0, ascending (nan counts as listed, as the device's is_nz)"""
    n = np.asarray(counts, dtype=float).ravel()
    return np.flatnonzero(n != 0)


def nonempty_derivatives(model, z, rs, counts):
    """-> dict(ll, grad [d + S], ll_cond, grad_cond, nnz) of the source-wise model at (z, rs) against counts [B], summed over the
    listed bins only"""
    d, S = len(model['anchor_z']), len(model['own'])
    F = d + S
    coef, rows = fo.factored_columns(model, z, rs)
    n_all = np.asarray(counts, dtype=float).ravel()
    Z = listed_bins(n_all)
    acc_ll, acc_g = Acc(()), Acc((F,))
    bad = False
    for b0 in range(0, len(Z), BLOCK):
        zb = Z[b0:b0 + BLOCK]
        block = np.array([np.asarray(model['ps'][s], dtype=float)[idx][zb] for s, idx in rows])
        X = tmatmul(coef, T(block))
        mu = X[0]
        n = n_all[zb]
        if np.any(mu.v <= 0) or np.any(n < 0) or np.any(n != np.floor(n)):
            bad = True
            break
        acc_ll.add(T.of(n) * mu.log())
        g = T.of(n) * (1.0 / mu)
        acc_g.add(X[1:1 + F] * T(g.v[None], g.a[None]))
    if bad:
        return dict(ll=-np.inf, ll_cond=0.0, grad=np.full(F, np.nan), grad_cond=np.zeros(F), nnz=len(Z))
    R = row_totals(model, rows)
    lam = tmatmul(coef, T(R.v[:, None], R.a[:, None]))                 # [1 + F, 1]: sum_s lambda_s and its derivatives
    acc_ll.add_scalar(-lam[0][0])
    acc_ll.add_scalar(-T(float(math.fsum(gammaln(n_all[Z] + 1).tolist()))))          # (weighted: the library sums it in float64)
    minus = -lam[1:1 + F]
    acc_g.add_scalar(T(minus.v[:, 0], minus.a[:, 0]))
    v, a = acc_ll.result()
    gv, ga = acc_g.result()
    return dict(ll=float(v), ll_cond=float(a), grad=gv, grad_cond=ga, nnz=len(Z))


def sparse_counts(rng, B, nnz, high=4):
    """counts [B] with exactly nnz listed bins at random places, 1 .. high events each"""
    n = np.zeros(B)
    n[rng.permutation(B)[:nnz]] = rng.integers(1, high + 1, nnz).astype(float)
    return n
