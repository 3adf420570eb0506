"""A numpy Fisher information of the binned Poisson likelihood for tests, over theta = (z [d], rate_scale [S]):

    I_qr = sum_b d_q mu_b d_r mu_b / mu_b        over the bins with mu_b > 0

from tests/hessian_oracle._mu_derivatives (exact face differences of `oracle.blueice_oracle`'s interpolation inside the cell
the point is assigned to).  With it: every entry's own condition cond_qr = sum_b |d_q mu_b d_r mu_b| / mu_b (what a sum of
rounded terms is measured against), the per-parameter number of bins with mu_b == 0 and d_q mu_b != 0 (unbounded information,
left out of the sums), and the total expectation.  `information_longdouble` forms the same sums in extended precision from
the same mu and dmu: what the float64 sums above lose to their own summation.  Test infrastructure only."""
import numpy as np

import hessian_oracle as ho


def information(model, z, rs):
    """-> dict(info [F, F], cond [F, F], unbounded [F] int, total, negative: some bin expects less than nothing or nan)"""
    mu, dmu, _, _, _, _ = ho._mu_derivatives(model, z, rs)
    return _sums(mu, dmu, float)


def information_longdouble(model, z, rs):
    """the same sums with every product, quotient and addition in numpy's longdouble"""
    mu, dmu, _, _, _, _ = ho._mu_derivatives(model, z, rs)
    return _sums(mu, dmu, np.longdouble)


def _sums(mu, dmu, dtype):
    mu, dmu = np.asarray(mu, dtype=dtype), np.asarray(dmu, dtype=dtype)
    pos = mu > 0
    a = dmu[:, pos]
    info = np.einsum('qb,rb->qr', a / mu[pos], a)
    cond = np.einsum('qb,rb->qr', np.abs(a) / mu[pos], np.abs(a))
    unbounded = np.count_nonzero((dmu != 0) & (mu == 0)[None, :], axis=1)
    return dict(info=info, cond=cond, unbounded=unbounded.astype(np.int64), total=mu.sum(), negative=bool(np.any(~(mu >= 0))))


def check(info, want, what='', tol=1e-10):
    """|info - oracle| <= tol max(1, cond) per entry (the bound tests/test_real_counts_gpu.py holds gradient entries to) ->
    the largest |err| / max(1, cond)"""
    err = np.abs(np.asarray(info, dtype=float) - np.asarray(want['info'], dtype=float))
    scale = np.maximum(1.0, np.asarray(want['cond'], dtype=float))
    assert np.all(err <= tol * scale), '%s: information %r, want %r (cond %r)' % (what, info, want['info'], want['cond'])
    return float(np.max(err / scale)) if err.size else 0.0
