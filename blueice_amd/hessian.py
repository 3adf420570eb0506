"""Second derivatives of the log likelihood in the user's parameters: the chain rule from the device Hessian over
(z, rate_scale) to rate multipliers and shape parameters, the log10 reparametrisation of rate multipliers, and the
gradient-difference Hessian used where the device has no analytic one; the same chain rule for the expected (Fisher)
information, and the covariance it gives when some parameters' information is unbounded.  Pure numpy on [P, ...] arrays: no device, no
likelihood object (the likelihood classes feed them, tests check them against finite differences)."""
import numpy as np

LN10 = np.log(10.0)


def user_jacobian(P, d, S, mult, livetime_factor, eff, eff_axis, rate_sources):
    """J [P, F, d + S] = d theta / d user parameter, theta = (z [d], rate_scale [S]), the user's parameters and the other
    arguments as in `chain_rule_hessian` (which, with `chain_rule_information`, is built on it)."""
    Fr = len(rate_sources)
    mult = np.broadcast_to(np.asarray(mult, float), (P, S))
    eff = np.broadcast_to(np.asarray(eff, float), (P, S))
    L = float(livetime_factor)
    J = np.zeros((P, Fr + d, d + S))
    for j, s in enumerate(rate_sources):
        J[:, j, d + s] = L * eff[:, s]
    for i in range(d):
        J[:, Fr + i, i] = 1.0
    for s, i in enumerate(eff_axis):
        if i is None or i < 0:
            continue
        J[:, Fr + i, d + s] = mult[:, s] * L
    return J


def chain_rule_hessian(gz, gs, hess, mult, livetime_factor, eff, eff_axis, rate_sources, prior_g=None, prior_h=None):
    """Gradient and Hessian of ll over the user's parameters from those over theta = (z [d], rate_scale [S]).

    The user's parameters are the rate multipliers m_s of the sources in `rate_sources` (in that order), then the d shape
    parameters x_i = z_i.  rate_scale_s = m_s * L * e_s: L = `livetime_factor` (scalar), e_s = `eff` [P, S] the efficiency
    factor of source s (1 where none); eff_axis[s] = i when e_s IS shape parameter x_i (then d rate_scale_s / d x_i = m_s L and
    d2 rate_scale_s / d m_s d x_i = L), -1 when it is a constant.
    gz [P, d], gs [P, S], hess [P, d + S, d + S]; mult [P, S]; prior_g / prior_h [P, F]: slopes and curvatures of the priors
    on the user's parameters (added; None = none).  -> (g [P, F], H [P, F, F])."""
    gz, gs, hess = np.asarray(gz, float), np.asarray(gs, float), np.asarray(hess, float)
    P, d = gz.shape
    S = gs.shape[1]
    Fr = len(rate_sources)
    F = Fr + d
    L = float(livetime_factor)
    J = user_jacobian(P, d, S, mult, L, eff, eff_axis, rate_sources)
    K = np.zeros((P, F, F))                            # sum_s d ll / d rate_scale_s * d2 rate_scale_s / d user^2
    for s, i in enumerate(eff_axis):
        if i is None or i < 0:
            continue
        if s in rate_sources:
            j = list(rate_sources).index(s)
            K[:, j, Fr + i] += gs[:, s] * L
            K[:, Fr + i, j] += gs[:, s] * L
    gth = np.concatenate([gz, gs], axis=1)
    g = np.einsum('pfk,pk->pf', J, gth)
    H = np.einsum('pfk,pkl,pgl->pfg', J, hess, J) + K
    if prior_g is not None:
        g = g + prior_g
    if prior_h is not None:
        H = H + np.einsum('pf,fg->pfg', prior_h, np.eye(F))
    return g, H


def chain_rule_information(info, mult, livetime_factor, eff, eff_axis, rate_sources, prior_curvature=None):
    """Expected (Fisher) information over the user's parameters from the one over theta = (z [d], rate_scale [S]) (info
    [P, d + S, d + S], bi_eval_fisher): J I J^T with the J of `chain_rule_hessian` (`user_jacobian`; same arguments, eff_axis
    has one entry per source).  There is no second-order term: the expected score is zero.  prior_curvature [P, F]: second
    derivatives of the log priors on the user's parameters; MINUS them goes on the diagonal (a Gaussian constraint adds
    1 / sigma^2).  -> [P, F, F]."""
    info = np.asarray(info, float)
    P = info.shape[0]
    S = len(eff_axis)
    d = info.shape[1] - S
    J = user_jacobian(P, d, S, mult, livetime_factor, eff, eff_axis, rate_sources)
    out = np.einsum('pfk,pkl,pgl->pfg', J, info, J)
    out = 0.5 * (out + np.swapaxes(out, 1, 2))          # (exactly symmetric whatever order the products were summed in)
    if prior_curvature is not None:
        idx = np.arange(out.shape[1])
        out[:, idx, idx] -= np.asarray(prior_curvature, float)
    return out


def chain_rule_unbounded(unbounded, mult, livetime_factor, eff, eff_axis, rate_sources):
    """unbounded [P, d + S] (bi_eval_fisher: bins that expect nothing but move with theta_k, left out of the information) ->
    bool [P, F]: the user's parameters that move such a theta_k (J_fk != 0), whose information is unbounded too."""
    unbounded = np.asarray(unbounded)
    P = unbounded.shape[0]
    S = len(eff_axis)
    J = user_jacobian(P, unbounded.shape[1] - S, S, mult, livetime_factor, eff, eff_axis, rate_sources)
    return np.any((J != 0) & (unbounded != 0)[:, None, :], axis=2)


def covariance_from_information(info, unbounded=None):
    """Covariance from an information matrix [F, F] or [P, F, F]: parameters flagged in `unbounded` (bool, [F] or [P, F]; None:
    none) get variance 0 and covariance 0 with everything -- the limit I_qq -> inf -- and the rest is the inverse of the
    remaining block, through its Cholesky factor.  nan where that block is not finite or not positive definite."""
    info = np.asarray(info, float)
    single = info.ndim == 2
    I3 = info[None] if single else info
    P, F = I3.shape[:2]
    flag = np.zeros((P, F), bool) if unbounded is None else np.broadcast_to(np.asarray(unbounded, bool), (P, F))
    cov = np.full((P, F, F), np.nan)
    for p in range(P):
        keep = np.flatnonzero(~flag[p])
        block = I3[p][np.ix_(keep, keep)]
        if not np.all(np.isfinite(block)):
            continue
        try:
            Li = np.linalg.inv(np.linalg.cholesky(block))
        except np.linalg.LinAlgError:
            continue
        cov[p] = 0.0
        cov[p][np.ix_(keep, keep)] = Li.T @ Li
    return cov[0] if single else cov


def to_log10(g, H, values, which):
    """Gradient and Hessian after the parameters flagged in `which` [F] are replaced by y = log10(x): values [P, F] are the
    x.  dx/dy = x ln10, d2x/dy2 = x ln10^2: H'_jk = x'_j x'_k H_jk + delta_jk x''_j g_j."""
    g, H = np.asarray(g, float), np.asarray(H, float)
    values = np.asarray(values, float)
    which = np.asarray(which, bool)
    d1 = np.where(which, values * LN10, 1.0)
    d2 = np.where(which, values * LN10 ** 2, 0.0)
    g2 = g * d1
    H2 = H * d1[:, :, None] * d1[:, None, :]
    idx = np.arange(g.shape[1])
    H2[:, idx, idx] += d2 * g
    return g2, H2


def prior_derivatives(log_prior, x):
    """Central differences of a (vectorised or scalar) log prior at x [P]: -> (slope [P], curvature [P]).  The slope takes
    the step of `values_and_gradients` (1e-6 relative), the second difference a wider one (1e-4).  A GaussianPrior gives both in
    closed form."""
    from .likelihood import _prior_of
    from .priors import GaussianPrior
    x = np.asarray(x, float)
    if isinstance(log_prior, GaussianPrior):
        return log_prior.slope(x), np.full(x.shape, log_prior.curvature)
    h1 = 1e-6 * np.maximum(1.0, np.abs(x))
    h2 = 1e-4 * np.maximum(1.0, np.abs(x))
    slope = (_prior_of(log_prior, x + h1) - _prior_of(log_prior, x - h1)) / (2 * h1)
    fp, f0, fm = _prior_of(log_prior, x + h2), _prior_of(log_prior, x), _prior_of(log_prior, x - h2)
    return slope, (fp - 2 * f0 + fm) / h2 ** 2


def difference_steps(x, lo, hi, last, h):
    """Steps of a central gradient difference kept inside the point's own interval [lo, hi]: -> (x_plus, x_minus).  hi is the
    next interval's start unless `last` (the closed top interval), so x_plus stays below it: one-sided at an edge."""
    x, lo, hi, h = (np.asarray(a, float) for a in (x, lo, hi, h))
    xp = x + h
    xp = np.where(xp < hi, xp, np.where(np.asarray(last, bool), hi, x))
    xm = np.maximum(x - h, lo)
    return xp, xm
