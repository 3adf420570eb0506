"""Log priors the library understands in closed form.

Any callable works as `log_prior=` of `add_rate_parameter` / `add_shape_parameter`, here as in the reference; it is then
called on the host, between the parameters and the device call, and differentiated numerically.  A `GaussianPrior` is a
callable too, but one whose value, slope and curvature are known: the host paths use them instead of differences, and the
native fit and sampler loops (bi_fit_batched_gauss, bi_sample_stretch_gauss) add the term themselves.
"""
import math

import numpy as np

from .exceptions import InvalidParameterSpecification

__all__ = ['GaussianPrior']

_HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


class GaussianPrior:
    """log of the normal density with `mean` and `sigma`: prior(x) = -0.5 ((x - mean) / sigma)^2 - log(sigma) - 0.5 log(2 pi)
    for scalars or arrays -- what `scipy.stats.norm(mean, sigma).logpdf` returns, in closed form."""

    def __init__(self, mean, sigma):
        try:
            mean, sigma = float(mean), float(sigma)
        except (TypeError, ValueError):
            raise InvalidParameterSpecification("GaussianPrior: mean and sigma must be numbers, not %r, %r" % (mean, sigma))
        if not (math.isfinite(sigma) and sigma > 0):
            raise InvalidParameterSpecification("GaussianPrior: sigma must be finite and > 0 (got %r)" % (sigma,))
        if not math.isfinite(mean):
            raise InvalidParameterSpecification("GaussianPrior: mean must be finite (got %r)" % (mean,))
        self.mean, self.sigma = mean, sigma
        self._log_sigma = math.log(sigma)
        self.log_norm = -self._log_sigma - _HALF_LOG_2PI         # the part that does not depend on x

    def __call__(self, x):
        t = (x - self.mean) / self.sigma
        return -0.5 * (t * t) - self._log_sigma - _HALF_LOG_2PI

    def slope(self, x):
        """d prior / d x = -(x - mean) / sigma^2, as (-t) / sigma with t = (x - mean) / sigma"""
        return -((x - self.mean) / self.sigma) / self.sigma

    @property
    def curvature(self):
        """d2 prior / d x2 = -1 / sigma^2, the same everywhere"""
        return -1.0 / self.sigma ** 2

    def __repr__(self):
        return 'GaussianPrior(mean=%r, sigma=%r)' % (self.mean, self.sigma)


def gaussian_terms(lf, float_names, z, mult):
    """The Gaussian constraint terms of a likelihood whose priors are all None or GaussianPrior, split the way the native
    loops take them: float_names [F] the optimiser variables; z [P, d], mult [P, S] the shape settings and rate multipliers
    of the P problems (the floating ones' columns are not read).
    -> (prior_mean [F], prior_sigma [F] (+inf: no term on that variable), prior_const [P]: the normalisation constants of
    the floating terms plus the complete priors of the fixed parameters)."""
    F, P = len(float_names), len(z)
    mean, sigma, const = np.zeros(F), np.full(F, np.inf), np.zeros(P)

    def take(name, prior, values):
        if prior is None:
            return
        if name in float_names:
            j = float_names.index(name)
            mean[j], sigma[j] = prior.mean, prior.sigma
            const[:] += prior.log_norm
        else:
            const[:] += prior(values)

    for i, (name, (_, prior, _)) in enumerate(lf.shape_parameters.items()):
        take(name, prior, z[:, i])
    for s, name in enumerate(lf.source_name_list):
        take(name + '_rate_multiplier', lf.rate_parameters.get(name), mult[:, s])
    return mean, sigma, const
