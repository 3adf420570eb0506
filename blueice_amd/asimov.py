"""Real-valued data on the device: Asimov datasets and weighted histograms as pseudo-data.

The Asimov dataset of a truth is the expectation itself, n_b = mu_b(truth) (Cowan, Cranmer, Gross, Vitells, Eur. Phys. J. C
71 (2011) 1554): one profile scan over it gives the median expected limit, its bands and the median discovery significance
without an ensemble of toys.  Such counts are no integers, and every ordinary data path of the library keeps scipy's
`poisson.logpmf` semantics (a non-integer count is -inf), so they live in a store of their own beside the likelihood's
data (bi_set_real_counts / bi_set_asimov_counts) and are evaluated by a kernel of their own (bi_eval_real).

    view = lf.asimov(s0_rate_multiplier=0.)            # the background-only Asimov data, made on the device
    view = lf.asimov_points({'shift': [-.5, 0., .5]})  # one set per truth
    view = lf.real_data(weighted_histogram)            # any counts >= 0, [*bins] or [T, *bins]

Each returns an `AsimovLikelihood`: a view of `lf` -- same model, parameters, bounds, priors and device context; it owns
nothing but the store -- whose value is the log-likelihood ratio to the saturated model plus the priors,

    view(**p) = -half_deviance(p) + prior(p),      half_deviance = sum_b (mu_b - n_b) - n_b log(mu_b / n_b)   (n_b = 0: mu_b)

a constant (`view.saturated_ll(t)`) below the likelihood, summed bin by bin without the ~N-sized cancellation of two
log-likelihoods.  The view evaluates through the parent's own host code (`eval_points`, `values_and_gradients`, ... of
DeviceLogLikelihood: priors, live time, efficiencies, status words) over a context proxy that presents -half_deviance as the
log-likelihood, and whose `fit_batched` is bi_fit_batched_real: the batched profile-fit engine (blueice_amd.profile) runs on
its native loop unchanged.  `lf` itself is not touched: its data stay resident and usable.

A prepared `SourceWiseBinnedLogLikelihood` is taken by the three module functions as well (`asimov(lf, **truth)`,
`asimov_points(lf, points)`, `real_data(lf, counts)`): its context keeps a store of the same kind beside its counts
(bi_sourcewise_set_real_counts / bi_sourcewise_set_asimov_counts, evaluated by bi_eval_sourcewise_real and fitted by
bi_fit_batched_sourcewise_real), and the view works over it unchanged.  Of the bound names, `lf.asimov_points` is bound on that
class; `lf.asimov` and `lf.real_data` stay refused there and name these functions.

There is one store per likelihood: making a new view replaces it, and an older view then raises instead of reading another
truth's data.  Beeston-Barlow (the expectation depends on the data), unbinned likelihoods, sums and re-parametrisations are
refused; a LogLikelihoodSum OF views of different likelihoods works through the host combinator.
"""
import numpy as np
from scipy.special import gammaln, xlogy

from . import inference
from .exceptions import NotPreparedException
from .likelihood import DeviceLogLikelihood, LogAncillaryLikelihood, LogLikelihoodBase, LogLikelihoodReParam, \
    LogLikelihoodSum

__all__ = ['AsimovLikelihood', 'asimov', 'asimov_points', 'real_data']


class _RealStoreContext:
    """What the parent's evaluation code sees as `ctx` on a view: the parent's device context with the real-valued store as
    the data and -half_deviance as the log-likelihood.  Only what has a meaning on the store is exposed: anything else of
    the DeviceContext (Hessians, plans, the sampler, toys) would read the parent's ordinary data and is an AttributeError."""
    _SHARED = ('d', 'S', 'B', 'device', 'interpolate', 'get_param', 'set_param', 'info', 'expected_counts')

    def __init__(self, view):
        self._view = view

    def __getattr__(self, name):
        if name in _RealStoreContext._SHARED:
            return getattr(self._view._parent.ctx, name)
        raise AttributeError("%r is not available on the context of an AsimovLikelihood view" % name)

    @property
    def _ctx(self):
        return self._view._live_ctx()

    @property
    def T(self):
        return self._ctx.real_count_sets

    def download_counts(self, t=0):
        return self._ctx.download_real_counts(t)

    def eval_one(self, z, rate_scale=None, dataset=0):
        half, _, _, st = self._ctx.eval_real(z if z is not None and len(z) else None, None if rate_scale is None else rate_scale[None, :],
                                             dataset, gradient=False)
        return -float(half[0]), int(st[0])

    def eval(self, z, rate_scale=None, dataset=None):
        half, _, _, st = self._ctx.eval_real(z, rate_scale, dataset, gradient=False)
        return -half, st

    def eval_grad(self, z, rate_scale=None, dataset=None):
        half, gz, gs, st = self._ctx.eval_real(z, rate_scale, dataset)
        return -half, -gz, -gs, st

    def fit_batched(self, *args, **kwargs):
        return self._ctx.fit_batched_real(*args, **kwargs)


class AsimovLikelihood:
    """A view of a BinnedLogLikelihood, or of a prepared SourceWiseBinnedLogLikelihood, on real-valued data (see the module's
    docstring).  Made by `asimov`, `asimov_points` and `real_data`, not directly."""
    # the parent's state a view shares (read through to the parent: a parameter added later is seen)
    _SHARED = ('shape_parameters', 'rate_parameters', 'config', 'pdf_base_config', 'source_name_list', 'source_list',
               'source_apply_efficiency', 'source_efficiency_names', 'source_allowed_negative', 'bin_shape', 'is_prepared',
               'model_statistical_uncertainty_handling', 'base_model', 'anchor_models', 'morpher', 'get_bounds', '_batch_terms',
               '_host_terms', '_kwargs_to_settings', '_interpret', '_finish_call', '_has_non_numeric')
    is_data_set = True
    supports_hessian = False

    def __init__(self, parent, n_sets, generation):
        self._parent, self.n_sets, self._generation = parent, int(n_sets), generation
        self.ctx = _RealStoreContext(self)

    def __getattr__(self, name):
        if name in AsimovLikelihood._SHARED:
            return getattr(self._parent, name)
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def _live_ctx(self):
        """-> the parent's device context, if this view's data are still the store's"""
        if self._parent.__dict__.get('_real_store_generation') != self._generation:
            raise NotPreparedException("this AsimovLikelihood view is stale: a later asimov() / asimov_points() / real_data() of the "
                                       "same likelihood replaced its data")
        return self._parent.ctx

    @property
    def supports_gradient(self):
        return self._parent.supports_gradient and self._parent.model_statistical_uncertainty_handling is None

    def counts(self, t=0):
        """-> the real-valued counts of set t, in the likelihood's bin shape"""
        return self.ctx.download_counts(t).reshape(tuple(self.bin_shape))

    def saturated_ll(self, t=0):
        """The constant between the view and the log-likelihood: log L of the saturated model mu_b = n_b on set t, with
        lgamma(n + 1) in the place of log n!  --  log L(p) = saturated_ll - half_deviance(p)."""
        n = self.ctx.download_counts(t)
        return float(np.sum(xlogy(n, n) - n - gammaln(n + 1)))

    def __call__(self, livetime_days=None, compute_pdf=False, full_output=False, dataset=0, **kwargs):
        if compute_pdf or full_output:
            raise NotImplementedError("an AsimovLikelihood view evaluates the morphed model only (no compute_pdf / full_output)")
        prior, zs, scale = self._host_terms(livetime_days, kwargs)
        if prior is None:
            return -float('inf')
        ll, st = self.ctx.eval_one(zs, scale, dataset)
        return self._finish_call(prior, zs, scale, ll, st)

    # the parent's batched entry points, over the store
    eval_points = DeviceLogLikelihood.eval_points
    value_and_gradient = DeviceLogLikelihood.value_and_gradient
    _prior_slope = staticmethod(DeviceLogLikelihood._prior_slope)

    def values_and_gradients(self, points, livetime_days=None, dataset=None):
        return DeviceLogLikelihood.values_and_gradients(self, points, livetime_days=livetime_days, dataset=dataset)


for _name in inference.__all__:
    setattr(AsimovLikelihood, _name, getattr(inference, _name))


def _binned_or_source_wise(lf, what):
    """The gate of the factories: a `BinnedLogLikelihood` without Beeston-Barlow (`inference._binned_for_gof`), or a prepared
    `SourceWiseBinnedLogLikelihood`, whose context keeps a real-valued store of its own under the same method names
    (bi_sourcewise_set_real_counts ... bi_fit_batched_sourcewise_real).  `_binned_for_gof` itself keeps refusing that class."""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if isinstance(lf, SourceWiseBinnedLogLikelihood):
        if not lf.is_prepared:
            raise NotPreparedException("%s requires you to first prepare the likelihood function using prepare()" % what)
        return lf
    return inference._binned_for_gof(lf, what)


def _new_view(lf, what, fill):
    """The factories' common part: refuse what has no real-valued path, fill the store (fill(ctx) -> sets), hand out the view."""
    _binned_or_source_wise(lf, what)
    n_sets = fill(lf.ctx)
    lf._real_store_generation = generation = object()
    return AsimovLikelihood(lf, n_sets, generation)


def asimov(lf, livetime_days=None, **truth):
    """The Asimov dataset of `truth` (parameter values; absent parameters at their defaults), n_b = mu_b(truth), made on
    the device -> an AsimovLikelihood view on it.  No observed data are needed.  ValueError for a truth outside the anchor
    box, with unphysical rates or with a negative expectation in some bin."""
    def fill(ctx):
        prior, zs, scale = lf._host_terms(livetime_days, truth)
        if prior is None:
            raise ValueError("asimov: the truth lies outside the anchor box")
        return ctx.set_asimov_counts(zs if len(zs) else None, scale[None, :])
    return _new_view(lf, 'asimov', fill)


def asimov_points(lf, points, livetime_days=None):
    """One Asimov dataset per truth: points = dict parameter name -> array [H] (as `eval_points`) -> a view on H sets,
    addressed by the `dataset` of its batched entry points (`bestfit_batched(view, datasets=...)`)."""
    def fill(ctx):
        z, scale, _ = lf._batch_terms(points, livetime_days)
        return ctx.set_asimov_counts(z if z.shape[1] else None, scale)
    return _new_view(lf, 'asimov_points', fill)


def real_data(lf, counts):
    """Real-valued counts as data: counts [*bins] or [T, *bins], every one finite and >= 0 (a weighted-MC histogram as
    pseudo-data in a closure test) -> a view on them."""
    def fill(ctx):
        c = np.asarray(counts, dtype=float)
        shape = tuple(lf.bin_shape)
        if c.shape != shape and c.shape[1:] != shape:
            raise ValueError("real_data: counts of shape %s, need %s or (T,) + %s" % (c.shape, shape, shape))
        ctx.set_real_counts(c)
        return ctx.real_count_sets
    return _new_view(lf, 'real_data', fill)


# the three factories double as methods; on what is no BinnedLogLikelihood they refuse with the reason
for _cls in (LogLikelihoodBase, LogLikelihoodSum, LogAncillaryLikelihood, LogLikelihoodReParam):
    for _name in ('asimov', 'asimov_points', 'real_data'):
        setattr(_cls, _name, globals()[_name])
