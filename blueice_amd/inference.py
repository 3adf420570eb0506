"""Fit drivers over a likelihood callable: the `bestfit_scipy` path of the reference
(blueice/inference.py:57-178) plus a batched `best_anchor` (:34-54).

These only need `lf(**kwargs) -> float`, `lf.rate_parameters`, `lf.shape_parameters`,
`lf.get_bounds`, `lf.pdf_base_config`; scipy.optimize is used as is.

Posteriors: `sample_posterior` (blueice_amd.sampler) runs an affine-invariant ensemble sampler over the floating parameters
-- on the device from proposal to chain where the likelihood is one device context -- and `bestfit_emcee` is the
reference's emcee driver (blueice/inference.py:254-321) on top of it; emcee itself is not used.  `plot_likelihood_ratio`
(:392-443) draws what `likelihood_ratio_scan` computes.

Uncertainties: `hesse` turns fitted values into the covariance (-H)^-1 of the floating parameters from the device Hessian
of the likelihood (`values_gradients_hessians`: bi_eval_hess, one call for a whole ensemble of fits), and
`bestfit_minuit` -- the reference's iminuit driver (blueice/inference.py:181-244) -- returns the batched engine's fit with
the parabolic errors sqrt(diag((-H)^-1)) that MIGRAD reports at errordef = 0.5.  iminuit itself is not used.

Goodness of fit: `gof_statistics` evaluates the deviance and Pearson's chi2 of the data term on the device (bi_eval_gof),
`goodness_of_fit` calibrates either with toys fitted like the data, and `expected_counts` hands back the per-bin expectation
the statistics are made of (bi_expected_counts).  Plain binned likelihoods only.  `expected_coarse`, `expected_coarse_points`
and `coarse_counts` (blueice_amd.coarse) sum the expectation and the data over the cells of a `CoarseBinning` on the device
-- projections with their components, a signal box -- and `gof_statistics` / `goodness_of_fit` take such a binning to test
where the data can tell.

Expected results without toys: `asimov_test_statistic`, `expected_upper_limit` and `expected_discovery_significance` profile
the Asimov dataset of a truth (blueice_amd.asimov: n_b = mu_b(truth), real-valued counts in a device store of their own) and
apply the asymptotic formulae of Cowan, Cranmer, Gross and Vitells.

Profiled quantities -- `likelihood_ratio_scan` with floating nuisances, `one_parameter_interval` -- run on the batched
profile-fit engine (blueice_amd.profile: all hypotheses advance together, one device call per optimiser iteration)
whenever the likelihood offers batched evaluation; a user-supplied `bestfit_routine` keeps the reference's sequential
loops (blueice/inference.py:332-443).
"""
from collections import OrderedDict
from copy import deepcopy

import warnings

import numpy as np
from scipy import stats
from scipy.optimize import brentq, minimize

from .exceptions import NoOpimizationNecessary, NotPreparedException, OptimizationFailed
from .hessian import chain_rule_information, chain_rule_unbounded, covariance_from_information, prior_derivatives, to_log10
from .profile import bestfit_batched, supports_batched_fits
from .sampler import sample_posterior
from .utils import is_numeric
from .coarse import (CoarseBinning, _binned_for_gof, _prepared, coarse_counts, coarse_information, coarse_statistics, expected_coarse,
                     expected_coarse_band, expected_coarse_jacobian, expected_coarse_jacobian_points, expected_coarse_points)

__all__ = ['best_anchor', 'make_objective', 'bestfit_scipy', 'bestfit_device', 'bestfit_batched', 'bestfit_toys', 'toy_mc_fits',
           'toy_test_statistics', 'neyman_thresholds', 'expected_counts', 'expected_counts_points', 'gof_statistics', 'goodness_of_fit',
           'expected_coarse', 'expected_coarse_points', 'coarse_counts',
           'expected_coarse_jacobian', 'expected_coarse_jacobian_points', 'expected_coarse_band', 'coarse_information',
           'asimov_test_statistic', 'expected_upper_limit', 'expected_discovery_significance',
           'fisher_information_points', 'fisher_information', 'expected_covariance', 'expected_errors',
           'one_parameter_interval', 'likelihood_ratio_scan', 'hesse', 'bestfit_minuit', 'sample_posterior', 'bestfit_emcee',
           'plot_likelihood_ratio']


def best_anchor(lf):
    """Shape-parameter dict of the anchor model with the highest likelihood -- all anchors in one
    batched device call when the likelihood offers `eval_points`."""
    if not len(lf.shape_parameters):
        return dict()
    names = list(lf.shape_parameters.keys())
    anchors = list(lf.anchor_models.keys())
    if hasattr(lf, 'eval_points'):
        results = lf.eval_points({n: [a[j] for a in anchors] for j, n in enumerate(names)})
    else:
        results = np.array([lf(**dict(zip(names, a))) for a in anchors])
    return dict(zip(names, anchors[int(np.argmax(results))]))


_FD_STEP = float(np.finfo(np.float64).eps) ** 0.5          # scipy.optimize._numdiff: relative step of '2-point' differences


def make_objective(lf, guess=None, minus=True, rates_in_log_space=False, with_gradient=False,
                   stencil_respects_bounds=False, **kwargs):
    """-> (f(x), names, guesses, bounds) over the parameters not fixed through kwargs.
    Rate multipliers come first (guess 1, bounds (0, None)), then shape parameters (bounds from the
    anchors, guess = base setting).  with_gradient (extensions, both for `scipy.optimize.minimize(..., jac=True)`):
    True -> f returns (value, analytic gradient) from one device pass (`lf.value_and_gradient`);
    'stencil' -> f returns (value, scipy's forward-difference gradient), the F + 1 stencil points evaluated in ONE
    batched device call (`lf.eval_points`)."""
    guess = guess or {}
    names, guesses, bounds = [], [], []
    for src in lf.rate_parameters:
        key = '%s_rate_multiplier' % src
        if key in kwargs:
            continue
        g = guess.get(key, 1)
        names.append(key)
        guesses.append(np.log10(g) if rates_in_log_space else g)
        bounds.append((None, None) if rates_in_log_space else (0, None))
    for key, (_, _, base_value) in lf.shape_parameters.items():
        if key in kwargs:
            continue
        g = guess.get(key)
        if g is None:
            g = lf.pdf_base_config.get(key)
            if not is_numeric(g):
                g = base_value
        names.append(key)
        guesses.append(g)
        bounds.append(lf.get_bounds(key))
    if not names:
        raise NoOpimizationNecessary("There are no parameters to fit, no optimization is necessary")
    sign = -1 if minus else 1
    log_rate = [rates_in_log_space and n.endswith('_rate_multiplier') for n in names]

    def objective(args):
        call = {n: (10 ** a if lg else a) for n, a, lg in zip(names, args, log_rate)}
        call.update(kwargs)
        return lf(**call) * sign

    def objective_with_gradient(args):
        call = {n: (10 ** a if lg else a) for n, a, lg in zip(names, args, log_rate)}
        call.update(kwargs)
        value, grads = lf.value_and_gradient(**call)
        g = np.array([grads[n] * (np.log(10.) * call[n] if lg else 1.0) for n, lg in zip(names, log_rate)])
        if not np.isfinite(value):
            g = np.zeros(len(names))
        return value * sign, g * sign

    def objective_with_stencil(args):
        """Value AND scipy's own forward-difference gradient from ONE batched device call: scipy's default minimiser
        differences the objective numerically, F + 1 scalar calls per gradient (blueice/inference.py:111-124,153-155 via
        scipy.optimize._numdiff); the F + 1 stencil points are independent, so they go to `lf.eval_points` together --
        same points (scipy's step sqrt(eps) * sign(x) * max(1, |x|), turned around at an upper bound), same
        differences, one launch in which the points of a grid cell share one pass over its templates."""
        args = np.asarray(args, dtype=float)
        F = len(args)
        h = _FD_STEP * np.where(args >= 0, 1.0, -1.0) * np.maximum(1.0, np.abs(args))
        for j, (lo_j, hi_j) in enumerate(stencil_bounds):
            if hi_j is not None and args[j] + h[j] > hi_j:
                h[j] = -abs(h[j])
            elif lo_j is not None and args[j] + h[j] < lo_j:
                h[j] = abs(h[j])
        pts = np.repeat(args[None, :], F + 1, axis=0)
        pts[np.arange(1, F + 1), np.arange(F)] += h
        call = {n: (10 ** pts[:, j] if lg else pts[:, j]) for j, (n, lg) in enumerate(zip(names, log_rate))}
        call.update(kwargs)
        vals = np.asarray(lf.eval_points(call), dtype=float) * sign
        with np.errstate(invalid='ignore'):
            grad = (vals[1:] - vals[0]) / ((args + h) - args)
        return vals[0], grad

    # bounds the stencil must respect: only those the minimiser is told about (pass_bounds_to_minimizer); without them
    # scipy steps blindly, and so does this
    stencil_bounds = [(None, None)] * len(names) if not stencil_respects_bounds else \
        [(None if b[0] in (None, -np.inf) else b[0], None if b[1] in (None, np.inf) else b[1]) for b in bounds]
    if with_gradient == 'stencil':
        return objective_with_stencil, names, np.array(guesses), bounds
    return (objective_with_gradient if with_gradient else objective), names, np.array(guesses), bounds


def bestfit_scipy(lf, minimize_kwargs=None, rates_in_log_space=False, pass_bounds_to_minimizer=False,
                  use_gradient=False, batch_stencil=True, **kwargs):
    """Maximise lf over its floating parameters -> (OrderedDict name -> value, max log likelihood).
    scipy's default minimizer first, Nelder-Mead as the fallback, OptimizationFailed after that.
    use_gradient=True (extension): hand scipy the analytic gradient computed in the same device pass as
    the value instead of letting it difference the objective numerically (n_parameters + 1 calls per step).
    batch_stencil (default on, when the likelihood evaluates batches): scipy still gets its own forward differences,
    but the n_parameters + 1 points behind each of them are evaluated in one device call (`make_objective`,
    with_gradient='stencil'); batch_stencil=False is the reference's stream of scalar calls."""
    minimize_kwargs = minimize_kwargs or {}
    use_gradient = use_gradient and bool(getattr(lf, 'supports_gradient', False))
    # scipy's gradient-based default methods difference the objective numerically: hand them the same differences, with
    # the stencil evaluated as one batch (not for methods that take no gradient, nor when the caller brings a jac)
    stencil = batch_stencil and not use_gradient and hasattr(lf, 'eval_points') and 'jac' not in minimize_kwargs and \
        str(minimize_kwargs.get('method', 'BFGS')).lower() in ('bfgs', 'l-bfgs-b', 'cg', 'slsqp', 'tnc')
    mode = dict(with_gradient=True) if use_gradient else \
        (dict(with_gradient='stencil', stencil_respects_bounds=pass_bounds_to_minimizer) if stencil else {})
    try:
        f, names, guess, bounds = lf.make_objective(minus=True, rates_in_log_space=rates_in_log_space, **dict(kwargs, **mode))
    except NoOpimizationNecessary:
        return {}, lf(**kwargs)
    use_bounds = bounds if pass_bounds_to_minimizer else None
    res = minimize(f, guess, bounds=use_bounds, **(dict(minimize_kwargs, jac=True) if mode else minimize_kwargs))
    if not res.success:
        retry = deepcopy(minimize_kwargs)
        retry.pop('method', None)
        if mode:
            f, names, guess, bounds = lf.make_objective(minus=True, rates_in_log_space=rates_in_log_space, **kwargs)
        res = minimize(f, guess, bounds=use_bounds, method='Nelder-Mead', **retry)
        if not res.success:
            raise OptimizationFailed("Optimization failure: ", res)
    x = res.x if len(names) != 1 else [res.x.item()]
    out = OrderedDict()
    for n, v in zip(names, x):
        out[n] = 10 ** v if (rates_in_log_space and n.endswith('_rate_multiplier')) else v
    return out, -res.fun


def bestfit_device(lf, guess=None, **kwargs):
    """`bestfit_scipy`'s signature and return value -- (OrderedDict name -> float, max log likelihood) -- from the batched
    engine with a single problem: analytic gradient, the kinks of the morph at the anchors handled as kinks (every fit
    starts on one: base values are anchors), starts in the other grid cells.  On C2 about half the time of scipy's
    minimiser on the same device likelihood, and a maximum that is never lower.  A drop-in wherever the reference takes a
    `bestfit_routine` (blueice/inference.py:324-330).  kwargs: parameters held fixed, as `bestfit_scipy`."""
    if not supports_batched_fits(lf):
        return bestfit_scipy(lf, guess=guess, **kwargs)
    try:
        best, ll = bestfit_batched(lf, guess=guess, **kwargs)
    except NoOpimizationNecessary:
        return {}, lf(**kwargs)
    return OrderedDict((k, float(v[0])) for k, v in best.items()), float(ll[0])


def _simulate_toys_at(lf, n_toys, seed, livetime_days, truth):
    """The one place where the toy layers call a generator.  n_toys an int and truth a dict of scalars: `lf.simulate_toys(n_toys,
    seed=, livetime_days=, **truth)` -- spelled as `simulate_toys_points` with a one-row `points` dict for a class that says so
    (`toys_through_points`: a source-wise model, whose bound `simulate_toys` stays refused).  n_toys an array [H] and truth a
    dict of arrays [H]: `lf.simulate_toys_points(truth, n_toys, ...)`, toys of several truths from one generator call.  An
    unbinned source-wise model takes both through its private `_simulate_toys_points` (source_wise_unbinned.py: its bound
    generator names stay refused).  The toys are the same either way: toy t of the call is toy toy_offset + t of the seed's
    ensemble."""
    points = np.ndim(n_toys) > 0
    draw = getattr(lf, '_simulate_toys_points', None)
    if draw is None and (points or getattr(type(lf), 'toys_through_points', False)):
        draw = lf.simulate_toys_points
    if draw is None:
        lf.simulate_toys(n_toys, seed=seed, livetime_days=livetime_days, **truth)
    elif points:
        draw(truth, n_toys, seed=seed, livetime_days=livetime_days)
    else:
        draw({k: np.array([float(v)]) for k, v in truth.items()}, [int(n_toys)], seed=seed, livetime_days=livetime_days)


def _binned_or_source_wise(lf, what, binning=None):
    """The gate of the layers that also take a source-wise model (toy fits, goodness of fit, expected_counts_points): a
    `BinnedLogLikelihood` without Beeston-Barlow (`_binned_for_gof`), or a prepared `SourceWiseBinnedLogLikelihood`, for which
    `binning` must be None or a `CoarseBinning` (bi_sourcewise_expected_coarse, bi_sourcewise_coarse_counts)."""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if isinstance(lf, SourceWiseBinnedLogLikelihood):
        if binning is not None and not isinstance(binning, CoarseBinning):
            raise NotImplementedError("%s(binning=...) is not available for a source-wise model (SourceWiseBinnedLogLikelihood) with a "
                                      "%s: its coarse views take a blueice_amd.coarse.CoarseBinning" % (what, type(binning).__name__))
        if not lf.is_prepared:
            raise NotPreparedException("%s requires you to first prepare the likelihood function using prepare()" % what)
        return lf
    return _binned_for_gof(lf, what)


def bestfit_toys(lf, t0=0, t1=None, **kwargs):
    """Fit every dataset the likelihood holds -- the toys of `simulate_toys`, or a stack handed to `set_binned_data` --
    at the same time: one problem per dataset on the batched profile-fit engine, one device call per optimiser iteration
    for all of them.  The reference's toy-MC loop is `d = lf.base_model.simulate(); lf.set_data(d); bestfit_scipy(lf)`,
    one toy after the other (blueice/model.py:69-91, inference.py:131-178).  kwargs: as `bestfit_batched` (fixed
    parameters, guess, ...).  -> (OrderedDict name -> fitted values [t1 - t0], max log likelihood [t1 - t0]).

    Device-generated toys exist as non-empty-bin lists only; evaluating them at a parameter point of their own needs the
    compacted templates of every toy (rows x non-empty bins x 8 bytes per toy: 41 MB at 4 sources x 5^3 anchors and
    10^4 events), within `compact_budget` (16 GB unless raised with lf.ctx.set_param BEFORE the toys are made)."""
    ctx = getattr(lf, 'ctx', None)
    if ctx is None:
        raise NotImplementedError("bestfit_toys needs a likelihood with its datasets on one device context")
    t1 = ctx.T if t1 is None else t1
    if not 0 <= t0 < t1 <= ctx.T:
        raise ValueError("datasets [%d, %d) of %d" % (t0, t1, ctx.T))
    return bestfit_batched(lf, datasets=np.arange(t0, t1), **kwargs)


def toy_mc_fits(lf, n_toys, chunk=256, seed=0, truth=None, livetime_days=None, first_toy=0, **fit_kwargs):
    """A toy-MC ensemble with a fit per toy, start to finish on the device: `n_toys` toys (binned, or event-level for an
    unbinned likelihood) drawn at the parameter
    values `truth` (dict; defaults elsewhere) and fitted, `chunk` toys at a time (`simulate_toys` + `bestfit_toys`) -- the
    reference's `for _ in range(n_toys): d = lf.base_model.simulate(); lf.set_data(d); bestfit_scipy(lf)`
    (blueice/model.py:69-91, inference.py:131-178).  The toys are numbered globally (the generator's counters are
    (seed, toy number, bin)), so the ensemble does not depend on `chunk`: that only bounds the HBM taken by the toys'
    compacted templates (see `bestfit_toys`).  first_toy: the number of this call's first toy -- ranks that each take a range
    of one ensemble (one process per GPU) draw the toys one process would.  fit_kwargs: parameters held fixed, `guess`, ...
    as `bestfit_batched`.  A SourceWiseUnbinnedLogLikelihood is taken too (its event toys: sourcewise_event_toys_points).
    -> (OrderedDict name -> fitted values [n_toys], max log likelihood [n_toys]).  Afterwards the likelihood's data are
    the toys of the last chunk."""
    ctx = getattr(lf, 'ctx', None)
    if ctx is None and hasattr(lf, '_device_context'):
        ctx = lf._device_context()             # (an unbinned likelihood makes its context with its first data)
    if ctx is None or not hasattr(lf, 'simulate_toys'):
        raise NotImplementedError("toy_mc_fits needs a binned or an unbinned likelihood with simulate_toys on one device context")
    best, lls = None, []
    try:
        for t0 in range(0, int(n_toys), int(chunk)):
            n = min(int(chunk), int(n_toys) - t0)
            ctx.set_param('toy_offset', int(first_toy) + t0)
            _simulate_toys_at(lf, n, seed, livetime_days, truth or {})
            b, ll = bestfit_toys(lf, livetime_days=livetime_days, **fit_kwargs)
            lls.append(ll)
            if best is None:
                best = OrderedDict((k, [v]) for k, v in b.items())
            else:
                for k, v in b.items():
                    best[k].append(v)
    finally:
        ctx.set_param('toy_offset', 0)
    return OrderedDict((k, np.concatenate(v)) for k, v in best.items()), np.concatenate(lls)


class ToyStatistics:
    """What `toy_test_statistics` returns: t [H, n] -- 2 (ll_free - ll_cond), raw (rounding can leave it a hair below 0), and
    0 where the one-sided rule says so --, ll_free, ll_cond, best (OrderedDict name -> the free fit's values [H, n]) and
    target_hat [H, n] (its entry of the target), hypotheses [H], kind, and the flags of the fits: converged / failed [H, n] (both fits of the toy converged or stalled on a
    flat stretch; either of them failed), n_converged, n_failed, and engine_calls (fit-engine and evaluation calls made)."""

    def __init__(self, hypotheses, kind, t, ll_free, ll_cond, target_hat, converged, failed, engine_calls=0, best=None):
        self.hypotheses, self.kind = np.asarray(hypotheses, dtype=float), kind
        self.t, self.ll_free, self.ll_cond, self.target_hat, self.best = t, ll_free, ll_cond, target_hat, best
        self.converged, self.failed = converged, failed
        self.n_converged, self.n_failed = int(np.count_nonzero(converged)), int(np.count_nonzero(failed))
        self.engine_calls = int(engine_calls)


def _resident_data(lf, ctx):
    """-> a callable that gives `lf` the data back that it holds now, or None where that is not possible"""
    if not getattr(lf, 'is_data_set', False):
        return None
    events_only = hasattr(lf, '_simulate_toys_points')     # (an unbinned source-wise model: its bound set_binned_data is a refusal)
    if not events_only and hasattr(lf, 'set_binned_data') and ctx is not None and hasattr(ctx, 'download_counts'):
        counts = np.stack([ctx.download_counts(t) for t in range(int(ctx.T))])
        counts = counts.reshape(((len(counts),) if len(counts) > 1 else ()) + tuple(lf.bin_shape))
        events = getattr(lf, '_data', None)

        def restore():
            lf.set_binned_data(counts)
            if events is not None:
                lf._data = events
        return restore
    if getattr(lf, '_data', None) is not None and hasattr(lf, 'set_data'):
        events = lf._data
        return lambda: lf.set_data(events)
    return None


def toy_test_statistics(lf, target, hypotheses, n_toys, seed=0, kind='central', truth=None, chunk=256, first_toy=0, toy_range=None,
                        livetime_days=None, fit_options=None, **fixed):
    """The profile-likelihood-ratio test statistic of `n_toys` toys at each of H hypotheses of `target`: the distribution
    that a toy-calibrated (Neyman) interval takes its critical values from, where `one_parameter_interval` by default
    takes Wilks' chi-square.

    Toy j of hypothesis i is drawn at {target: hypotheses[i], **truth_i} (truth: dict of nuisance values, scalars or
    arrays [H]; other parameters at their defaults) and is toy D = first_toy + i n_toys + j of the seed's ensemble: the
    result does not depend on `chunk`, and ranks can each take toy_range = (j0, j1), the toys j0 <= j < j1 of every
    hypothesis.  Toys are drawn and fitted `chunk` at a time.  A likelihood with `simulate_toys_points` (binned; an unbinned
    source-wise model through sourcewise_event_toys_points) gets chunks
    that run across hypothesis boundaries -- toys of several hypotheses from one generator call, fitted in one engine
    call per fit; any other likelihood with `simulate_toys` (unbinned; a duck-typed one) gets chunks of one hypothesis, with
    its context's toy_offset set as `toy_mc_fits` does -- as does a toy_range that leaves toys out (the numbers of a
    generator call are consecutive).

    The fit recipe, per chunk of m toys with h_of_toy [m] the hypothesis of every toy:
      conditional:  bestfit_batched(lf, points={target: h_of_toy}, datasets=arange(m), **fit_options, **fixed)
                    (`eval_points` where nothing is left to profile);
      free:         bestfit_batched(lf, datasets=arange(m), also_from=[the conditional solution with target = h_of_toy], ...):
                    the free maximum is never started below the conditional one.
    t = 2 (ll_free - ll_cond), not clipped; for kind 'upper' t = 0 where target_hat >= hypothesis, for 'lower' where
    target_hat <= hypothesis (the rule `one_parameter_interval` applies to the data); 'central' keeps every t.
    fixed (kwargs): parameters held fixed in both fits.  -> ToyStatistics.

    Afterwards the likelihood has its own data back where that is possible: a binned likelihood's resident datasets are read
    (`download_counts`) before and handed to `set_binned_data` after -- the same counts, as a dense stack; an unbinned
    one (an unbinned source-wise model too) gets `set_data` of the events it still holds.  It is not possible for datasets that exist on the device only
    (`set_datasets`, simulated events): then the toys of the last chunk stay, as after `toy_mc_fits`."""
    if kind not in ('upper', 'lower', 'central'):
        raise ValueError("kind must be 'upper', 'lower' or 'central'")
    hyp = np.atleast_1d(np.asarray(hypotheses, dtype=float))
    H, n = len(hyp), int(n_toys)
    j0, j1 = (0, n) if toy_range is None else (int(toy_range[0]), int(toy_range[1]))
    if not 0 <= j0 < j1 <= n:
        raise ValueError("toy_range (%d, %d) of %d toys per hypothesis" % (j0, j1, n))
    nj, chunk = j1 - j0, max(int(chunk), 1)
    truth = {k: np.broadcast_to(np.asarray(v, dtype=float), (H,)) for k, v in (truth or {}).items()}
    fit_options = dict(fit_options or {})
    more_starts = list(fit_options.pop('also_from', ()))
    ctx = getattr(lf, 'ctx', None)
    if ctx is None and hasattr(lf, '_device_context'):
        ctx = lf._device_context()             # (an unbinned likelihood makes its context with its first data)
    if not hasattr(lf, 'simulate_toys') or not supports_batched_fits(lf):
        raise NotImplementedError("toy_test_statistics needs a likelihood with simulate_toys and batched evaluation")
    mixed = hasattr(lf, 'simulate_toys_points') and nj == n
    restore = _resident_data(lf, ctx)
    out = {k: np.empty(H * nj) for k in ('ll_free', 'll_cond', 'target_hat')}
    flags = {k: np.zeros(H * nj, dtype=bool) for k in ('converged', 'failed')}
    calls, fitted = 0, None
    try:
        f0 = 0
        while f0 < H * nj:                     # toys in hypothesis-major order: toy f is (i, j) = (f // nj, j0 + f % nj)
            f1 = min(f0 + chunk, H * nj if mixed else (f0 // nj + 1) * nj)
            i_of = np.arange(f0, f1) // nj
            i_a, i_b = int(i_of[0]), int(i_of[-1]) + 1
            if ctx is not None:
                ctx.set_param('toy_offset', int(first_toy) + i_a * n + j0 + f0 % nj)
            if mixed:
                pts = {k: v[i_a:i_b] for k, v in truth.items()}
                pts[target] = hyp[i_a:i_b]
                _simulate_toys_at(lf, np.bincount(i_of - i_a, minlength=i_b - i_a), seed, livetime_days, pts)
            else:
                _simulate_toys_at(lf, f1 - f0, seed, livetime_days,
                                  dict({k: float(v[i_a]) for k, v in truth.items()}, **{target: float(hyp[i_a])}))
            ds, h_of_toy = np.arange(f1 - f0), hyp[i_of]
            try:
                start, ll_cond, info_c = bestfit_batched(lf, points={target: h_of_toy}, datasets=ds, livetime_days=livetime_days,
                                                         return_info=True, also_from=more_starts, **fit_options, **fixed)
                calls += info_c['calls']
            except NoOpimizationNecessary:
                start, info_c = {}, None
                ll_cond = np.asarray(lf.eval_points(dict(fixed, **{target: h_of_toy}), livetime_days=livetime_days, dataset=ds))
                calls += 1
            start = dict(start, **{target: h_of_toy})
            best, ll_free, info_f = bestfit_batched(lf, datasets=ds, livetime_days=livetime_days, return_info=True,
                                                    also_from=more_starts + [start], **fit_options, **fixed)
            calls += info_f['calls']
            out['ll_free'][f0:f1], out['ll_cond'][f0:f1], out['target_hat'][f0:f1] = ll_free, ll_cond, best[target]
            if fitted is None:
                fitted = OrderedDict((k, np.empty(H * nj)) for k in best)
            for k, v in best.items():
                fitted[k][f0:f1] = v
            done, bad = info_f['converged'] | info_f['stalled'], np.array(info_f['failed'], dtype=bool)
            if info_c is not None:
                done, bad = done & (info_c['converged'] | info_c['stalled']), bad | info_c['failed']
            flags['converged'][f0:f1], flags['failed'][f0:f1] = done, bad
            f0 = f1
    finally:
        if ctx is not None:
            ctx.set_param('toy_offset', 0)
        if restore is not None:
            restore()
    out = {k: v.reshape(H, nj) for k, v in out.items()}
    t = 2 * (out['ll_free'] - out['ll_cond'])
    if kind == 'upper':
        t = np.where(out['target_hat'] >= hyp[:, None], 0.0, t)
    elif kind == 'lower':
        t = np.where(out['target_hat'] <= hyp[:, None], 0.0, t)
    return ToyStatistics(hyp, kind, t, out['ll_free'], out['ll_cond'], out['target_hat'], flags['converged'].reshape(H, nj),
                         flags['failed'].reshape(H, nj), calls, OrderedDict((k, v.reshape(H, nj)) for k, v in fitted.items()))


class ToyThresholds:
    """Critical values of the test statistic from toys: a `t_ppf(hypothesis, quantile)` for `one_parameter_interval`.

    At each tabulated hypothesis the value is the empirical quantile of t over its toys on the conservative side
    (numpy.quantile(..., method='higher'): an order statistic, never an interpolation below one); between hypotheses it is
    interpolated linearly, beyond the first and last it is held constant.  The level of that quantile is chosen so that the
    table's large-sample (Wilks) limit is what `one_parameter_interval` compares with by default, norm.ppf(quantile)**2:
      kind 'upper' / 'lower': t is half chi-square, P(t <= c) = Phi(sqrt(c)) -> level = quantile (for a quantile below 1/2
                              -- kind 'lower' searches with 1 - confidence_level -- its mirror image 1 - quantile, which has
                              the same norm.ppf(quantile)**2);
      kind 'central':         t is chi-square with one degree of freedom, P(t <= c) = 2 Phi(sqrt(c)) - 1 -> level = |2 quantile - 1|.
    A level above 1 - 1/n needs more than the n toys per hypothesis of the table, and is refused."""

    def __init__(self, hypotheses, t, kind):
        if kind not in ('upper', 'lower', 'central'):
            raise ValueError("kind must be 'upper', 'lower' or 'central'")
        hyp, t = np.atleast_1d(np.asarray(hypotheses, dtype=float)), np.atleast_2d(np.asarray(t, dtype=float))
        if t.shape[0] != len(hyp) or t.shape[1] < 1 or not np.all(np.isfinite(t)):
            raise ValueError("need a finite table t [H, n] with a row per hypothesis")
        order = np.argsort(hyp, kind='stable')
        self.hypotheses, self.t, self.kind = hyp[order], t[order], kind
        self._critical = {}

    @classmethod
    def from_statistics(cls, stats_):
        return cls(stats_.hypotheses, stats_.t, stats_.kind)

    def level(self, quantile):
        quantile = float(quantile)
        return abs(2 * quantile - 1) if self.kind == 'central' else max(quantile, 1 - quantile)

    def critical_values(self, quantile):
        """-> the critical value at every tabulated hypothesis [H]"""
        level, n = self.level(quantile), self.t.shape[1]
        if level > 1 - 1.0 / n:
            raise ValueError("quantile %g asks for the level %g of the test statistic: %d toys per hypothesis resolve levels up to "
                             "1 - 1/n = %g only -- more toys are needed" % (quantile, level, n, 1 - 1.0 / n))
        if level not in self._critical:
            self._critical[level] = np.quantile(self.t, level, axis=1, method='higher')
        return self._critical[level]

    def __call__(self, hypothesis, quantile):
        return float(np.interp(float(hypothesis), self.hypotheses, self.critical_values(quantile)))


def neyman_thresholds(lf, target, hypotheses, n_toys, **options):
    """Toy-calibrated critical values for `one_parameter_interval`: `toy_test_statistics` (same arguments and options; its
    `kind` must be the interval's) tabulated as a `ToyThresholds`, e.g.
        table = lf.neyman_thresholds('s0_rate_multiplier', np.linspace(0.5, 4, 16), 1000, kind='upper')
        limit = lf.one_parameter_interval('s0_rate_multiplier', bound=4., kind='upper', t_ppf=table)
    A ToyStatistics at hand (ranks' parts put together, say) becomes a table with ToyThresholds.from_statistics(stats)."""
    return ToyThresholds.from_statistics(toy_test_statistics(lf, target, hypotheses, n_toys, **options))


# ---- goodness of fit ------------------------------------------------------------------------------------------------

def expected_counts_points(lf, points, per_source=False, livetime_days=None):
    """The expected events per bin at P parameter points: points = dict parameter name -> array [P] (scalars broadcast;
    absent parameters take their defaults), as `eval_points` -> mu [P, *bin_shape], or [P, S, *bin_shape] with per_source
    (source order: `source_name_list`; the sum over sources is the total).  Live time, rate multipliers and efficiencies
    enter exactly as in `lf(**params)` (the same host terms); the morph runs on the device (bi_expected_counts), where the
    dense templates lie -- no data are needed.  A point outside the anchor box or with unphysical rates gets nan.
    Also for a prepared source-wise model (bi_sourcewise_expected_counts)."""
    _binned_or_source_wise(lf, 'expected_counts_points')
    z, scale, _ = lf._batch_terms(points, livetime_days)
    mu = lf.ctx.expected_counts(z if z.shape[1] else None, scale, per_source=per_source)
    return mu.reshape(mu.shape[:-1] + tuple(lf.bin_shape))


def expected_counts(lf, per_source=False, livetime_days=None, **params):
    """The expected events per bin at one parameter point -> array of `lf.bin_shape`, or [S, *bin_shape] with per_source:
    the best-fit histogram, the denominator of a pull.  As `expected_counts_points`, with the host terms of the scalar
    call `lf(**params)`; nan outside the anchor box or where the rates are unphysical.  Refused for a source-wise model
    (SourceWiseBinnedLogLikelihood): call `expected_counts_points(lf, points, per_source=)` with one-row arrays there."""
    _binned_for_gof(lf, 'expected_counts')
    _, zs, scale = lf._host_terms(livetime_days, params)
    S = len(lf.source_name_list)
    shape = ((S,) if per_source else ()) + tuple(lf.bin_shape)
    if zs is None:
        return np.full(shape, np.nan)
    return lf.ctx.expected_counts(zs if len(zs) else None, scale[None, :], per_source=per_source)[0].reshape(shape)


def gof_statistics(lf, points=None, datasets=None, livetime_days=None, binning=None, **fixed):
    """Goodness-of-fit statistics of the binned data at P parameter points, summed bin by bin on the device (bi_eval_gof):
        deviance = 2 sum_b [mu_b - n_b - n_b log(mu_b / n_b)]     (the likelihood ratio against the saturated model, Baker-Cousins)
        pearson  =   sum_b (n_b - mu_b)^2 / mu_b
    with an empty bin contributing 2 mu_b and mu_b.  points: dict parameter name -> array [P] (as `eval_points`); fixed
    (kwargs): parameters at one value everywhere; datasets: the dataset of every point [P], e.g. np.arange(T) with the fitted
    values of `bestfit_toys` (None: dataset 0).
    -> dict(deviance [P], pearson [P], n_bins, n_events [P] (the events of every point's dataset), status [P]).
    PRIORS ARE NOT PART OF EITHER STATISTIC: both are statements about the data term only, whatever constraint terms the
    likelihood carries.  A point outside the anchor box or with unphysical rates gives +inf in both; so does a point where
    the likelihood is -inf (an event in a bin where nothing is expected), and both are nan where it is nan.

    binning: a `CoarseBinning` -- both statistics are then formed over its C cells, from the expectation and the counts summed
    over the fine bins of every cell on the device (bi_expected_coarse, bi_coarse_counts) and the same per-cell forms
    (`coarse_statistics`); n_bins is C, and n_events counts the events inside the cells.  THE STATISTIC IS THEN A STATEMENT
    ABOUT THE COARSE CELLS ONLY: what happens inside a cell, or in fine bins that belong to no cell, is invisible to it -- in
    particular an event in a fine bin with no expectation no longer forces +inf, unless its whole cell expects nothing.
    A prepared source-wise model is taken too (bi_eval_sourcewise_gof; with `binning` bi_sourcewise_expected_coarse and
    bi_sourcewise_coarse_counts)."""
    _binned_or_source_wise(lf, 'gof_statistics', binning)
    if not lf.is_data_set:
        raise NotPreparedException("gof_statistics requires you to first set the data using set_data()")
    pts = dict(fixed)
    pts.update(points or {})
    z, scale, _ = lf._batch_terms(pts, livetime_days)
    if datasets is not None:
        datasets = np.atleast_1d(np.asarray(datasets, dtype=np.int64))
        P = max(len(z), len(datasets))
        z, scale = np.broadcast_to(z, (P, z.shape[1])), np.broadcast_to(scale, (P, scale.shape[1]))
        datasets = np.broadcast_to(datasets, (P,))
    if binning is not None:
        return _gof_statistics_coarse(lf, binning, z, scale, datasets)
    half, pearson, st = lf.ctx.eval_gof(z if z.shape[1] else None, scale, datasets)
    ds = np.zeros(len(half), dtype=np.int64) if datasets is None else datasets
    totals = {int(t): float(lf.ctx.download_counts(int(t)).sum()) for t in np.unique(ds) if 0 <= t < lf.ctx.T}
    return dict(deviance=2.0 * half, pearson=pearson, n_bins=int(np.prod(lf.bin_shape, dtype=np.int64)),
                n_events=np.array([totals.get(int(t), np.nan) for t in ds]), status=st)


def _gof_statistics_coarse(lf, binning, z, scale, datasets):
    """`gof_statistics` over the cells of `binning`: z [P, d], scale [P, S] and datasets [P] (or None) as it prepared them"""
    _prepared(lf, binning, 'gof_statistics')
    mu, st = lf.ctx.expected_coarse(binning.n_cells, z if z.shape[1] else None, scale)
    ds = np.zeros(len(mu), dtype=np.int64) if datasets is None else np.asarray(datasets, dtype=np.int64)
    T = int(lf.ctx.T)
    known = np.unique(ds[(ds >= 0) & (ds < T)])
    n_of = np.full((len(mu), binning.n_cells), np.nan)
    if len(known):
        table = lf.ctx.coarse_counts(binning.n_cells, known)
        inside = np.isin(ds, known)
        n_of[inside] = table[np.searchsorted(known, ds[inside])]
    st = np.where((ds < 0) | (ds >= T), st | 16, st).astype(np.int32)       # (BI_ST_BAD_DATASET, as bi_eval_gof reports it)
    deviance, pearson = coarse_statistics(n_of, mu)
    dead = st != 0
    deviance[dead] = pearson[dead] = np.inf
    return dict(deviance=deviance, pearson=pearson, n_bins=int(binning.n_cells), n_events=n_of.sum(axis=1), status=st)


def toy_p_value(observed, toys, failed=None):
    """The p-value of `observed` among the toys' statistics: (1 + #{toys >= observed}) / (n + 1) -- ties count as >=, and so
    do toys whose fit failed (`failed` [n], bool) and toys whose statistic is nan: the conservative side, never dropped."""
    toys = np.atleast_1d(np.asarray(toys, dtype=float))
    if toys.ndim != 1 or len(toys) == 0:
        raise ValueError("toy_p_value needs the statistics of at least one toy")
    above = ~(toys < float(observed))
    if failed is not None:
        failed = np.asarray(failed, dtype=bool)
        if failed.shape != toys.shape:
            raise ValueError("failed must have one flag per toy")
        above = above | failed
    return (1.0 + np.count_nonzero(above)) / (len(toys) + 1.0)


class GofResult:
    """What `goodness_of_fit` returns: statistic ('deviance' or 'pearson'), observed (its value for the data at their best
    fit), toys [n] (its value for every toy at that toy's own fit), p_value = (1 + #{toys >= observed}) / (n + 1),
    p_value_chi2 = chi2.sf(observed, ndof) with ndof = n_bins - n_floating -- ASYMPTOTIC: unreliable with sparse bins (few
    expected events per bin), where the toys are the answer --, best (OrderedDict name -> fitted value of the data),
    toy_best (OrderedDict name -> fitted values [n]), failed [n] and n_failed: the toys whose fit failed; they count as >=
    observed in p_value and are reported, never dropped."""

    def __init__(self, statistic, observed, toys, failed, ndof, best, toy_best):
        self.statistic, self.observed, self.toys = statistic, float(observed), np.asarray(toys, dtype=float)
        self.failed = np.asarray(failed, dtype=bool)
        self.n_failed = int(np.count_nonzero(self.failed))
        self.ndof, self.best, self.toy_best = int(ndof), best, toy_best
        self.p_value = toy_p_value(self.observed, self.toys, self.failed)
        self.p_value_chi2 = float(stats.chi2.sf(self.observed, self.ndof)) if self.ndof > 0 else float('nan')


def goodness_of_fit(lf, n_toys=1000, statistic='deviance', chunk=256, seed=0, first_toy=0, fit_options=None, livetime_days=None,
                    binning=None, **fixed):
    """Does the fitted model describe the data?  The goodness-of-fit statistic ('deviance' or 'pearson', see
    `gof_statistics`) of the data at their best fit, and its p-value from toys that are treated like the data:
      1. the data are fitted (`bestfit_batched`; `fixed` parameters stay fixed, fit_options go to the engine);
      2. the observed statistic is evaluated at that fit;
      3. `n_toys` toys are drawn at the fitted values (`simulate_toys`), `chunk` at a time; toy j is toy first_toy + j of the
         seed's ensemble, so the result does not depend on `chunk` (as `toy_mc_fits`);
      4. every toy is fitted (`bestfit_toys`, the same options);
      5. every toy's statistic is evaluated at its own fit.
    -> GofResult.  Priors shape the fits but are no part of the statistic.  p_value_chi2 is the asymptotic reading
    chi2.sf(observed, n_bins - n_floating); with sparse bins it is unreliable and p_value is the number to quote.
    Afterwards the likelihood has its own data back (as after `toy_test_statistics`).

    binning: a `CoarseBinning` -- the data and every toy are still FITTED on the fine bins, but the statistic of steps 2 and 5
    is formed over the cells of the binning (`gof_statistics(..., binning=)`: a statement about the coarse cells only), where
    a test on ~10^4 events has power that it lacks on 10^6 fine bins; ndof = n_cells - n_floating.
    A prepared source-wise model is taken too, with or without `binning` (its toys: `simulate_toys_points` with one truth)."""
    _binned_or_source_wise(lf, 'goodness_of_fit', binning)
    if statistic not in ('deviance', 'pearson'):
        raise ValueError("statistic must be 'deviance' or 'pearson'")
    n, chunk = int(n_toys), max(int(chunk), 1)
    if n < 1:
        raise ValueError("goodness_of_fit needs at least one toy")
    fit_options = dict(fit_options or {})
    ctx = lf.ctx
    try:
        b, _ = bestfit_batched(lf, livetime_days=livetime_days, **fit_options, **fixed)
        best = OrderedDict((k, float(v[0])) for k, v in b.items())
    except NoOpimizationNecessary:
        best = OrderedDict()
    truth = dict(fixed, **best)
    observed = float(gof_statistics(lf, livetime_days=livetime_days, binning=binning, **truth)[statistic][0])
    n_bins = int(np.prod(lf.bin_shape, dtype=np.int64)) if binning is None else int(binning.n_cells)
    restore = _resident_data(lf, ctx)
    toys, failed = np.empty(n), np.zeros(n, dtype=bool)
    toy_best = OrderedDict((k, np.empty(n)) for k in best)
    try:
        for t0 in range(0, n, chunk):
            m = min(chunk, n - t0)
            ctx.set_param('toy_offset', int(first_toy) + t0)
            _simulate_toys_at(lf, m, seed, livetime_days, truth)
            fitted = {}
            if best:
                fitted, _, info = bestfit_toys(lf, livetime_days=livetime_days, return_info=True, **fit_options, **fixed)
                failed[t0:t0 + m] = info['failed']
                for k, v in fitted.items():
                    toy_best[k][t0:t0 + m] = v
            toys[t0:t0 + m] = gof_statistics(lf, points=fitted, datasets=np.arange(m), livetime_days=livetime_days, binning=binning,
                                             **fixed)[statistic]
    finally:
        ctx.set_param('toy_offset', 0)
        if restore is not None:
            restore()
    return GofResult(statistic, observed, toys, failed, n_bins - len(best), best, toy_best)


def _covariance(lf, values, livetime_days=None, datasets=None, log_rates=False, **fixed):
    """-> (names of the floating parameters, covariance [P, F, F], scalar input?) -- see `hesse`."""
    if not hasattr(lf, 'values_gradients_hessians'):
        raise NotImplementedError("hesse needs a likelihood with values_gradients_hessians")
    floating = list(values.keys())
    cols = {k: np.atleast_1d(np.asarray(v, dtype=float)) for k, v in values.items()}
    scalar = all(np.ndim(v) == 0 for v in values.values()) and datasets is None
    P = max([len(c) for c in cols.values()] + [1 if datasets is None else len(np.atleast_1d(datasets))])
    points = {k: np.broadcast_to(c, (P,)) for k, c in cols.items()}
    points.update((k, np.broadcast_to(np.asarray(v, dtype=float), (P,))) for k, v in fixed.items())
    options = {} if datasets is None else dict(dataset=np.broadcast_to(np.asarray(datasets, dtype=np.int64), (P,)))
    ll, grads, names, H = lf.values_gradients_hessians(points, livetime_days=livetime_days, **options)
    missing = [k for k in floating if k not in names]
    if missing:
        raise ValueError("not parameters of the likelihood: %s" % ', '.join(missing))
    order = [k for k in names if k in floating]
    idx = np.array([names.index(k) for k in order], dtype=int)
    g = np.stack([grads[k] for k in order], axis=1) if order else np.zeros((P, 0))
    Hf = H[:, idx[:, None], idx[None, :]]
    if log_rates:
        g, Hf = to_log10(g, Hf, np.stack([points[k] for k in order], axis=1), [k.endswith('_rate_multiplier') for k in order])
    F = len(order)
    cov = np.full((P, F, F), np.nan)
    ok = np.isfinite(ll) & np.all(np.isfinite(Hf), axis=(1, 2))
    for p in np.flatnonzero(ok):
        try:
            L = np.linalg.cholesky(-Hf[p])
        except np.linalg.LinAlgError:
            ok[p] = False
            continue
        Li = np.linalg.inv(L)
        cov[p] = Li.T @ Li
    if not ok.all():
        warnings.warn("hesse: -H is not positive definite (or ll = -inf) at %d of %d points: their covariance is nan"
                      % (int(np.count_nonzero(~ok)), P), RuntimeWarning, stacklevel=3)
    return order, cov, scalar


def hesse(lf, values, livetime_days=None, datasets=None, information='observed', **fixed):
    """Covariance of the floating parameters at fitted values: (-H)^-1, H the Hessian of the log likelihood from the device
    (`lf.values_gradients_hessians`, one call for all points).

    values: the first return of a `bestfit_*` -- dict name -> scalar, or -> array [P] (an ensemble of fits); the parameters
    named there float, `fixed` holds others at given values.  datasets: the dataset of every point, e.g. np.arange(T) for
    the T toys fitted by `bestfit_toys`.  -> (names [F], covariance [F, F] for scalar values, [P, F, F] for arrays).  The
    covariance is nan (with one warning per call) where -H is not positive definite or ll = -inf.  On an anchor the
    Hessian is that of the cell the point is assigned to.

    information='expected': the inverse of the Fisher information at `values` instead (`expected_covariance`'s, all points
    in one device call; the data and `datasets` are not looked at) -- positive semi-definite by construction, the
    alternative where -H of sparse data or of a fit that ended on a kink of the morph is not positive definite."""
    if information == 'expected':
        cols = {k: np.atleast_1d(np.asarray(v, dtype=float)) for k, v in values.items()}
        scalar = all(np.ndim(v) == 0 for v in values.values()) and datasets is None
        P = max([len(c) for c in cols.values()] + [1 if datasets is None else len(np.atleast_1d(datasets))])
        points = {k: np.broadcast_to(c, (P,)) for k, c in cols.items()}
        points.update((k, np.broadcast_to(np.asarray(v, dtype=float), (P,))) for k, v in fixed.items())
        names, cov = _expected_covariance_points(lf, points, list(values.keys()), livetime_days, True, False, 'hesse')
        return names, (cov[0] if scalar else cov)
    if information != 'observed':
        raise ValueError("hesse: information = %r (it is 'observed' or 'expected')" % (information,))
    names, cov, scalar = _covariance(lf, values, livetime_days=livetime_days, datasets=datasets, **fixed)
    return names, (cov[0] if scalar else cov)


# ---- expected (Fisher) information ------------------------------------------------------------------------------------

def _binned_for_fisher(lf, what):
    """The gate of the expected information: a `BinnedLogLikelihood` without Beeston-Barlow (`_binned_for_gof`), or a prepared
    source-wise model (its context has eval_fisher; everything else behind `_binned_for_gof` keeps refusing it)."""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if isinstance(lf, SourceWiseBinnedLogLikelihood):
        if not lf.is_prepared:
            raise NotPreparedException("%s requires you to first prepare the likelihood function using prepare()" % what)
        return lf
    return _binned_for_gof(lf, what)


def fisher_information_points(lf, points, livetime_days=None, priors=True):
    """The expected (Fisher) information of the binned likelihood at P truths, before any data exist:
        I_qr = sum_b d_q mu_b d_r mu_b / mu_b    (- the curvature of the log priors on the diagonal, unless priors=False)
    over every registered rate multiplier, then every shape parameter.  points = dict parameter name -> array [P] (as
    `eval_points`; absent parameters at their defaults).  -> (names [F], I [P, F, F], unbounded [P, F] bool).  The sum over
    the bins runs on the device (bi_eval_fisher: one pass over the corner rows of every truth, no data needed); live time,
    efficiencies and shape parameters that double as efficiencies enter by the chain rule of `values_gradients_hessians`
    (`chain_rule_information`), priors through `prior_derivatives`.  A bin that expects nothing at the truth but would with
    another value of a parameter (a signal multiplier of 0, a truth on an anchor) holds unbounded information on it: it is
    left out of I and the parameter is flagged.  A truth outside the anchor box, with unphysical rates or with a negative
    expectation gives a nan matrix.  On an anchor I is that of the cell the point is assigned to."""
    _binned_for_fisher(lf, 'fisher_information_points')
    z, scale, _ = lf._batch_terms(points, livetime_days)
    P = len(z)
    info, _, unb, _ = lf.ctx.eval_fisher(z if z.shape[1] else None, scale)
    mult, L, eff, eff_axis, rate_sources = lf._chain_rule_terms(points, P, livetime_days)
    curvature = None
    if priors:
        nr = len(rate_sources)
        curvature = np.zeros((P, nr + z.shape[1]))
        for j, s in enumerate(rate_sources):
            lp = lf.rate_parameters[lf.source_name_list[s]]
            if lp is not None:
                curvature[:, j] = prior_derivatives(lp, mult[:, s])[1]
        for i, (_, (_, lp, _)) in enumerate(lf.shape_parameters.items()):
            if lp is not None:
                curvature[:, nr + i] = prior_derivatives(lp, z[:, i])[1]
    out = chain_rule_information(info, mult, L, eff, eff_axis, rate_sources, curvature)
    return lf._parameter_names(), out, chain_rule_unbounded(unb, mult, L, eff, eff_axis, rate_sources)


def fisher_information(lf, livetime_days=None, priors=True, **truth):
    """`fisher_information_points` at one truth (parameter values; absent parameters at their defaults) ->
    (names [F], I [F, F], unbounded [F] bool)."""
    names, info, unb = fisher_information_points(lf, {k: np.array([v], dtype=float) for k, v in truth.items()},
                                                 livetime_days=livetime_days, priors=priors)
    return names, info[0], unb[0]


def _expected_covariance_points(lf, points, floating, livetime_days, priors, log_rates, what):
    """-> (names of the floating parameters, covariance [P, F, F]) from the Fisher information at `points`; one warning."""
    names, info, unb = fisher_information_points(lf, points, livetime_days=livetime_days, priors=priors)
    floating = names if floating is None else list(floating)
    missing = [k for k in floating if k not in names]
    if missing:
        raise ValueError("not parameters of the likelihood: %s" % ', '.join(missing))
    order = [k for k in names if k in floating]
    idx = np.array([names.index(k) for k in order], dtype=int)
    If = info[:, idx[:, None], idx[None, :]]
    uf = unb[:, idx]
    if log_rates:            # y = log10 x: dx / dy = x ln 10 on both sides (no second-order term: the expected score is zero)
        P = len(info)
        x = np.stack([np.broadcast_to(np.asarray(points.get(k, 1.0), dtype=float), (P,)) * np.log(10.0) if k.endswith('_rate_multiplier')
                      else np.ones(P) for k in order], axis=1) if order else np.zeros((P, 0))
        If = If * x[:, :, None] * x[:, None, :]
    cov = covariance_from_information(If, uf)
    bad = ~np.all(np.isfinite(cov), axis=(1, 2))
    if uf.any() or bad.any():
        said = []
        if uf.any():
            said.append("unbounded information on %s at %d of %d points (bins that expect nothing there but would with another value: "
                        "variance 0)" % (', '.join(k for k, u in zip(order, uf.any(axis=0)) if u), int(np.count_nonzero(uf.any(axis=1))), len(cov)))
        if bad.any():
            said.append("the information is singular or nan at %d of %d points: their covariance is nan" % (int(np.count_nonzero(bad)), len(cov)))
        warnings.warn("%s: %s" % (what, '; '.join(said)), RuntimeWarning, stacklevel=3)
    return order, cov


def expected_covariance(lf, floating=None, livetime_days=None, priors=True, rates_in_log_space=False, **truth):
    """The expected covariance of the parameters at a truth, before any data exist: the inverse of the Fisher information
    (`fisher_information`) -> (names [F], covariance [F, F]), `hesse`'s format.  floating: the names that float (default:
    every registered parameter); the others are held at their truth -- their rows and columns are struck before the
    inversion.  A parameter with unbounded information gets variance 0 (`covariance_from_information`); the covariance is nan
    where the floating block is singular.  Either issues one warning.  rates_in_log_space: rate multipliers as log10 values,
    as `bestfit_minuit` reports them."""
    order, cov = _expected_covariance_points(lf, {k: np.array([v], dtype=float) for k, v in truth.items()}, floating, livetime_days,
                                             priors, rates_in_log_space, 'expected_covariance')
    return order, cov[0]


def expected_errors(lf, floating=None, livetime_days=None, priors=True, rates_in_log_space=False, **truth):
    """The expected standard deviations at a truth -> OrderedDict name -> sigma: the square roots of the diagonal of
    `expected_covariance` (same arguments)."""
    order, cov = _expected_covariance_points(lf, {k: np.array([v], dtype=float) for k, v in truth.items()}, floating, livetime_days,
                                             priors, rates_in_log_space, 'expected_errors')
    return OrderedDict(zip(order, np.sqrt(np.diag(cov[0]))))


_MINUIT_DISPLAY_OPTIONS = ('print_level', 'pedantic', 'errordef')


def bestfit_minuit(lf, minimize_kwargs=None, rates_in_log_space=False, **kwargs):
    """The reference's `bestfit_minuit` (blueice/inference.py:181-244) without iminuit: -> ({name: value, name + '_error':
    sigma}, max log likelihood).  Values are `bestfit_device`'s (the batched engine); sigma = sqrt(diag((-H)^-1)) from the
    device Hessian -- MIGRAD's parabolic errors at errordef = 0.5.  With rates_in_log_space=True rate multipliers are
    reported as log10 values with the errors of those, as the reference's Minuit in log space does.  minimize_kwargs: the
    Minuit display options print_level, pedantic and errordef are accepted and ignored, any other key is a ValueError.
    kwargs: parameters held fixed (and `guess`), as `bestfit_scipy`.  Nothing floating: ({}, lf(**kwargs))."""
    unknown = sorted(set(minimize_kwargs or {}) - set(_MINUIT_DISPLAY_OPTIONS))
    if unknown:
        raise ValueError("bestfit_minuit: unsupported minimize_kwargs %s (only %s are accepted, and ignored)"
                         % (', '.join(unknown), ', '.join(_MINUIT_DISPLAY_OPTIONS)))
    guess = kwargs.pop('guess', None)
    fixed = {k: v for k, v in kwargs.items() if k != 'livetime_days'}
    floating = ['%s_rate_multiplier' % s for s in lf.rate_parameters] + list(lf.shape_parameters)
    if not [k for k in floating if k not in fixed]:
        return {}, lf(**kwargs)
    best, ll = bestfit_device(lf, guess=guess, **kwargs)
    if not best:
        return {}, ll
    names, cov, _ = _covariance(lf, best, livetime_days=kwargs.get('livetime_days'), log_rates=rates_in_log_space, **fixed)
    err = np.sqrt(np.diag(cov[0]))
    result = OrderedDict()
    for k, v in best.items():
        result[k] = float(np.log10(v)) if rates_in_log_space and k.endswith('_rate_multiplier') else float(v)
    for k, e in zip(names, err):
        result[k + '_error'] = float(e)
    return result, float(ll)


def bestfit_emcee(ll, quiet=False, return_errors=False, return_samples=False, n_walkers=40, n_steps=200, n_burn_in=100,
                  n_threads=1, seed=0, **kwargs):
    """The reference's `bestfit_emcee` (blueice/inference.py:254-321) without emcee: `sample_posterior` runs the ensemble
    (the stretch move emcee defaults to; the reference's start, guess * U(0.95, 1.05) per walker) and the point estimate is
    read off the chain the way the reference's code does -- `n_steps` steps are run, the first `n_burn_in` of them dropped.
    -> ({name: posterior median}, ll at the medians)
       [, {name: half the width of the central 68.27 % interval} with return_errors]
       [, samples [-1, F], walker by walker, with return_samples].
    quiet=False prints the mean acceptance fraction and, when `corner` can be imported, draws its corner plot of the whole
    chain.  n_threads is accepted and ignored (the walkers of a half-step are one device batch); seed: the random stream
    (extension).  kwargs: `guess` and parameters held fixed, as `make_objective`; `engine`, `p0`, `a` go to
    `sample_posterior`; `livetime_days` goes to the sampler and to the final likelihood call.  One dataset only:
    `datasets` / `first_ensemble` belong to `sample_posterior`."""
    for key in ('datasets', 'first_ensemble'):
        if key in kwargs:
            raise ValueError("bestfit_emcee fits one dataset: %s is an option of sample_posterior" % key)
    sampler_only = {k: kwargs.pop(k) for k in ('engine', 'p0', 'a') if k in kwargs}
    run = sample_posterior(ll, n_walkers=n_walkers, n_steps=n_steps, seed=seed, **sampler_only, **kwargs)
    kept = run.flat(discard=n_burn_in)                                 # [W * (n_steps - n_burn_in), F]
    if not quiet:
        print("Mean acceptance fraction: %.3f" % float(run.acceptance_fraction.mean()))
        try:
            import corner
        except ImportError:
            corner = None
        if corner is not None:
            from matplotlib import pyplot
            corner.corner(run.flat(), labels=run.names, show_titles=True, range=[0.99 for _ in run.names])
            pyplot.show()
    # central 68.27 % interval and median per parameter, in one pass over the kept samples
    one_sigma = float(stats.norm.cdf(1.0) - stats.norm.cdf(-1.0))
    q_lo, q_mid, q_hi = np.quantile(kept, [0.5 - one_sigma / 2, 0.5, 0.5 + one_sigma / 2], axis=0)
    medians = OrderedDict(zip(run.names, q_mid))
    held = {k: v for k, v in kwargs.items() if k != 'guess'}
    at_median = ll(**held, **medians)
    if return_errors:
        return medians, at_median, OrderedDict(zip(run.names, 0.5 * (q_hi - q_lo)))
    if return_samples:
        return medians, at_median, kept
    return medians, at_median


def _first_crossing(tfun, a, b, xtol=1e-11, points_per_round=16, max_rounds=12):
    """The root of t between a and b that lies nearest to a, by rounds of batched evaluations: every round evaluates a
    fan of hypotheses inside the current bracket in ONE call of tfun(h [n]) -> t [n] -- uniformly spaced at first, then
    half of them clustered around the secant estimate (t is smooth) -- and keeps the first sign change seen from a.
    Like brentq, raises ValueError when t(a) and t(b) have the same sign."""
    ta, tb = tfun(np.array([a, b], dtype=float))
    if ta == 0:
        return float(a)
    if tb == 0:
        return float(b)
    if not np.isfinite(ta) or not np.isfinite(tb) or np.sign(ta) == np.sign(tb):
        raise ValueError("f(a) and f(b) must have different signs")
    xs, ts = np.array([a, b], dtype=float), np.array([ta, tb], dtype=float)
    K = points_per_round
    for rnd in range(max_rounds):
        (lo, hi), (tl, th) = xs, ts
        if abs(hi - lo) <= xtol * max(1.0, abs(lo), abs(hi)):
            break
        fan = np.linspace(lo, hi, K + 2)[1:-1]
        if rnd >= 1:
            secant = lo - tl * (hi - lo) / (th - tl)
            steps = abs(hi - lo) * 0.5 ** np.arange(3, 3 + 3 * (K // 4), 3)
            near = secant + np.concatenate([-steps, [0.0], steps])
            near = near[(near > min(lo, hi)) & (near < max(lo, hi))]
            fan = np.unique(np.concatenate([np.linspace(lo, hi, K // 2 + 2)[1:-1], near]))
            if hi < lo:
                fan = fan[::-1]
        allx = np.concatenate([[lo], fan, [hi]])
        allt = np.concatenate([[tl], tfun(fan), [th]])
        k = np.flatnonzero(np.sign(allt[1:]) != np.sign(allt[0]))[0]          # first sign change seen from a
        xs, ts = allx[k:k + 2], allt[k:k + 2]
        if ts[1] == 0:
            return float(xs[1])
    (lo, hi), (tl, th) = xs, ts
    return float(lo - tl * (hi - lo) / (th - tl))


# options of bestfit_scipy that the reference's callers pass through `**kwargs` of the scan / interval drivers
# (blueice/inference.py:332-443 forward them to the fit routine) -- they are NOT fixed parameters
_FIT_ROUTINE_OPTIONS = ('minimize_kwargs', 'rates_in_log_space', 'pass_bounds_to_minimizer', 'use_gradient', 'batch_stencil',
                        'guess')


def _takes_fit_routine_options(kwargs):
    """True when the caller handed options of the fit routine along with the fixed parameters: those calls keep the
    reference's sequential loop over `bestfit_scipy(lf, **kwargs)`, which understands them."""
    return any(k in kwargs for k in _FIT_ROUTINE_OPTIONS)


def one_parameter_interval(lf, target, bound, confidence_level=0.9, kind='upper', bestfit_routine=None, fit_options=None,
                           t_ppf=None, **kwargs):
    """Profile-likelihood interval on parameter `target` (reference: blueice/inference.py:332-389).
    kind 'upper' / 'lower': `bound` is the far end of the line search; 'central': a 2-tuple.
    The test statistic 2 (max logL - logL profiled at the hypothesis) is compared with
    norm.ppf(quantile)**2 (Wilks) or with t_ppf(hypothesis, quantile); the crossing is the one the reference's brentq
    search finds.  With a likelihood that evaluates batches (and no bestfit_routine of the caller's) the search runs on
    the batched profile-fit engine: every round profiles a fan of hypotheses in lock-step on the device (a handful of
    rounds of ~16 fits, each a few dozen device calls) instead of brentq's chain of nested sequential fits (3 387 scalar
    likelihood calls per limit in SURVEY.md's probe); otherwise the reference's loop.  fit_options: dict of options of the
    batched engine (`bestfit_batched`: multi_start='cells', gtol, ...).  `neyman_thresholds` makes a t_ppf from toys."""
    fit_options = dict(fit_options or {})
    if target is None:
        target = lf.source_list[-1] + '_rate_multiplier'
    # (options of bestfit_scipy among the kwargs -- minimize_kwargs, pass_bounds_to_minimizer, ... -- go where the
    # reference sends them: to the fit routine, point by point)
    batched = bestfit_routine is None and supports_batched_fits(lf) and not _takes_fit_routine_options(kwargs)
    fit = bestfit_routine or bestfit_scipy
    if batched:
        try:
            best, ll = bestfit_batched(lf, **fit_options, **kwargs)
            best, max_ll = {k: float(v[0]) for k, v in best.items()}, float(ll[0])
        except NoOpimizationNecessary:
            batched = False
    if not batched:
        best, max_ll = fit(lf, **kwargs)
    global_best = best[target]

    def critical_of(hypothesis, quantile):
        return stats.norm.ppf(quantile) ** 2 if t_ppf is None else t_ppf(hypothesis, quantile)

    def one_sided_ok(hypothesis):
        return (kind == 'upper' and hypothesis <= global_best) or (kind == 'lower' and hypothesis >= global_best)

    def t(hypothesis, quantile):
        critical = critical_of(hypothesis, quantile)
        if one_sided_ok(hypothesis):
            return 0 - critical
        _, ll = fit(lf, **dict(kwargs, **{target: hypothesis}))
        return 2 * (max_ll - ll) - critical

    def t_batched(quantile):
        nuisances = [k for k in best if k != target]

        def tfun(hs):
            hs = np.asarray(hs, dtype=float)
            crit = np.array([critical_of(h, quantile) for h in hs])
            out = 0.0 - crit
            need = np.array([not one_sided_ok(h) for h in hs])
            if np.any(need):
                if nuisances:                       # every hypothesis starts where the reference starts AND at the global best fit's nuisances
                    _, ll = bestfit_batched(lf, points={target: hs[need]}, also_from=[{k: best[k] for k in nuisances}], **fit_options, **kwargs)
                else:                               # nothing left to profile: plain evaluations
                    ll = np.asarray(lf.eval_points(dict(kwargs, **{target: hs[need]})))
                out[need] = 2 * (max_ll - ll) - crit[need]
            return out
        return tfun

    def search(a, b, quantile):
        if batched:
            return _first_crossing(t_batched(quantile), a, b)
        return brentq(t, a, b, args=(quantile,))

    if kind == 'central':
        return (search(bound[0], global_best, (1 - confidence_level) / 2),
                search(global_best, bound[1], 1 - (1 - confidence_level) / 2))
    if kind == 'lower':
        return search(bound, global_best, 1 - confidence_level)
    if kind == 'upper':
        return search(global_best, bound, confidence_level)
    raise ValueError("kind must be 'upper', 'lower' or 'central'")


def likelihood_ratio_scan(lf, *space, bestfit_routine=None, fit_options=None, **kwargs):
    """-log likelihood ratio over a 1-d or 2-d grid of parameter values: the numbers behind the reference's
    `plot_likelihood_ratio` (blueice/inference.py:392-443) without the plotting.
    space: (name, values) tuples.  Parameters given in kwargs are fixed, all others are fitted at every grid
    point.  When nothing is left to fit the whole grid is ONE batched device call (`lf.eval_points`); with floating
    nuisances the grid points are profiled together on the batched fit engine (blueice_amd.profile: one device call per
    optimiser iteration over the whole grid) -- unless the caller brings a `bestfit_routine`, which is then run point by
    point as the reference does.  Returns an array of shape [len(values_0)(, len(values_1))], best point = 0."""
    if not 1 <= len(space) <= 2:
        raise ValueError("Can't handle %d dimensions" % len(space))
    names = [n for n, _ in space]
    grids = np.meshgrid(*[np.asarray(v, dtype=float) for _, v in space], indexing='ij')
    floating = [p + '_rate_multiplier' for p in lf.rate_parameters if p + '_rate_multiplier' not in kwargs] + \
               [p for p in lf.shape_parameters if p not in kwargs]
    floating = [p for p in floating if p not in names]
    pts = {n: g.ravel() for n, g in zip(names, grids)}
    routine_options = _takes_fit_routine_options(kwargs)
    if not floating and hasattr(lf, 'eval_points'):
        pts.update({k: v for k, v in kwargs.items() if k not in _FIT_ROUTINE_OPTIONS})
        ll = np.asarray(lf.eval_points(pts)).reshape(grids[0].shape)
    elif floating and bestfit_routine is None and supports_batched_fits(lf) and not routine_options:
        ll = bestfit_batched(lf, points=pts, **(fit_options or {}), **kwargs)[1].reshape(grids[0].shape)
    else:
        fit = bestfit_routine or bestfit_scipy
        ll = np.empty(grids[0].shape)
        for idx in np.ndindex(*grids[0].shape):
            ll[idx] = fit(lf, **dict(kwargs, **{n: float(g[idx]) for n, g in zip(names, grids)}))[1]
    return np.nanmax(ll) - ll


# ---- expected results from the Asimov dataset ------------------------------------------------------------------------

def _asimov_truth(lf, target, truth):
    """-> (truth dict with the target in it, the target's value there); default: target = 0, everything else at its default"""
    truth = {target: 0.0} if truth is None else dict(truth)
    if target not in truth:
        if target.endswith('_rate_multiplier'):
            truth[target] = 1.0
        else:
            truth[target] = lf._kwargs_to_settings()[1][target]
    return truth, float(truth[target])


def _asimov_fits(view, target, hypotheses, truth, fit_options, livetime_days, fixed):
    """-> (max over everything [scalar], max at every hypothesis of the target [H]) of the view's value -D + prior"""
    options = dict(fit_options or {})
    if livetime_days is not None:
        options['livetime_days'] = livetime_days
    start = {k: v for k, v in truth.items() if k not in fixed}
    free = bestfit_batched(view, also_from=[start], **options, **fixed)[1][0]
    nuisance_start = {k: v for k, v in start.items() if k != target}
    try:
        cond = bestfit_batched(view, points={target: hypotheses}, also_from=[nuisance_start], **options, **fixed)[1]
    except NoOpimizationNecessary:            # nothing left to profile: plain evaluations
        cond = np.asarray(view.eval_points(dict(fixed, **{target: hypotheses}), livetime_days=livetime_days))
    return float(free), np.asarray(cond, dtype=float)


def asimov_test_statistic(lf, target, hypotheses, truth=None, fit_options=None, livetime_days=None, **fixed):
    """The profile-likelihood test statistic of every hypothesis of `target` on the Asimov dataset of `truth`:
        q_A [H] = 2 (min_nu D(h, nu) - min D),     D = half-deviance + (-prior)
    (Cowan, Cranmer, Gross, Vitells: sqrt(q_A) is the median significance with which h is excluded when `truth` holds; for
    truth = the signal hypothesis and h = 0, the median discovery significance).  truth: dict of parameter values (default:
    target = 0, everything else at its default) at which the data are made (`lf.asimov`); fixed (kwargs): parameters held
    fixed in every fit; fit_options: options of `bestfit_batched`.  All hypotheses are profiled in ONE `bestfit_batched` call
    on the view, on the native loop (bi_fit_batched_real); D is summed bin by bin without cancellation, so q_A is good to
    ~1e-10 max(1, D), not to 1e-10 of a log-likelihood.  `lf`'s own data are not touched."""
    hypotheses = np.atleast_1d(np.asarray(hypotheses, dtype=float))
    truth, _ = _asimov_truth(lf, target, truth)
    from .asimov import asimov              # (the module function: it takes a source-wise model too, whose bound name refuses)
    view = asimov(lf, livetime_days=livetime_days, **truth)
    free, cond = _asimov_fits(view, target, hypotheses, truth, fit_options, livetime_days, fixed)
    return 2.0 * (free - cond)


def expected_upper_limit(lf, target, bound, confidence_level=0.9, n_sigma=(-2, -1, 0, 1, 2), truth=None, fit_options=None,
                         livetime_days=None, **fixed):
    """The expected upper limit on `target` and its band from the Asimov dataset of `truth` (default: background only,
    target = 0) -> {N: limit} for every N of n_sigma: the N-sigma expected limit is where sqrt(q_A(mu)) crosses
    Phi^-1(confidence_level) + N, i.e. `one_parameter_interval(view, target, bound, kind='upper', t_ppf=lambda h, q:
    (norm.ppf(q) + N) ** 2)` on the Asimov view; N = 0 is the median.  An N with Phi^-1(confidence_level) + N <= 0 has no
    crossing above the truth and returns the truth's value of the target.  bound: the far end of the search, as
    `one_parameter_interval`."""
    truth, at_truth = _asimov_truth(lf, target, truth)
    from .asimov import asimov              # (the module function: it takes a source-wise model too, whose bound name refuses)
    view = asimov(lf, livetime_days=livetime_days, **truth)
    more = dict(fixed)
    if livetime_days is not None:
        more['livetime_days'] = livetime_days
    out = OrderedDict()
    for n in n_sigma:
        if stats.norm.ppf(confidence_level) + n <= 0:
            out[n] = at_truth
            continue
        out[n] = one_parameter_interval(view, target, bound, confidence_level=confidence_level, kind='upper', fit_options=fit_options,
                                        t_ppf=lambda h, q, n=n: (stats.norm.ppf(q) + n) ** 2, **more)
    return out


def expected_discovery_significance(lf, target, truth, fit_options=None, livetime_days=None, **fixed):
    """The median significance with which target = 0 is rejected when `truth` (dict of parameter values: the signal
    hypothesis) holds: sqrt(q_A(0)) on the Asimov dataset of `truth`."""
    q = asimov_test_statistic(lf, target, [0.0], truth=truth, fit_options=fit_options, livetime_days=livetime_days, **fixed)[0]
    return float(np.sqrt(max(q, 0.0)))


_BESTFIT_ROUTINES = dict(scipy=bestfit_scipy, minuit=bestfit_minuit, emcee=bestfit_emcee, device=bestfit_device)


def plot_likelihood_ratio(lf, *space, vmax=15, bestfit_routine=None, plot_kwargs=None, **kwargs):
    """Draw the -log likelihood ratio over a 1-d or 2-d grid of parameter values with matplotlib (the reference's
    `plot_likelihood_ratio`, blueice/inference.py:392-443, into the current axes): a curve for one (name, values) tuple, a
    colour mesh with its colour bar for two.  vmax: the top of the y axis / colour scale; plot_kwargs go to the curve / mesh;
    parameters in kwargs are fixed, all others are fitted at every grid point -- the numbers are `likelihood_ratio_scan`'s
    (one batched device call, or the batched profile-fit engine), unless a `bestfit_routine` (a callable, or 'scipy' /
    'minuit' / 'emcee' / 'device') asks for the point-by-point loop.  Returns the values drawn (the reference returns
    nothing)."""
    from matplotlib import pyplot
    if isinstance(bestfit_routine, str):
        if bestfit_routine not in _BESTFIT_ROUTINES:
            raise ValueError("unknown bestfit_routine %r" % bestfit_routine)
        bestfit_routine = _BESTFIT_ROUTINES[bestfit_routine]
    ratio = likelihood_ratio_scan(lf, *space, bestfit_routine=bestfit_routine, **kwargs)
    style = dict(plot_kwargs or {})
    axes = pyplot.gca()
    title = "-Log likelihood ratio"
    axis_values = [np.asarray(values, dtype=float) for _, values in space]
    if len(space) == 1:
        axes.plot(axis_values[0], ratio, **style)
        axes.set(xlabel=space[0][0], ylabel=title, xlim=(axis_values[0].min(), axis_values[0].max()), ylim=(0, vmax))
    else:
        # (a mesh over the two axes' values: rows of `ratio` run along the first parameter, which is drawn horizontally)
        mesh = axes.pcolormesh(axis_values[0], axis_values[1], ratio.T, vmax=vmax, shading='nearest', **style)
        axes.figure.colorbar(mesh, ax=axes, label=title)
        axes.set(xlabel=space[0][0], ylabel=space[1][0])
    return ratio
