"""Coarse views of a binned likelihood: projections on one or two analysis dimensions, a rebinned analysis space, a signal box.

`CoarseBinning` is the host specification: a tensor product of groups of adjacent fine bins, one list of boundaries per
analysis dimension.  `expected_coarse` / `expected_coarse_points` return the morphed expectation summed over the cells,
`coarse_counts` the resident data summed the same way -- both reduced on the device (bi_expected_coarse, bi_coarse_counts:
the corner rows of a point are streamed once and summed as they arrive, the fine bins never cross the bus) --, and
`coarse_statistics` forms the deviance and Pearson's chi2 over the cells, which `gof_statistics(..., binning=)` and
`goodness_of_fit(..., binning=)` use (blueice_amd.inference).  `expected_coarse_jacobian` / `_points` add the first
derivatives of every cell in the user's parameters, summed over the cells in the same single pass
(bi_expected_coarse_jacobian); `expected_coarse_band` turns a covariance of the parameters (`hesse`, `expected_covariance`)
into the uncertainty band of a coarse view and the impact of every parameter on it, and `coarse_information` gives the Fisher
information of the likelihood at that binning, cell by cell.  Plain binned likelihoods; a source-wise model
(`SourceWiseBinnedLogLikelihood`) has the binning, the expectation and the counts per cell (bi_sourcewise_expected_coarse,
bi_sourcewise_coarse_counts) and with them the rebinned goodness of fit.  Its derivatives have spellings of their own --
`sourcewise_coarse_jacobian` / `_points` (per source as well), `sourcewise_coarse_band`, `sourcewise_coarse_information`, over
bi_sourcewise_expected_coarse_jacobian, whose device work does not grow with the number of shape parameters -- and the four
grid-model names keep refusing a source-wise model, naming them.

    box = CoarseBinning(lf, keep=['cs1'], rebin={'cs1': 4}, ranges={'cs2': (2.0, 3.5)})
    mu = lf.expected_coarse(box, per_source=True, **best)            # [S, n_cs1 / 4]
    band = np.percentile(lf.expected_coarse_points(box, samples), [16, 50, 84], axis=0)
    mu, sigma, impacts = lf.expected_coarse_band(box, *lf.hesse(best), **best)
"""
from collections import OrderedDict

import numpy as np

from .exceptions import NotPreparedException
from .hessian import user_jacobian

__all__ = ['CoarseBinning', 'expected_coarse', 'expected_coarse_points', 'coarse_counts', 'coarse_statistics',
           'expected_coarse_jacobian', 'expected_coarse_jacobian_points', 'expected_coarse_band', 'coarse_information',
           'propagate_covariance', 'information_per_cell', 'sourcewise_coarse_jacobian', 'sourcewise_coarse_jacobian_points',
           'sourcewise_coarse_band', 'sourcewise_coarse_information']

EDGE_TOLERANCE = 1e-9          # an edge value must lie within this fraction of the bin's width of a fine edge


def _binned_for_gof(lf, what, prepared=True):
    """-> lf if it is a binned likelihood without Beeston-Barlow; NotImplementedError otherwise (before any device work).
    prepared=False: the type alone is checked (a `CoarseBinning` needs the analysis space only, fixed when the likelihood is made)"""
    from .likelihood import BinnedLogLikelihood
    if not isinstance(lf, BinnedLogLikelihood):
        raise NotImplementedError("%s needs a BinnedLogLikelihood: a %s has no bins of its own" % (what, type(lf).__name__))
    if lf.model_statistical_uncertainty_handling is not None:
        raise NotImplementedError("%s is not defined with Beeston-Barlow (model_statistical_uncertainty_handling = %r): the "
                                  "expectation depends on the data" % (what, lf.model_statistical_uncertainty_handling))
    if prepared and not lf.is_prepared:
        if len(lf.shape_parameters):
            raise NotPreparedException("%s requires you to first prepare the likelihood function using prepare()" % what)
        lf.prepare()            # nothing to morph: preparation is trivial
    return lf


def _binned_for_coarse(lf, what, prepared=True, derivatives=False):
    """The gate of the coarse views proper (the binning, the expectation and the counts per cell): what `_binned_for_gof` lets
    through, or a `SourceWiseBinnedLogLikelihood`, whose context has the three calls under the same names
    (bi_sourcewise_set_coarse_binning, bi_sourcewise_expected_coarse, bi_sourcewise_coarse_counts).  derivatives=True: the call
    is one of the grid model's derivative functions, which a source-wise model has under spellings of its own (`_SOURCEWISE_SPELLINGS`).
    `_binned_for_gof` itself keeps refusing the class."""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if not isinstance(lf, SourceWiseBinnedLogLikelihood):
        return _binned_for_gof(lf, what, prepared)
    if derivatives:
        _refuse_sourcewise(lf, what)
    if prepared and not lf.is_prepared:
        raise NotPreparedException("%s requires you to first prepare the likelihood function using prepare()" % what)
    return lf


# the grid model's derivative functions -> what a source-wise model has in their place, and back
_SOURCEWISE_SPELLINGS = {
    'expected_coarse_jacobian_points': 'sourcewise_coarse_jacobian_points(lf, binning, points, per_source=)',
    'expected_coarse_jacobian': 'sourcewise_coarse_jacobian(lf, binning, per_source=, **params)',
    'expected_coarse_band': 'sourcewise_coarse_band(lf, binning, names, covariance, **params)',
    'coarse_information': 'sourcewise_coarse_information(lf, binning, **truth)',
}
_GRID_SPELLINGS = {
    'sourcewise_coarse_jacobian_points': 'expected_coarse_jacobian_points(lf, binning, points)',
    'sourcewise_coarse_jacobian': 'expected_coarse_jacobian(lf, binning, **params)',
    'sourcewise_coarse_band': 'expected_coarse_band(lf, binning, names, covariance, **params)',
    'sourcewise_coarse_information': 'coarse_information(lf, binning, **truth)',
}


def _refuse_sourcewise(lf, what):
    """NotImplementedError for a source-wise model in one of the grid model's derivative functions, naming the spelling that works;
    any other likelihood passes (its own gates follow)"""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if isinstance(lf, SourceWiseBinnedLogLikelihood):
        raise NotImplementedError("%s is the grid model's spelling and is not available for a source-wise model "
                                  "(SourceWiseBinnedLogLikelihood); call blueice_amd.coarse.%s" % (what, _SOURCEWISE_SPELLINGS[what]))


def _sourcewise_prepared(lf, binning, what):
    """The gate of the `sourcewise_coarse_*` functions, before any device work: a prepared `SourceWiseBinnedLogLikelihood`
    (NotImplementedError naming the grid spelling for anything else, NotPreparedException for an unprepared one) and a
    `CoarseBinning` (TypeError), which becomes the binning of the likelihood's context."""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if not isinstance(lf, SourceWiseBinnedLogLikelihood):
        raise NotImplementedError("%s needs a source-wise model (SourceWiseBinnedLogLikelihood), not a %s; for a BinnedLogLikelihood "
                                  "call blueice_amd.coarse.%s" % (what, type(lf).__name__, _GRID_SPELLINGS[what]))
    return _prepared(lf, binning, what)


def _edge_index(name, fine, value):
    """-> the index of the fine edge `value` coincides with; ValueError if there is none"""
    value = float(value)
    i = int(np.argmin(np.abs(fine - value)))
    widths = np.diff(fine)
    width = min(widths[max(i - 1, 0)], widths[min(i, len(widths) - 1)])
    if not abs(fine[i] - value) <= EDGE_TOLERANCE * width:
        raise ValueError("%r: %r is not an edge of the fine binning (nearest: %r)" % (name, value, float(fine[i])))
    return i


class CoarseBinning:
    """A coarse binning of the analysis space of a plain `BinnedLogLikelihood` or a `SourceWiseBinnedLogLikelihood`.

    keep    names of the analysis dimensions that stay as axes of the result, in the order of the analysis space; the others
            are summed over.  Default: all.
    rebin   name -> int n: merge n adjacent fine bins, starting at the first bin of the range, the last group possibly
            shorter; or name -> ascending edge values, each of which must coincide with a fine edge to within 1e-9 of that
            bin's width (ValueError otherwise).  Kept dimensions only.
    ranges  name -> (lo, hi) edge values, checked the same way: fine bins outside belong to no cell.  For kept and summed
            dimensions alike -- a signal box is one cell.

    dims, shape, edges (per kept dimension), n_cells; groups: per ANALYSIS dimension the ascending fine-bin boundaries
    e_0 < ... < e_m (group g holds the fine bins e_g <= i < e_g+1; a summed dimension has one group); fine_shape.
    `bin_map()` is the executable specification: fine flat index -> coarse flat index, both in C order."""

    def __init__(self, lf, keep=None, rebin=None, ranges=None):
        _binned_for_coarse(lf, 'CoarseBinning', prepared=False)
        space = [(str(n), np.asarray(e, dtype=float)) for n, e in lf.base_model.config['analysis_space']]
        names = [n for n, _ in space]
        keep = names if keep is None else ([keep] if isinstance(keep, str) else list(keep))
        rebin, ranges = dict(rebin or {}), dict(ranges or {})
        for what, given in (('keep', keep), ('rebin', rebin), ('ranges', ranges)):
            for n in given:
                if n not in names:
                    raise ValueError("%s: %r is not a dimension of the analysis space %s" % (what, n, names))
        if len(set(keep)) != len(keep):
            raise ValueError("keep names a dimension twice: %s" % (keep,))
        self.fine_shape = tuple(len(e) - 1 for _, e in space)
        self.fine_dims, self.fine_edges = names, [e for _, e in space]
        self.dims, self.edges, self.groups = [], [], []
        for name, fine in space:
            n_fine = len(fine) - 1
            lo, hi = 0, n_fine
            if name in ranges:
                a, b = ranges[name]
                lo, hi = _edge_index(name, fine, a), _edge_index(name, fine, b)
                if not lo < hi:
                    raise ValueError("%r: the range (%r, %r) holds no bin" % (name, a, b))
            if name not in keep:
                if name in rebin:
                    raise ValueError("%r is summed over: it cannot be rebinned (keep it, or give its range)" % name)
                bounds = [lo, hi]
            elif name not in rebin:
                bounds = list(range(lo, hi + 1))
            elif np.ndim(rebin[name]) == 0:
                n = int(rebin[name])
                if n < 1 or n != rebin[name]:
                    raise ValueError("%r: rebin by %r" % (name, rebin[name]))
                bounds = list(range(lo, hi, n)) + [hi]
            else:
                bounds = [_edge_index(name, fine, v) for v in np.asarray(rebin[name], dtype=float).ravel()]
                if len(bounds) < 2 or np.any(np.diff(bounds) <= 0):
                    raise ValueError("%r: the rebinned edges must be at least two, ascending" % name)
                if bounds[0] < lo or bounds[-1] > hi:
                    raise ValueError("%r: the rebinned edges leave the range" % name)
            self.groups.append(np.asarray(bounds, dtype=np.int32))
            if name in keep:
                self.dims.append(name)
                self.edges.append(fine[self.groups[-1]])
        self.shape = tuple(len(e) - 1 for e in self.edges)
        self.n_cells = int(np.prod(self.shape, dtype=np.int64))

    def bin_map(self):
        """int32 [B]: the coarse flat index of every fine bin (C order, as `lf.bin_shape` implies), -1 where it is left out"""
        cell = np.zeros(self.fine_shape, dtype=np.int64)
        out = np.zeros(self.fine_shape, dtype=bool)
        for axis, (n, bounds) in enumerate(zip(self.fine_shape, self.groups)):
            g = np.searchsorted(bounds, np.arange(n), side='right') - 1
            left_out = (np.arange(n) < bounds[0]) | (np.arange(n) >= bounds[-1])
            shape = [1] * len(self.fine_shape)
            shape[axis] = n
            cell = cell * (len(bounds) - 1) + np.where(left_out, 0, g).reshape(shape)
            out = out | left_out.reshape(shape)
        return np.where(out, -1, cell).astype(np.int32).ravel()

    def attach(self, lf, what, derivatives=False):
        """Refuse what has no coarse view (derivatives=True: or not its derivatives), then make this the coarse binning of lf's
        device context -- a no-op while the context still holds it (a new model releases it).  ValueError for a likelihood with
        another analysis space."""
        _binned_for_coarse(lf, what, derivatives=derivatives)
        space = lf.base_model.config['analysis_space']
        if [str(n) for n, _ in space] != self.fine_dims or tuple(lf.bin_shape) != self.fine_shape or \
                not all(np.array_equal(np.asarray(e, dtype=float), mine) for (_, e), mine in zip(space, self.fine_edges)):
            raise ValueError("%s: the binning was made for another analysis space (dimensions %s, bins %s)" % (what, self.fine_dims, self.fine_shape))
        cells = lf.ctx.set_coarse_binning(self.fine_shape, self.groups)
        assert cells == self.n_cells
        return lf


def _prepared(lf, binning, what, derivatives=False):
    if not isinstance(binning, CoarseBinning):
        _binned_for_coarse(lf, what, derivatives=derivatives)                   # (the likelihood's own refusal comes first)
        raise TypeError("%s needs a CoarseBinning, not a %s" % (what, type(binning).__name__))
    return binning.attach(lf, what, derivatives=derivatives)


def expected_coarse_points(lf, binning, points, per_source=False, livetime_days=None):
    """The expected events per cell of `binning` at P parameter points: points = dict parameter name -> array [P] (scalars
    broadcast; absent parameters take their defaults), as `expected_counts_points` -> mu [P, *binning.shape], or
    [P, S, *binning.shape] with per_source.  The host terms (live time, rate multipliers, efficiencies) are those of
    `expected_counts_points`; the morph and the sum over the fine bins of every cell run on the device in one pass over the
    corner rows (bi_expected_coarse).  A point outside the anchor box or with unphysical rates gets nan in every cell."""
    _prepared(lf, binning, 'expected_coarse_points')
    z, scale, _ = lf._batch_terms(points, livetime_days)
    mu, _ = lf.ctx.expected_coarse(binning.n_cells, z if z.shape[1] else None, scale, per_source=per_source)
    return mu.reshape(mu.shape[:-1] + binning.shape)


def expected_coarse(lf, binning, per_source=False, livetime_days=None, **params):
    """The expected events per cell of `binning` at one parameter point -> array of `binning.shape`, or [S, *binning.shape]
    with per_source: a projection of the fitted model with its components.  As `expected_coarse_points`, with the host terms
    of the scalar call `lf(**params)`; nan outside the anchor box or where the rates are unphysical."""
    from .source_wise import SourceWiseBinnedLogLikelihood
    if isinstance(lf, SourceWiseBinnedLogLikelihood):            # (the one-row `_points` form, as its other layers)
        return expected_coarse_points(lf, binning, {k: np.array([v], dtype=float) for k, v in params.items()}, per_source=per_source,
                                      livetime_days=livetime_days)[0]
    _prepared(lf, binning, 'expected_coarse')
    _, zs, scale = lf._host_terms(livetime_days, params)
    shape = ((len(lf.source_name_list),) if per_source else ()) + binning.shape
    if zs is None:
        return np.full(shape, np.nan)
    mu, _ = lf.ctx.expected_coarse(binning.n_cells, zs if len(zs) else None, scale[None, :], per_source=per_source)
    return mu[0].reshape(shape)


def expected_coarse_jacobian_points(lf, binning, points, livetime_days=None):
    """The expected events per cell of `binning` and their first derivatives in the user's parameters at P points (as
    `expected_coarse_points`) -> (names [F], mu [P, *binning.shape], J [P, F, *binning.shape]): names is every registered rate
    multiplier, then every shape parameter (`hesse`'s and `fisher_information`'s order), J[p, f] = d mu_C / d names[f].  The
    derivatives over theta = (z, rate_scale) are summed over the cells on the device in the one pass over the corner rows that
    forms mu (bi_expected_coarse_jacobian: mu has the bits of `expected_coarse_points`), and carried to the user's parameters by
    the chain rule of `values_gradients_hessians` (`hessian.user_jacobian`: live time, efficiencies, shape parameters that
    double as efficiencies).  On an anchor the slopes are those of the cell the point is assigned to.  A point outside the
    anchor box or with unphysical rates is nan throughout."""
    _prepared(lf, binning, 'expected_coarse_jacobian_points', derivatives=True)
    z, scale, _ = lf._batch_terms(points, livetime_days)
    P = len(z)
    mu, jac, _ = lf.ctx.expected_coarse_jacobian(binning.n_cells, z if z.shape[1] else None, scale)
    mult, L, eff, eff_axis, rate_sources = lf._chain_rule_terms(points, P, livetime_days)
    U = user_jacobian(P, z.shape[1], scale.shape[1], mult, L, eff, eff_axis, rate_sources)
    J = np.einsum('pfk,pkc->pfc', U, jac)
    return lf._parameter_names(), mu.reshape((P,) + binning.shape), J.reshape(J.shape[:2] + binning.shape)


def expected_coarse_jacobian(lf, binning, livetime_days=None, **params):
    """`expected_coarse_jacobian_points` at one point (parameter values; absent parameters at their defaults) ->
    (names [F], mu [*binning.shape], J [F, *binning.shape])."""
    _refuse_sourcewise(lf, 'expected_coarse_jacobian')
    names, mu, J = expected_coarse_jacobian_points(lf, binning, {k: np.array([v], dtype=float) for k, v in params.items()},
                                                   livetime_days=livetime_days)
    return names, mu[0], J[0]


def propagate_covariance(jacobian_names, J, names, covariance):
    """Linear propagation of a parameter covariance to the cells (pure numpy, no device): J [F, ...] = d mu / d parameter with
    rows named `jacobian_names`, (names [K], covariance [K, K]) what `hesse` / `expected_covariance` return -> (sigma [...],
    impacts): sigma^2 = J_K^T covariance J_K over the K named parameters (the others are held fixed), impacts an OrderedDict
    name -> J_name sqrt(covariance_name,name), the shift of every cell when that parameter alone moves by its standard
    deviation (signed).  A name that is no row of J is a ValueError; nan in the covariance gives nan."""
    jacobian_names, names = list(jacobian_names), list(names)
    missing = [k for k in names if k not in jacobian_names]
    if missing:
        raise ValueError("not parameters of the likelihood: %s" % ', '.join(str(k) for k in missing))
    if len(set(names)) != len(names):
        raise ValueError("a parameter is named twice: %s" % (names,))
    J = np.asarray(J, dtype=float)
    covariance = np.asarray(covariance, dtype=float)
    if covariance.shape != (len(names), len(names)):
        raise ValueError("the covariance of %d parameters is [%d, %d], not %s" % (len(names), len(names), len(names), covariance.shape))
    Jk = J[[jacobian_names.index(k) for k in names]] if names else np.zeros((0,) + J.shape[1:])
    with np.errstate(invalid='ignore'):
        variance = np.einsum('k...,kl,l...->...', Jk, covariance, Jk)
        sigma = np.sqrt(np.where(variance < 0, 0.0, variance))            # (a rounded zero is no negative variance)
        impacts = OrderedDict((k, Jk[i] * np.sqrt(covariance[i, i])) for i, k in enumerate(names))
    return sigma, impacts


def expected_coarse_band(lf, binning, names, covariance, livetime_days=None, **params):
    """The uncertainty band of a coarse view from a covariance of the parameters, without a posterior chain:
    (names [K], covariance [K, K]) as `hesse` / `expected_covariance` return them, `params` the point (fitted values plus fixed
    ones) -> (mu [*binning.shape], sigma [*binning.shape], impacts: OrderedDict name -> [*binning.shape]), by
    `propagate_covariance` of `expected_coarse_jacobian` -- one device call.  Linear propagation: the band of a model whose
    cells are far from linear over one standard deviation is the posterior's (`expected_coarse_points` over samples)."""
    _refuse_sourcewise(lf, 'expected_coarse_band')
    all_names, mu, J = expected_coarse_jacobian(lf, binning, livetime_days=livetime_days, **params)
    sigma, impacts = propagate_covariance(all_names, J, names, covariance)
    return mu, sigma, impacts


def information_per_cell(J, mu):
    """The Fisher information of independent Poisson cells, cell by cell (pure numpy): J [F, ...], mu [...] ->
    (I [F, F, ...] = J J^T / mu where mu > 0, unbounded [F, ...] bool).  A cell with mu = 0 contributes 0, and the parameters
    that move it (J != 0) are flagged: one event there would decide them.  A negative or nan mu gives nan in that cell."""
    J, mu = np.asarray(J, dtype=float), np.asarray(mu, dtype=float)
    with np.errstate(all='ignore'):
        info = np.where(mu > 0, J[:, None] * J[None, :] / np.where(mu > 0, mu, 1.0), np.where(mu == 0, 0.0, np.nan))
    return info, (mu == 0) & (J != 0)


def coarse_information(lf, binning, livetime_days=None, **truth):
    """The expected (Fisher) information of the likelihood AT THAT BINNING, cell by cell, at a truth (parameter values; absent
    parameters at their defaults) -> (names [F], I [F, F, *binning.shape], unbounded [F, *binning.shape] bool):
    I_C = J_C J_C^T / mu_C (`information_per_cell` of `expected_coarse_jacobian`), no priors.  Its sum over the cells is what
    an analysis in those cells can know; with the identity binning that is `fisher_information(priors=False)`, and no
    rebinning adds to it.  Where the cells show which part of the analysis space constrains which parameter."""
    _refuse_sourcewise(lf, 'coarse_information')
    names, mu, J = expected_coarse_jacobian(lf, binning, livetime_days=livetime_days, **truth)
    info, unbounded = information_per_cell(J, mu)
    return names, info, unbounded


def sourcewise_coarse_jacobian_points(lf, binning, points, per_source=False, livetime_days=None):
    """`expected_coarse_jacobian_points` for a prepared `SourceWiseBinnedLogLikelihood` -> (names [F], mu [P, *binning.shape],
    J [P, F, *binning.shape]), or with per_source (names, mu [P, S, *binning.shape], J [P, S, F, *binning.shape]): every source's
    cells and their derivatives, J[p, s, f] = d mu_s,C / d names[f] -- an impact table per component.  names and the chain rule
    to the user's parameters are those of the grid model (`hessian.user_jacobian`; with per_source the same U is applied to every
    source's block).  On the device one pass over the point's rows sums the sources' basis columns per cell
    (bi_sourcewise_expected_coarse_jacobian); the contraction to the d + S derivatives is the host's, so the number of shape
    parameters does not enter the device work and has no limit but the model's.  The total mu has the bits of
    `expected_coarse_points`; the per-source mu equals its per-source form to rounding.  A point outside the anchor box or with
    unphysical rates is nan throughout."""
    return _sourcewise_jacobian(lf, binning, points, per_source, livetime_days, 'sourcewise_coarse_jacobian_points')


def _sourcewise_jacobian(lf, binning, points, per_source, livetime_days, what):
    """`sourcewise_coarse_jacobian_points` behind the gate of the public function `what`: one gate, one context call"""
    _sourcewise_prepared(lf, binning, what)
    z, scale, _ = lf._batch_terms(points, livetime_days)
    P = len(z)
    mu, jac, _ = lf.ctx.expected_coarse_jacobian(binning.n_cells, z if z.shape[1] else None, scale, per_source=per_source)
    mult, L, eff, eff_axis, rate_sources = lf._chain_rule_terms(points, P, livetime_days)
    U = user_jacobian(P, z.shape[1], scale.shape[1], mult, L, eff, eff_axis, rate_sources)
    J = np.einsum('pfk,pskc->psfc', U, jac) if per_source else np.einsum('pfk,pkc->pfc', U, jac)
    return lf._parameter_names(), mu.reshape(mu.shape[:-1] + binning.shape), J.reshape(J.shape[:-1] + binning.shape)


def sourcewise_coarse_jacobian(lf, binning, per_source=False, livetime_days=None, **params):
    """`sourcewise_coarse_jacobian_points` at one point (parameter values; absent parameters at their defaults) ->
    (names [F], mu [(S,) *binning.shape], J [(S,) F, *binning.shape])."""
    return _sourcewise_one(lf, binning, params, per_source, livetime_days, 'sourcewise_coarse_jacobian')


def _sourcewise_one(lf, binning, params, per_source, livetime_days, what):
    names, mu, J = _sourcewise_jacobian(lf, binning, {k: np.array([v], dtype=float) for k, v in params.items()}, per_source,
                                        livetime_days, what)
    return names, mu[0], J[0]


def sourcewise_coarse_band(lf, binning, names, covariance, livetime_days=None, **params):
    """`expected_coarse_band` for a prepared `SourceWiseBinnedLogLikelihood`: (names [K], covariance [K, K]) as
    `inference.hesse(lf, ...)` / `inference.expected_covariance(lf, ...)` return them, `params` the point ->
    (mu [*binning.shape], sigma [*binning.shape], impacts: OrderedDict name -> [*binning.shape]) by `propagate_covariance` of
    `sourcewise_coarse_jacobian` -- one device call for all parameters."""
    all_names, mu, J = _sourcewise_one(lf, binning, params, False, livetime_days, 'sourcewise_coarse_band')
    sigma, impacts = propagate_covariance(all_names, J, names, covariance)
    return mu, sigma, impacts


def sourcewise_coarse_information(lf, binning, livetime_days=None, **truth):
    """`coarse_information` for a prepared `SourceWiseBinnedLogLikelihood` -> (names [F], I [F, F, *binning.shape],
    unbounded [F, *binning.shape] bool): `information_per_cell` of `sourcewise_coarse_jacobian`, no priors."""
    names, mu, J = _sourcewise_one(lf, binning, truth, False, livetime_days, 'sourcewise_coarse_information')
    info, unbounded = information_per_cell(J, mu)
    return names, info, unbounded


def coarse_counts(lf, binning, datasets=None):
    """The resident datasets' counts per cell of `binning` -> [T, *binning.shape] (datasets: indices, None: all), summed on
    the device from whichever form the data are held in (dense, or the lists of device-generated toys)."""
    _prepared(lf, binning, 'coarse_counts')
    if not lf.is_data_set:
        raise NotPreparedException("coarse_counts requires you to first set the data using set_data()")
    n = lf.ctx.coarse_counts(binning.n_cells, datasets)
    return n.reshape((len(n),) + binning.shape)


def coarse_statistics(n, mu):
    """The goodness-of-fit statistics over coarse cells, from counts n and expectations mu (arrays [..., C], broadcast against
    each other) -> (deviance [...], pearson [...]), in the cancellation-free per-cell forms of the device's `gof_terms`:
        half-deviance   n > 0: (mu - n) - n log(mu / n)     n = 0: mu
        Pearson         n > 0: (n - mu)^2 / mu              n = 0: mu
    n = mu = 0 gives 0 in both, n > 0 with mu = 0 gives +inf in both; a negative or nan mu (or a nan n) gives nan in both, a
    negative or non-integer n +inf in both."""
    n, mu = np.broadcast_arrays(np.asarray(n, dtype=float), np.asarray(mu, dtype=float))
    hit = n > 0
    with np.errstate(all='ignore'):
        safe_n = np.where(hit, n, 1.0)
        half = np.where(hit, (mu - n) - n * np.log(np.where(hit, mu, 1.0) / safe_n), mu)
        pearson = np.where(hit, (n - mu) ** 2 / np.where(hit & (mu == 0), 1.0, mu), mu)
        empty_expectation = hit & (mu == 0)
        half = np.where(empty_expectation, np.inf, half)
        pearson = np.where(empty_expectation, np.inf, pearson)
        no_count = (n < 0) | (n != np.floor(n))
        half, pearson = np.where(no_count, np.inf, half), np.where(no_count, np.inf, pearson)
        bad = ~(mu >= 0) | np.isnan(n)
        half, pearson = np.where(bad, np.nan, half), np.where(bad, np.nan, pearson)
    return 2.0 * half.sum(axis=-1), pearson.sum(axis=-1)
