"""Source-wise UNBINNED likelihoods on the device: one anchor grid per source, over events.

    lf = SourceWiseUnbinnedLogLikelihood(pdf_base_config, likelihood_config=None, **overrides)
    lf.add_rate_parameter(...); lf.add_shape_parameter(...); lf.prepare(); lf.set_data(d)   (or lf.set_datasets([d0, d1, ...]))
    lf(**params), lf.eval_points, lf.value_and_gradient, lf.values_and_gradients,
    lf.value_gradient_hessian, lf.values_gradients_hessians, lf.bestfit_minuit, blueice_amd.inference.hesse(lf, values, datasets=),
    lf.bestfit_scipy, lf.bestfit_batched, lf.bestfit_device, lf.likelihood_ratio_scan, lf.one_parameter_interval,
    blueice_amd.inference.bestfit_toys(lf) over the sets of set_datasets, lf.n_events_per_dataset, and as a term of a LogLikelihoodSum
    sourcewise_event_toys(lf, n_toys, seed, **truth), sourcewise_event_toys_points(lf, points, n_toys, seed), sourcewise_simulated_events(lf),
    blueice_amd.inference.toy_mc_fits(lf, ...), .toy_test_statistics(lf, ...), .neyman_thresholds(lf, ...)
    blueice_amd.sampler.sample_posterior(lf, ...), blueice_amd.inference.bestfit_emcee(lf, ...), blueice_amd.grid.grid_scan(lf, ...)

This is the reference's `source_wise_interpolation` for the likelihood it exists for (blueice/likelihood.py:152-171, 210-240,
534-563): every source keeps the pdf values of the events at the anchors of the shape parameters IT responds to only.
`UnbinnedLogLikelihood(source_wise_interpolation=True)` builds the same few models but then expands them to the Cartesian grid of
all shape parameters on the device -- prod n_i anchors x S x N values -- which caps the number of shape parameters at a handful.
Here the device holds the event store of a source-wise model (bi_sourcewise_score_events / bi_sourcewise_events_begin,
include/blueice_hip.h): sum_s prod_{i in O_s} n_i rows of N values, and an evaluation reads sum_s 2^e_s of them
(k_sourcewise_events):
    ll = sum_e log(sum_s r_s tau_s,e) - sum_s r_s,     tau_s,e the multilinear interpolation of source s's own anchors at event e
with the reference's outlier clamp (config['outlier_likelihood'], default 1e-12) and nan-dropping (numpy.nansum over sources).

`prepare()` builds models at the projected anchors only.  Where every source is a HistogramPdfSource with one interpolation
method (the test of UnbinnedLogLikelihood's device scoring) the density histograms are the model's rows and `set_data` /
`set_datasets` send the event coordinates only; otherwise the model is a one-bin carrier of the geometry and the rates and the
events are scored on the host, one `source.pdf(*coords)` per own anchor row.  Both give the same bits.

Limits as SourceWiseBinnedLogLikelihood's: 32 shape parameters, 8 sources, 3 own parameters per source.

Second derivatives: with `likelihood_config['analytic_hessian'] = True`, `supports_hessian` is true once data are set and
`value_gradient_hessian`, `values_gradients_hessians`, `bestfit_minuit` and `blueice_amd.inference.hesse` run on the analytic
Hessian over the event store (bi_eval_sourcewise_events_hess, kernel k_sourcewise_events_curv: one pass over the events and a
host contraction per point) through the usual chain rule (priors, GaussianPrior, live time); `hessian_method` is 'analytic'.  By
default (`analytic_hessian` False) `supports_hessian` is False and the same calls take central differences of the analytic
gradient, 2 F + 1 displaced gradient evaluations per point, `hessian_method` 'gradient-differences': the behaviour the class had
before the analytic route existed, which stays the default so that results do not change under existing users.  Events carry no
expected information: `fisher_information*` and `expected_*` stay refused either way.

Event-level toys are drawn on the device (bi_sourcewise_simulate_event_toys; kernels k_sourcewise_pmf and k_sourcewise_sim_*):
`sourcewise_event_toys_points(lf, points, n_toys, seed)` draws n_toys[h] toys at the H truths of `points` in one call and makes
them the likelihood's datasets, `sourcewise_event_toys` is its one-truth spelling and `sourcewise_simulated_events(lf, t)` fetches
the events.  The stream is `UnbinnedLogLikelihood.simulate_toys`': toy t of a call is toy toy_offset + t of the seed's ensemble,
whatever the number of toys, the grouping of truths into calls or the sub-batches the device works in, and where no comparison
is a near-tie it is event for event the toy the expanded grid model draws.  They need `scoring_route == 'device'`.  On top of
them `blueice_amd.inference.toy_mc_fits(lf, ...)`, `toy_test_statistics(lf, ...)` and `neyman_thresholds(lf, ...)` take the
class, with chunks that run across hypothesis boundaries as for binned models.  The bound lf.simulate_toy* / lf.toy_* /
lf.neyman_thresholds stay refused and name these spellings.
Posteriors and marginal likelihoods run on the event store as well, as functions that take the class:
`blueice_amd.sampler.sample_posterior(lf, ...)` and `blueice_amd.inference.bestfit_emcee(lf, ...)` (bi_sample_stretch_sourcewise_events:
the proposals planned on the device by the event variant of k_sourcewise_plan, the chain bit for bit the host engine's, no host wait
inside the step loop, GaussianPrior constraints on the device) and `blueice_amd.grid.grid_scan(lf, ...)`
(bi_grid_reduce_sourcewise_events, one work item per grid point); `datasets=` indexes the event sets of `set_datasets` or of
`sourcewise_event_toys*`.  `likelihood_config['sourcewise_grid_route']` applies: 'auto' and 'points' are the per-point route, 'scan'
raises -- the matrix-core scan route does not read the event store, and there is no `eval_points_scan` here.  The bound
lf.sample_posterior / lf.bestfit_emcee / lf.grid_scan stay refused and name these spellings.
Refused with NotImplementedError: compute_pdf / full_output, allow_negative sources, Beeston-Barlow, the bound sampling and grid_scan
methods, and everything that reads the dense store of a binned source-wise model.
"""
import numpy as np

from .exceptions import NotPreparedException
from .likelihood import LogLikelihoodBase, _needs_preparation, histogram_lookup_method
from .source_wise import _SourceWiseLikelihood

__all__ = ['SourceWiseUnbinnedLogLikelihood', 'sourcewise_event_toys', 'sourcewise_event_toys_points', 'sourcewise_simulated_events']

_SCOPE = ("an unbinned source-wise model (SourceWiseUnbinnedLogLikelihood) has value, gradient, the fit, scan and interval layers and "
          "fits of the event sets of set_datasets, and (likelihood_config['analytic_hessian'] = True) the analytic Hessian behind "
          "values_gradients_hessians, bestfit_minuit and inference.hesse; event toys drawn on the device are the functions "
          "sourcewise_event_toys(lf, n_toys, seed, **truth), sourcewise_event_toys_points(lf, points, n_toys, seed) and "
          "sourcewise_simulated_events(lf, t) of blueice_amd, and toy-calibrated inference is blueice_amd.inference.toy_mc_fits(lf, ...), "
          "toy_test_statistics(lf, ...) and neyman_thresholds(lf, ...), not the bound methods; posterior sampling and gridded "
          "likelihoods are the functions blueice_amd.sampler.sample_posterior(lf, ...), blueice_amd.inference.bestfit_emcee(lf, ...) and "
          "blueice_amd.grid.grid_scan(lf, ...), not the bound methods either; not the expected (Fisher) information, or anything that "
          "reads binned counts")


def _refused(name):
    def method(self, *args, **kwargs):
        raise NotImplementedError("%s is not available: %s" % (name, _SCOPE))
    method.__name__ = name
    return method


class SourceWiseUnbinnedLogLikelihood(_SourceWiseLikelihood):
    """Extended unbinned likelihood whose sources each morph over their own shape parameters (see the module's docstring)."""

    _REFUSED = ('simulate_toy', 'simulate_toys', 'simulate_toys_points', 'simulated_events', 'eval_toys', 'eval_toys_points',
                'toy_mc_fits', 'toy_test_statistics', 'neyman_thresholds', 'sample_posterior', 'bestfit_emcee', 'grid_scan',
                'set_binned_data', 'best_anchor', 'ps_interpolator', 'n_model_events_interpolator',
                'fisher_information', 'fisher_information_points', 'expected_covariance', 'expected_errors',
                'gof_statistics', 'goodness_of_fit', 'expected_counts', 'expected_counts_points',
                'expected_coarse', 'expected_coarse_points', 'coarse_counts', 'asimov', 'asimov_points', 'asimov_test_statistic',
                'real_data', 'expected_upper_limit', 'expected_discovery_significance')

    _full_grid_class = 'UnbinnedLogLikelihood'

    @property
    def supports_hessian(self):
        """True once data are set when likelihood_config['analytic_hessian'] is true: the analytic Hessian over the event store
        (bi_eval_sourcewise_events_hess; `hessian_method` is then 'analytic').  The default is False -- `values_gradients_hessians`
        takes differences of the analytic gradient, as it did before the analytic route existed -- so that nothing changes for
        a likelihood that does not ask for it."""
        return bool(self.config.get('analytic_hessian', False)) and self.ctx is not None and bool(self.is_data_set)

    def _device_hessian(self, z, scale, dataset):
        return self.ctx.eval_events_hess(z, scale, dataset)

    def __init__(self, pdf_base_config, likelihood_config=None, **kwargs):
        super().__init__(pdf_base_config, likelihood_config, **kwargs)
        self.outlier_likelihood = self.config.get('outlier_likelihood', 1e-12)
        self._lookup = None             # (method, grid) of the device scoring, or None: the events are scored on the host

    # -- lifecycle -------------------------------------------------------------------------
    def prepare(self, n_cores=1, ipp_client=None):
        """Models at the anchors some source needs only, then the model's rows: the sources' density histograms where the
        device can look the events up in them, else one bin per row (the model then carries the geometry and the rates)."""
        self._build_projected_anchors(n_cores)
        S = len(self.source_name_list)
        edges = [np.asarray(e, dtype=float) for _, e in self.base_model.config['analysis_space']]
        sources = [src for s in range(S) for src in self._own_sources(s)]
        method = histogram_lookup_method(sources, edges) if self.config.get('device_scoring', True) else None
        if method is None:
            self._lookup = None
            self._upload_source_rows(1, lambda source: np.ones(1))
        else:
            self._lookup = (method, edges if method == 'piecewise' else [0.5 * (e[:-1] + e[1:]) for e in edges])
            n_bins = int(np.prod([len(e) - 1 for e in edges], dtype=np.int64))
            self._upload_source_rows(n_bins, lambda source: source._pdf_histogram.histogram.ravel())
        self.is_data_set = False
        self.is_prepared = True

    @property
    def scoring_route(self):
        """'device' (bi_sourcewise_score_events) or 'host' (one source.pdf call per own anchor row): the route the next
        set_data takes for events with finite coordinates"""
        return 'device' if self._lookup else 'host'

    @_needs_preparation
    def set_data(self, d):
        """Score the events at every source's own anchors and make them dataset 0."""
        LogLikelihoodBase.set_data(self, d)
        self._set_event_sets([d])

    @_needs_preparation
    def set_datasets(self, datasets):
        """Make a list of T event record arrays the likelihood's datasets (dataset 0 is what plain `lf(**params)` sees;
        `eval_points(..., dataset=)` and `blueice_amd.inference.bestfit_toys(lf)` take them all)."""
        datasets = list(datasets)
        if not datasets:
            raise ValueError("need at least one dataset")
        names = [n for n, _ in self.base_model.config['analysis_space']]
        for t, d in enumerate(datasets):
            fields = getattr(getattr(d, 'dtype', None), 'names', None) or ()
            missing = [n for n in names if n not in fields]
            if missing:
                raise ValueError("dataset %d lacks the analysis dimensions %s" % (t, ', '.join(missing)))
        LogLikelihoodBase.set_data(self, datasets[0])
        if len(datasets) > 1:
            self._data = None
        self._set_event_sets(datasets)

    def _set_event_sets(self, datasets):
        self.bin_shape = (len(datasets[0]),)
        coords = [[np.asarray(c, dtype=float) for c in self.base_model.to_analysis_dimensions(d)] for d in datasets]
        if self._lookup and all(np.all(np.isfinite(c)) for cs in coords for c in cs):
            method, grid = self._lookup
            if method == 'linear':               # constant density in the outer half of the boundary bins (source.py:232-241)
                coords = [[np.clip(c, g[0], g[-1]) for c, g in zip(cs, grid)] for cs in coords]
            self.ctx.score_events(method, grid, coords, self.outlier_likelihood)
            self.last_scoring_route = 'device'
            return
        own = [self._own_sources(s) for s in range(len(self.source_name_list))]

        def rows(s, local):
            source = own[s][local]
            parts = [np.asarray(source.pdf(*cs), dtype=float).reshape(len(d)) for cs, d in zip(coords, datasets)]
            return np.concatenate(parts) if parts else np.zeros(0)
        self.ctx.set_event_rows([len(d) for d in datasets], rows, self.outlier_likelihood)
        self.last_scoring_route = 'host'

    def _native_sample_stretch(self, *args, **kwargs):
        """what blueice_amd.sampler.sample_posterior (and through it inference.bestfit_emcee) calls for this class in the place of
        ctx.sample_stretch: the sampler on the event store (the bound sample_posterior / bestfit_emcee stay refused)"""
        return self.ctx.sample_stretch_events(*args, **kwargs)

    def _native_grid_reduce(self, *args, **kwargs):
        """what blueice_amd.grid.grid_scan calls for this class in the place of ctx.grid_reduce (the bound grid_scan stays refused)"""
        return self.ctx.grid_reduce_events(*args, **kwargs)

    def _simulate_toys_points(self, points, n_toys, seed=0, livetime_days=None):
        """what blueice_amd.inference's toy layers call for this class (the bound simulate_toys_points stays refused)"""
        return sourcewise_event_toys_points(self, points, n_toys, seed=seed, livetime_days=livetime_days)

    @property
    def n_events_per_dataset(self):
        """events of every dataset the likelihood holds: [T]"""
        return self.ctx.event_set_counts()

    @property
    def data_events_per_bin(self):
        raise NotImplementedError("data_events_per_bin is not available: %s" % _SCOPE)


for _name in SourceWiseUnbinnedLogLikelihood._REFUSED:
    setattr(SourceWiseUnbinnedLogLikelihood, _name, _refused(_name))


# ---- event-level toys drawn on the device -------------------------------------------------------------------------------------

def sourcewise_event_toys_points(lf, points, n_toys, seed=0, livetime_days=None):
    """Draw event-level toys ON THE DEVICE at H truth points in one call (bi_sourcewise_simulate_event_toys) and make them the
    likelihood's datasets: n_toys[h] toys (an int: the same number everywhere) at truth h, truth-major.  points: dict parameter
    name -> array [H] (scalars broadcast; absent parameters take their defaults), as `eval_points`.  Per source N_s ~ Poisson(r_s),
    every event a bin of the source's morphed histogram drawn with probability density x volume and a uniform position inside it
    -- `UnbinnedLogLikelihood.simulate_toys`' stream: toy t of the call is toy `toy_offset + t` (the context parameter) of the
    seed's ensemble, so an ensemble over many hypotheses does not depend on how they are grouped into calls.  Dataset 0 is what
    plain `lf(**params)` sees; `eval_points(..., dataset=)`, `inference.bestfit_toys(lf)` and `inference.hesse(..., datasets=)`
    take them all.  Afterwards `toy_truth` [T] holds the truth index of every dataset.  Needs histogram-pdf sources with one
    lookup method (`scoring_route == 'device'`), NotImplementedError otherwise.  -> events per toy and source [T, S]."""
    if not isinstance(lf, SourceWiseUnbinnedLogLikelihood):
        raise TypeError("sourcewise_event_toys_points takes a SourceWiseUnbinnedLogLikelihood, not a %s" % type(lf).__name__)
    if not lf.is_prepared:
        raise NotPreparedException("sourcewise_event_toys_points requires you to first prepare the likelihood function using prepare()")
    if lf.scoring_route != 'device':
        raise NotImplementedError("event toys of an unbinned source-wise model are drawn on the device from the sources' density "
                                  "histograms: they need scoring_route == 'device' (every source a HistogramPdfSource with one "
                                  "interpolation method, likelihood_config['device_scoring'] not False); this likelihood scores on the host")
    z, scale, _ = lf._batch_terms(points, livetime_days)
    H = max(len(z), np.size(n_toys))
    n_toys = np.ascontiguousarray(np.broadcast_to(np.asarray(n_toys, dtype=np.int64), (H,)))
    z, scale = np.broadcast_to(z, (H, z.shape[1])), np.broadcast_to(scale, (H, scale.shape[1]))
    for i, name in enumerate(lf.shape_parameters):
        lo, hi = lf.get_bounds(name)
        outside = np.flatnonzero(~((z[:, i] >= lo) & (z[:, i] <= hi)))
        if len(outside):
            raise ValueError("cannot simulate outside the anchor box (truth %d: %s = %r)" % (outside[0], name, z[outside[0], i]))
    edges = [np.asarray(e, dtype=float) for _, e in lf.base_model.config['analysis_space']]
    counts = lf.ctx.simulate_event_toys(lf._lookup[0], edges, z if z.shape[1] else None, scale, n_toys, seed, lf.outlier_likelihood)
    lf._data = None
    lf.is_data_set = True
    lf.bin_shape = (int(counts[0].sum()),)
    lf.toy_truth = np.repeat(np.arange(H), n_toys)
    lf.last_scoring_route = 'device'
    return counts


def sourcewise_event_toys(lf, n_toys, seed=0, livetime_days=None, **truth):
    """`sourcewise_event_toys_points` at one truth: `n_toys` toys at the given parameter values (defaults elsewhere), the
    counterpart of `UnbinnedLogLikelihood.simulate_toys`.  -> events per toy and source [T, S]."""
    if int(n_toys) < 1:
        raise ValueError("n_toys must be at least 1")
    return sourcewise_event_toys_points(lf, {k: np.array([float(v)]) for k, v in truth.items()}, [int(n_toys)], seed=seed,
                                        livetime_days=livetime_days)


def sourcewise_simulated_events(lf, t=None):
    """The events of the toys `sourcewise_event_toys*` drew, as a record array with the analysis dimensions and a 'source' field,
    as `Model.simulate` returns them: of toy t, or (t = None) of all toys, set by set in drawn order, with a 'toy' field when
    the likelihood holds more than one -- what `UnbinnedLogLikelihood.simulated_events` returns."""
    coords, source = lf.ctx.download_events()
    names = [n for n, _ in lf.base_model.config['analysis_space']]
    many = lf.ctx.T > 1
    d = np.zeros(coords.shape[1], dtype=[(n, float) for n in names] + [('source', int)] + ([('toy', int)] if many else []))
    for n, c in zip(names, coords):
        d[n] = c
    d['source'] = source
    if many:
        d['toy'] = np.repeat(np.arange(lf.ctx.T), lf.ctx.event_set_counts())
    if t is None:
        return d
    if not many:
        if t != 0:
            raise ValueError("the likelihood holds one toy")
        return d
    keep = d[d['toy'] == int(t)]
    return keep[[n for n in keep.dtype.names if n != 'toy']].copy()
