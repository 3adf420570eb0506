"""Source-wise UNBINNED likelihoods on the device: one anchor grid per source, over events.

    lf = SourceWiseUnbinnedLogLikelihood(pdf_base_config, likelihood_config=None, **overrides)
    lf.add_rate_parameter(...); lf.add_shape_parameter(...); lf.prepare(); lf.set_data(d)   (or lf.set_datasets([d0, d1, ...]))
    lf(**params), lf.eval_points, lf.value_and_gradient, lf.values_and_gradients,
    lf.value_gradient_hessian, lf.values_gradients_hessians, lf.bestfit_minuit, blueice_amd.inference.hesse(lf, values, datasets=),
    lf.bestfit_scipy, lf.bestfit_batched, lf.bestfit_device, lf.likelihood_ratio_scan, lf.one_parameter_interval,
    blueice_amd.inference.bestfit_toys(lf) over the sets of set_datasets, lf.n_events_per_dataset, and as a term of a LogLikelihoodSum

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
Refused with NotImplementedError: compute_pdf / full_output, allow_negative sources, Beeston-Barlow, event toys drawn on the
device (simulate_toy*), sampling and grid_scan, and everything that reads the dense store of a binned source-wise model.
"""
import numpy as np

from .likelihood import LogLikelihoodBase, _needs_preparation, histogram_lookup_method
from .source_wise import _SourceWiseLikelihood

__all__ = ['SourceWiseUnbinnedLogLikelihood']

_SCOPE = ("an unbinned source-wise model (SourceWiseUnbinnedLogLikelihood) has value, gradient, the fit, scan and interval layers and "
          "fits of the event sets of set_datasets, and (likelihood_config['analytic_hessian'] = True) the analytic Hessian behind "
          "values_gradients_hessians, bestfit_minuit and inference.hesse; not event toys drawn on the device, sampling, gridded "
          "likelihoods, the expected (Fisher) information, or anything that reads binned counts")


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

    @property
    def n_events_per_dataset(self):
        """events of every dataset the likelihood holds: [T]"""
        return self.ctx.event_set_counts()

    @property
    def data_events_per_bin(self):
        raise NotImplementedError("data_events_per_bin is not available: %s" % _SCOPE)


for _name in SourceWiseUnbinnedLogLikelihood._REFUSED:
    setattr(SourceWiseUnbinnedLogLikelihood, _name, _refused(_name))
