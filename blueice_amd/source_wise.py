"""Source-wise likelihoods on the device: one anchor grid per source.  This module: binned data, the context both kinds share
(`SourceWiseContext`) and their common base; unbinned data -- the event store of the same model -- is
`source_wise_unbinned.SourceWiseUnbinnedLogLikelihood`.

    lf = SourceWiseBinnedLogLikelihood(pdf_base_config, likelihood_config=None, **overrides)
    lf.add_rate_parameter(...); lf.add_shape_parameter(...); lf.prepare(); lf.set_data(d)
    lf(**params), lf.eval_points, lf.value_and_gradient, lf.values_and_gradients,
    lf.bestfit_scipy, lf.bestfit_batched, lf.bestfit_device, lf.likelihood_ratio_scan, lf.one_parameter_interval,
    lf.value_gradient_hessian, lf.values_gradients_hessians, lf.bestfit_minuit, blueice_amd.inference.hesse(lf, values),
    lf.fisher_information_points, lf.expected_covariance, lf.expected_errors,
    lf.simulate_toys_points, lf.toy_test_statistics, lf.neyman_thresholds, and as functions of blueice_amd.inference:
    bestfit_toys(lf), toy_mc_fits(lf, n), gof_statistics(lf, ...), goodness_of_fit(lf, ...), expected_counts_points(lf, points),
    lf.asimov_points, lf.asimov_test_statistic, lf.expected_discovery_significance, blueice_amd.asimov.asimov(lf, **truth),
    blueice_amd.asimov.real_data(lf, counts), blueice_amd.inference.expected_upper_limit(lf, target, bound),
    blueice_amd.coarse.CoarseBinning(lf, ...), expected_coarse_points(lf, binning, points), expected_coarse(lf, binning, **params),
    coarse_counts(lf, binning), and gof_statistics(lf, ..., binning=) / goodness_of_fit(lf, ..., binning=)

`BinnedLogLikelihood` morphs over ONE tensor-product grid of all shape parameters: prod n_i anchor models in HBM and S 2^d
rows per evaluation, which caps the number of shape parameters at a handful.  Here every source morphs over the parameters
IT responds to only (`source_shape_parameters`: all of them except the settings its config lists under dont_hash_settings --
the reference's `source_wise_interpolation`, which the reference and `BinnedLogLikelihood` refuse for binned likelihoods):
source s keeps prod_{i in O_s} n_i rows, and an evaluation reads sum_s 2^e_s of them (libblueice_hip's bi_factored_* /
bi_eval_factored / bi_fit_batched_factored, include/blueice_hip.h).  `prepare()` builds models only at the anchors some source
needs and never enumerates the product grid.

Second derivatives are analytic (bi_eval_sourcewise_hess, bi_eval_sourcewise_fisher): each source is multilinear over at most
three own axes, so the Hessian and the expected information over all d + S parameters follow from one Gram matrix over at most
32 per-source basis columns and a few linear sums, whatever the number of shape parameters.  `lf.hesse` and
`lf.fisher_information` stay unbound (their messages name the spellings that work).

Toys, goodness of fit and the expectation per bin run on the device too (bi_sourcewise_generate_toys, bi_eval_sourcewise_gof,
bi_sourcewise_expected_counts): toy ensembles at truth points replace the counts as dense datasets and are fitted in lock-step by
the layers that exist for the grid model, which duck-type on the context.  The bound names the earlier tests pin -- lf.simulate_toys,
lf.bestfit_toys, lf.toy_mc_fits, lf.gof_statistics, lf.goodness_of_fit, lf.expected_counts, lf.expected_counts_points -- stay
refused and name the spelling that works; `blueice_amd.inference.expected_counts(lf, **params)` stays refused as well (use the
`_points` form with one-row arrays).

Asimov and real-valued data live in a store of their own beside the counts (bi_sourcewise_set_real_counts,
bi_sourcewise_set_asimov_counts), evaluated by bi_eval_sourcewise_real and fitted by bi_fit_batched_sourcewise_real: the factories
of blueice_amd.asimov take a prepared source-wise model and return the `AsimovLikelihood` view they return for a
`BinnedLogLikelihood`, and `asimov_test_statistic`, `expected_upper_limit` and `expected_discovery_significance` of
blueice_amd.inference run over it -- one profile scan where an ensemble of toys per hypothesis would be needed otherwise.  No
observed data are needed for them.  The bound lf.asimov, lf.real_data and lf.expected_upper_limit stay refused and name these
spellings; lf.asimov_points, lf.asimov_test_statistic and lf.expected_discovery_significance are bound.

Coarse views -- projections, a rebinned analysis space, a signal box -- are summed on the device as well
(bi_sourcewise_set_coarse_binning, bi_sourcewise_expected_coarse, bi_sourcewise_coarse_counts): the functions of blueice_amd.coarse
take a prepared source-wise model and a `CoarseBinning` made for it, and `gof_statistics` / `goodness_of_fit` of
blueice_amd.inference take that binning as `binning=` (the toys are still fitted on the fine bins).  A projection comes down as
its cells, not as every fine bin.  The bound lf.expected_coarse, lf.expected_coarse_points and lf.coarse_counts stay refused and
name these spellings.  The derivatives of coarse views are summed in the same kind of pass (bi_sourcewise_expected_coarse_jacobian:
the per-cell sums of the sources' basis columns, contracted on the host, so the number of shape parameters does not enter the
device work), per source as well: blueice_amd.coarse.sourcewise_coarse_jacobian / _points, sourcewise_coarse_band and
sourcewise_coarse_information.  The grid model's names (expected_coarse_jacobian*, expected_coarse_band, coarse_information), as
functions of blueice_amd.coarse and as bound names, stay refused and name those spellings.

The ensemble sampler runs on this model too (bi_sample_stretch_sourcewise): a planner kernel turns the proposals into work items
on the device (k_sourcewise_plan; `ctx.eval_planned` is the same path for points given by the host), so a half-step is five
launches queued on one stream and the step loop waits for nothing.  `blueice_amd.sampler.sample_posterior(lf, ...)` and
`blueice_amd.inference.bestfit_emcee(lf, ...)` reach it through `BatchObjective.native()` like any other likelihood, with
`datasets=` after `simulate_toys_points` and with `GaussianPrior` constraints on the device.  The bound lf.sample_posterior and
lf.bestfit_emcee stay refused and name these spellings.

Gridded likelihoods -- the marginal likelihood by quadrature, the grid profile, a credible limit without a chain -- run on the
device as well (bi_grid_reduce_sourcewise): `blueice_amd.grid.grid_scan(lf, keep=..., reduce=...)` takes a prepared source-wise
model, with `datasets=` after `simulate_toys_points` and with priors; the bound lf.grid_scan stays refused.
`likelihood_config['sourcewise_grid_route']` -- 'auto' (default), 'points' or 'scan' -- names how a chunk of the grid is
evaluated: one work item per point (the kernels of eval_points), or the matrix-core scan route (bi_eval_sourcewise_scan,
`lf.eval_points_scan(points)`): the points sorted by (cell tuple, dataset) on the device and evaluated 16 at a time on the fp64
matrix cores over the compacted rows of the non-empty-bin form, a group's rows read once per strip of bins.  That route needs
`nonempty_bins` and at most 32 rows per point (sum_s 2^e_s); its values agree with eval_points' to rounding, and -- unlike every
other entry point -- a point's bits may depend on the batch it is evaluated in (a repeated call repeats its bits).  No existing
entry point changes its route: eval_points, the fits and the sampler keep their kernels and their bits.

The counts are dense, and by default every evaluation walks every bin.  `likelihood_config['nonempty_bins']` -- False (default),
True or 'auto' (build when at most a quarter of the bins of all datasets hold events) -- adds the non-empty-bin form of the data
(bi_sourcewise_build_nonempty; `ctx.build_nonempty()` / `ctx.drop_nonempty()`): per dataset the list of bins with events and a
compacted copy of the model's rows over it, so that ll = sum over the listed bins of n log mu, less sum_s r_s N_s with N_s the
interpolated row totals, less the lgamma sum.  `set_data`, `set_binned_data` and `simulate_toys_points` rebuild it after they
change the counts; `lf(**params)`, eval_points, values_and_gradients, the native fits, scans, intervals, toy fits, `neyman_thresholds`
and the sampler then read the listed bins only, with no change of their own (results agree with the dense form's to rounding, not
bit for bit).  Hessians, Fisher information, goodness of fit, the expectation, coarse views and the real-valued store keep reading
the dense store.

Limits: 32 shape parameters, 8 sources, at most 3 own parameters per source (a source that responds to more belongs on the
full grid).  Unbinned data: `SourceWiseContext.score_events` / `set_event_rows` put an event store beside the counts
(bi_sourcewise_score_events, bi_sourcewise_events_begin ...); while it exists `eval`, `eval_grad` and `fit_batched` are the extended
unbinned likelihood over its event sets and every other call of the context is refused by the library; `drop_events` releases it.
`SourceWiseContext.simulate_event_toys` draws event-level toys on the device into that store (bi_sourcewise_simulate_event_toys)
and `download_events` fetches them; the class layer is blueice_amd.source_wise_unbinned.
Not available, and refused with NotImplementedError: sources that may go negative, Beeston-Barlow, compute_pdf /
full_output calls, eval_toys*, Hessians, sampling and gridded likelihoods on an Asimov view, and the bound lf.grid_scan (the
function is the spelling that works, above).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _capi
from ._capi import as_f64, ptr
from .device import DeviceContext, grid_reduce_call
from .histdd import Histdd, device_histograms
from .likelihood import DeviceLogLikelihood, LogLikelihoodBase, _needs_data, _needs_preparation

__all__ = ['SourceWiseBinnedLogLikelihood', 'SourceWiseContext', 'MAX_SHAPE_PARAMETERS', 'MAX_SOURCES', 'MAX_OWN_PARAMETERS']

MAX_SHAPE_PARAMETERS, MAX_SOURCES, MAX_OWN_PARAMETERS = 32, 8, 3


def _find_cell(g, z):
    """scipy's find_indices on one axis, the last cell closed -> (k, t)"""
    n = len(g)
    if z == g[n - 1]:
        k = n - 2
    else:
        k = min(max(int(np.searchsorted(g, z, side='right')) - 1, 0), n - 2)
    return k, (z - g[k]) / (g[k + 1] - g[k])


class SourceWiseContext:
    """What the evaluation code of DeviceLogLikelihood and the native fit loop (profile.BatchObjective.native) see as `ctx`:
    a thin adapter over a DeviceContext whose model is the source-wise store.  It exposes what they duck-type on -- eval,
    eval_grad, eval_hess (eval_events_hess on the event store), eval_fisher, eval_gof, expected_counts, set_coarse_binning, expected_coarse, expected_coarse_jacobian,
    coarse_counts,
    generate_toys_points, download_counts, simulate_event_toys / download_events (event-level toys into the event store), set_param / get_param,
    fit_batched, interpolate('mus', z), T, the real-valued store under DeviceContext's names (set_real_counts, set_asimov_counts,
    real_count_sets, download_real_counts, eval_real, fit_batched_real), sample_stretch (with eval_planned, the same device planner
    for points given by the host) -- and the uploads; nothing else of the DeviceContext (plans, grids ...) has a meaning here and is
    an AttributeError."""

    def __init__(self, device=None):
        self._dev = DeviceContext(device)
        self.device = self._dev.device
        self.d = self.S = self.B = None
        self.T = 0
        self._counts = None
        self._coarse_key = None
        self._binned = None                     # (T, host copy) of the counts while an event store stands in front of them
        self._sim_k = 0                         # analysis dimensions of the events simulate_event_toys drew

    def set_param(self, name, value):
        """a parameter of the underlying context (`toy_offset`: the number of a generator call's first toy in the seed's ensemble)"""
        self._dev.set_param(name, value)

    def get_param(self, name):
        return self._dev.get_param(name)

    def close(self):
        self._dev.close()

    def info(self):
        return self._dev.info()

    def histogram_events(self, edges, coords):
        return self._dev.histogram_events(edges, coords)

    # -- model -----------------------------------------------------------------------------
    def begin_model(self, anchor_z, S, B, own_axes):
        """anchor_z: d ascending arrays; own_axes: per source the ascending indices of the axes it owns"""
        dev = self._dev
        anchor_z, n_anchor, flat = dev._grid_args(anchor_z)
        own_axes = [tuple(int(i) for i in own) for own in own_axes]
        n_own = np.array([len(own) for own in own_axes], dtype=np.int32)
        own_flat = np.array([i for own in own_axes for i in own], dtype=np.int32)
        self._coarse_key = None                 # (bi_factored_begin releases the store's coarse binning)
        dev._check(dev._lib.bi_factored_begin(dev._h, len(anchor_z), ptr(n_anchor), ptr(flat), int(S), int(B), ptr(n_own),
                                              ptr(own_flat) if len(own_flat) else None))
        self.d, self.S, self.B = len(anchor_z), int(S), int(B)
        self.anchor_z, self.own_axes = anchor_z, own_axes
        self.mus = [np.zeros(tuple(len(anchor_z[i]) for i in own)) for own in own_axes]      # host copy of the rates
        self.T = 0
        self._counts = None
        self._binned = None

    def set_anchor(self, s, local_index, ps_row, mu):
        dev = self._dev
        ps_row = as_f64(ps_row).reshape(self.B)
        dev._check(dev._lib.bi_factored_set_anchor(dev._h, int(s), int(local_index), ptr(ps_row), float(mu)))
        self.mus[s].reshape(-1)[int(local_index)] = float(mu)

    def end_model(self):
        self._dev._check(self._dev._lib.bi_factored_end(self._dev._h))

    def set_counts(self, counts):
        """counts: [*bins] (one dataset) or [T, *bins]"""
        dev = self._dev
        c = as_f64(counts)
        if c.size == 0 or c.size % self.B:
            raise ValueError("counts size %d is not a positive multiple of B=%d" % (c.size, self.B))
        T = c.size // self.B
        c = c.reshape(T, self.B)
        dev._check(dev._lib.bi_factored_set_counts(dev._h, T, ptr(c)))
        self._counts = c.copy()
        self.T = T

    def download_counts(self, t=0):
        """dataset t [B] of whatever the store holds: the host copy of uploaded counts, or toys read from the device"""
        if self._counts is not None:
            return self._counts[int(t)].copy()
        dev = self._dev
        out = np.empty(self.B, dtype=np.float64)
        dev._check(dev._lib.bi_sourcewise_download_counts(dev._h, int(t), ptr(out)))
        return out

    def generate_toys_points(self, z, rate_scale=None, n_toys=1, seed=0):
        """Replace the counts by sum(n_toys) toy datasets drawn on the device, n_toys[h] of them at truth (z[h], rate_scale[h]),
        truth-major (bi_sourcewise_generate_toys: always one draw per bin; toy t is toy toy_offset + t of the seed's ensemble).
        -> methods [H]: 0, or -1 for a truth without toys (DeviceContext.generate_toys_points' shape)."""
        dev = self._dev
        n_toys = np.ascontiguousarray(np.atleast_1d(n_toys), dtype=np.int64)
        H = len(n_toys)
        z = np.ascontiguousarray(as_f64(z).reshape(H, self.d)) if self.d else None
        if rate_scale is not None:
            rate_scale = np.ascontiguousarray(np.broadcast_to(as_f64(np.atleast_2d(rate_scale)), (H, self.S)))
        dev._check(dev._lib.bi_sourcewise_generate_toys(dev._h, H, ptr(z), ptr(rate_scale), ptr(n_toys), int(seed) & (2**64 - 1)))
        self._counts = None                     # the toys exist on the device only
        self.T = int(n_toys.sum())
        return np.where(n_toys > 0, 0, -1).astype(np.int32)

    # -- the non-empty-bin form of the data (bi_sourcewise_build_nonempty) ------------------
    def build_nonempty(self):
        """Build the non-empty-bin form of all T datasets of the store as it stands: their lists of bins with events and, per
        dataset, a compacted copy of the model's rows over its list.  While it exists (and the parameter `sourcewise_form` is 1)
        eval, eval_grad, fit_batched, eval_planned and sample_stretch read the listed bins only; every other call keeps reading
        the dense store.  New counts, toys or a new model release it.  -> list lengths [T].  ValueError (BI_ERR_INVALID) when
        the copies would exceed the parameter `compact_budget`: nothing is built then."""
        dev = self._dev
        nnz = np.zeros(max(int(self.T), 1), dtype=np.int64)
        dev._check(dev._lib.bi_sourcewise_build_nonempty(dev._h, ptr(nnz)))
        return nnz[:int(self.T)]

    def drop_nonempty(self):
        """Release the non-empty-bin form: the calls above read the dense store again."""
        self._dev._check(self._dev._lib.bi_sourcewise_drop_nonempty(self._dev._h))

    # -- the event store: unbinned data (bi_sourcewise_score_events, bi_sourcewise_events_begin ...) ------
    def score_events(self, method, grid, coords, outlier_likelihood=0.0):
        """Make T event sets the context's data, scored ON THE DEVICE: the model's rows are density histograms over the analysis
        space, looked up with `method` -- 'piecewise' (grid = the bin edges) or 'linear' (grid = the bin centres; the
        coordinates arrive clipped).  coords: a list of T sets, each a list of k coordinate arrays.  While the store exists
        eval, eval_grad and fit_batched are the extended unbinned likelihood (`dataset` indexes the sets) and every other call
        of this class is refused by the library."""
        dev = self._dev
        grid, n_grid, flat = dev._grid_args(grid)
        k = len(grid)
        sets = [[as_f64(c).ravel() for c in cs] for cs in coords]
        if not sets or any(len(cs) != k or any(len(c) != len(cs[0]) for c in cs) for cs in sets):
            raise ValueError("coords must be a list of event sets, each with one coordinate array per analysis dimension")
        offsets = np.concatenate([[0], np.cumsum([len(cs[0]) for cs in sets])]).astype(np.int64)
        block = np.ascontiguousarray(np.stack([np.concatenate([cs[i] for cs in sets]) for i in range(k)]))
        dev._check(dev._lib.bi_sourcewise_score_events(dev._h, {'piecewise': 0, 'linear': 1}[method], k, ptr(n_grid), ptr(flat), len(sets),
                                                       ptr(offsets), ptr(block), float(outlier_likelihood)))
        self._enter_events(len(sets))

    def set_event_rows(self, n_events, rows, outlier_likelihood=0.0):
        """Make T event sets of n_events [T] events the context's data from pdf values scored on the host: rows(s, local_index)
        -> values [sum(n_events)], set after set, finite or nan, called once per anchor row of every source (C order over
        the source's own axes).  The model's own rows are not read."""
        dev = self._dev
        n_events = np.ascontiguousarray(np.atleast_1d(n_events), dtype=np.int64)
        total = int(n_events.sum())
        dev._check(dev._lib.bi_sourcewise_events_begin(dev._h, len(n_events), ptr(n_events), float(outlier_likelihood)))
        try:
            for s, mus in enumerate(self.mus):
                for local in range(mus.size):
                    v = np.ascontiguousarray(as_f64(rows(s, local)).reshape(total))
                    dev._check(dev._lib.bi_sourcewise_events_set_row(dev._h, s, local, ptr(v) if total else None))
            dev._check(dev._lib.bi_sourcewise_events_end(dev._h))
        except Exception:
            self.drop_events()
            raise
        self._enter_events(len(n_events))

    def _enter_events(self, T):
        if self._binned is None:                # (the counts stay resident beside the store, unread)
            self._binned = (self.T, self._counts)
        self._counts = None
        self.T = T

    def drop_events(self):
        """Release the event store: the context is a binned source-wise model again, with the counts it held before (if any)."""
        self._dev._check(self._dev._lib.bi_sourcewise_drop_events(self._dev._h))
        if self._binned is not None:
            self.T, self._counts = self._binned
            self._binned = None

    def event_set_counts(self):
        """events of every set of the store: [T]"""
        T = int(self.get_param('sourcewise_event_sets'))
        out = np.zeros(max(T, 1), dtype=np.int64)
        self._dev._check(self._dev._lib.bi_sourcewise_event_set_counts(self._dev._h, ptr(out)))
        return out[:T]

    def download_event_set(self, t=0):
        """the stored pdf values of set t: [rows, N_t] (for tests)"""
        n = int(self.event_set_counts()[int(t)])
        out = np.empty((sum(m.size for m in self.mus), n), dtype=np.float64)
        self._dev._check(self._dev._lib.bi_sourcewise_download_event_set(self._dev._h, int(t), ptr(out) if n else None))
        return out

    def simulate_event_toys(self, method, edges, z, rate_scale=None, n_toys=1, seed=0, outlier_likelihood=0.0):
        """Draw sum(n_toys) event-level toys ON THE DEVICE, n_toys[h] of them at truth (z[h], rate_scale[h]), truth-major, and make
        them the context's event sets (bi_sourcewise_simulate_event_toys): the model's rows are density histograms over `edges`
        (k ascending arrays), the events are scored with `method` ('piecewise' or 'linear') as `score_events` scores them.  Toy t
        of the call is toy toy_offset + t (the context parameter) of the seed's ensemble.  -> events per (toy, source) [T, S].
        Everything is validated before the previous store is touched (ValueError)."""
        dev = self._dev
        edges, n_edges, flat = dev._grid_args(edges)
        n_toys = np.ascontiguousarray(np.atleast_1d(n_toys), dtype=np.int64)
        H = len(n_toys)
        z = np.ascontiguousarray(as_f64(z).reshape(H, self.d)) if self.d else None
        if rate_scale is not None:
            rate_scale = np.ascontiguousarray(np.broadcast_to(as_f64(np.atleast_2d(rate_scale)), (H, self.S)))
        T = int(n_toys.sum()) if H and (n_toys >= 0).all() else 0
        counts = np.zeros((max(T, 1), self.S), dtype=np.int64)
        dev._check(dev._lib.bi_sourcewise_simulate_event_toys(dev._h, {'piecewise': 0, 'linear': 1}[method], len(edges), ptr(n_edges), ptr(flat),
                                                              H, ptr(z), ptr(rate_scale), ptr(n_toys), int(seed) & (2**64 - 1),
                                                              float(outlier_likelihood), ptr(counts)))
        self._enter_events(T)
        self._sim_k = len(edges)
        return counts[:T]

    def simulated_event_count(self):
        """events of the resident simulated toys in all; -1 when the store (if any) was not drawn on the device"""
        return int(self._dev._lib.bi_sourcewise_simulated_event_count(self._dev._h))

    def download_events(self):
        """The events `simulate_event_toys` drew, without the padding, set by set -> (coords [k, N], source [N]); their split
        into sets is `event_set_counts()`.  NotPreparedException once another store has replaced the toys."""
        dev = self._dev
        N = self.simulated_event_count()
        if N < 0:
            dev._check(dev._lib.bi_sourcewise_download_events(dev._h, None, None))
        k = self._sim_k
        coords = np.empty((k, max(N, 0)), dtype=np.float64)
        source = np.empty(max(N, 0), dtype=np.int32)
        dev._check(dev._lib.bi_sourcewise_download_events(dev._h, ptr(coords) if N else None, ptr(source) if N else None))
        return coords, source

    # -- evaluation ------------------------------------------------------------------------
    def _point_args(self, z, rate_scale, dataset):
        if self.d:
            z = as_f64(z).reshape(-1, self.d)
            P = len(z)
        else:
            P = 1 if rate_scale is None else len(np.atleast_2d(rate_scale))
            z = None
        if rate_scale is not None:
            rate_scale = np.ascontiguousarray(np.broadcast_to(as_f64(np.atleast_2d(rate_scale)), (P, self.S)))
        if dataset is not None:
            dataset = np.ascontiguousarray(np.broadcast_to(np.asarray(dataset, dtype=np.int64), (P,)))
        return P, z, rate_scale, dataset

    def eval(self, z, rate_scale=None, dataset=None):
        """-> (ll [P], status [P])"""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        ll = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_factored(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), None, ptr(status)))
        return ll, status

    def eval_planned(self, z, rate_scale=None, dataset=None):
        """`eval` with the work items made on the device (bi_eval_sourcewise_planned: the rows are uploaded as they are, the
        planner kernel screens them and writes the descriptors) -> (ll [P], status [P]), bit for bit `eval`'s."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        ll = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_planned(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(status)))
        return ll, status

    def eval_events_planned(self, z, rate_scale=None, dataset=None):
        """`eval_planned` on the event store (bi_eval_sourcewise_events_planned: the planner's event variant, then the event kernel
        of `eval`), `dataset` indexing the event sets -> (ll [P], status [P]), bit for bit `eval`'s on the store.  Without a
        finished store the library refuses."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        ll = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_events_planned(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(status)))
        return ll, status

    def eval_scan(self, z, rate_scale=None, dataset=None):
        """`eval_planned` on the matrix-core scan route (bi_eval_sourcewise_scan): the points are sorted by (cell tuple, dataset)
        on the device and evaluated 16 at a time over the compacted rows of the non-empty-bin form, each group's rows read once
        per strip of bins -> (ll [P], status [P]).  Status words and the -inf of rejected points are `eval_planned`'s bit for
        bit; a live point's ll agrees to rounding, and its bits may depend on the batch (the same call repeats its bits).
        `last_scan_counters` [5]: groups, work items, live points, launches, host reads of the call.  ValueError
        (BI_ERR_INVALID) unless the form is built (`build_nonempty`) and a point reads at most 32 rows."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        ll = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        counters = np.zeros(5, dtype=np.int64)
        dev._check(dev._lib.bi_eval_sourcewise_scan(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(status), ptr(counters)))
        self.last_scan_counters = counters
        return ll, status

    def grid_reduce(self, kind, index, z0, scale0, unit, dataset, n_keep, nodes, term=None, logw=None, chunk=0, route=-1):
        """bi_grid_reduce_sourcewise: DeviceContext.grid_reduce with the source-wise likelihood -- the same arguments and
        return value, and `route`: 0 = one work item per point (the kernels of `eval_planned`), 1 = the matrix-core scan route
        (`eval_scan`), -1 = 1 where the model is eligible (the non-empty-bin form built, at most 32 rows per point), else 0.
        -> (log_marginal [E, K], profile [E, K], argmax [E, K], counters [5]: chunks, evaluations, excluded points, launches,
        the route taken)."""
        dev = self._dev
        rc, out = grid_reduce_call(dev._lib.bi_grid_reduce_sourcewise, 'bi_grid_reduce_sourcewise', dev._h, self.d, self.S, kind, index, z0, scale0,
                                   unit, dataset, n_keep, nodes, term, logw, chunk, 5, extra=(int(route),))
        dev._check(rc)
        return out

    def grid_reduce_events(self, kind, index, z0, scale0, unit, dataset, n_keep, nodes, term=None, logw=None, chunk=0, route=-1):
        """bi_grid_reduce_sourcewise_events: `grid_reduce` on the event store, `dataset` indexing the event sets -- the same
        arguments and return value.  The chunks are evaluated by the kernels of `eval_events_planned` (route 0; -1 takes it);
        route 1 raises ValueError: the matrix-core scan route does not read the event store."""
        dev = self._dev
        rc, out = grid_reduce_call(dev._lib.bi_grid_reduce_sourcewise_events, 'bi_grid_reduce_sourcewise_events', dev._h, self.d, self.S, kind,
                                   index, z0, scale0, unit, dataset, n_keep, nodes, term, logw, chunk, 5, extra=(int(route),))
        dev._check(rc)
        return out

    def sample_stretch(self, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a=2.0, seed=0, first_ensemble=0, priors=None):
        """bi_sample_stretch_sourcewise: DeviceContext.sample_stretch with the source-wise likelihood as the target -- the same
        arguments, random stream and return value (chain [n_steps, E, W, F], ll [n_steps, E, W], n_accepted [E, W], counters),
        `priors` included.  counters has five entries here: half-steps, evaluations, accepted moves, launches, and the stream
        synchronisations inside the step loop (0: the loop is queued without a host wait)."""
        return self._sample_stretch(self._dev._lib.bi_sample_stretch_sourcewise, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a,
                                    seed, first_ensemble, priors)

    def sample_stretch_events(self, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a=2.0, seed=0, first_ensemble=0,
                              priors=None):
        """bi_sample_stretch_sourcewise_events: `sample_stretch` with the event store's likelihood as the target, `dataset`
        indexing the event sets -- the same arguments, random stream and return value; the chain is bit for bit the host engine's
        on the same store.  Without a finished store the library refuses."""
        return self._sample_stretch(self._dev._lib.bi_sample_stretch_sourcewise_events, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi,
                                    n_steps, a, seed, first_ensemble, priors)

    def _sample_stretch(self, call, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a, seed, first_ensemble, priors):
        dev = self._dev
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        E, W2, F = x0.shape
        if W2 != W:
            raise ValueError("x0 must be [E, W, F]")
        kind, index = np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(index, dtype=np.int32)

        def rows(v, n):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1, n), (E, n)))
        z0 = rows(z0, self.d) if self.d else None
        scale0, unit = rows(scale0, self.S), rows(unit, self.S)
        if dataset is not None:
            dataset = np.ascontiguousarray(np.broadcast_to(np.asarray(dataset, dtype=np.int64), (E,)))
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        if len(kind) != F or len(index) != F or len(lo) != F or len(hi) != F:
            raise ValueError("kind, index, lo and hi must have one entry per variable")
        n_steps = int(n_steps)
        chain = np.empty((max(n_steps, 0), E, W, F))
        ll = np.empty((max(n_steps, 0), E, W))
        n_acc = np.zeros((E, W), dtype=np.int64)
        counters = np.zeros(5, dtype=np.int64)
        mean = sigma = const = None
        if priors is not None:
            mean, sigma, const = dev._gauss_terms(priors, F, E)
        dev._check(call(dev._h, E, int(W), F, ptr(kind), ptr(index), ptr(z0), ptr(scale0), ptr(unit), ptr(dataset), ptr(x0), ptr(lo), ptr(hi),
                        n_steps, float(a), int(seed) & (2 ** 64 - 1), int(first_ensemble), ptr(mean), ptr(sigma), ptr(const), ptr(chain), ptr(ll),
                        ptr(n_acc), ptr(counters)))
        return chain, ll, n_acc, counters

    def eval_grad(self, z, rate_scale=None, dataset=None):
        """-> (ll [P], dll/dz [P, d], dll/drate_scale [P, S], status [P])"""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        ll = np.empty(P, dtype=np.float64)
        grad = np.empty((P, self.d + self.S), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_factored(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(grad), ptr(status)))
        return ll, grad[:, :self.d], grad[:, self.d:], status

    def eval_hess(self, z, rate_scale=None, dataset=None):
        """Value, gradient and analytic Hessian (bi_eval_sourcewise_hess) -> (ll [P], dll/dz [P, d], dll/drate_scale [P, S],
        H [P, d + S, d + S] over (z, rate_scale), status [P]): DeviceContext.eval_hess's shapes.  ll, the gradient and the status
        are eval_grad's bits; H is nan wherever ll is not finite."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        F = self.d + self.S
        ll = np.empty(P, dtype=np.float64)
        grad = np.empty((P, F), dtype=np.float64)
        hess = np.empty((P, F, F), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_hess(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(grad), ptr(hess),
                                                    ptr(status)))
        return ll, grad[:, :self.d], grad[:, self.d:], hess, status

    def eval_events_hess(self, z, rate_scale=None, dataset=None):
        """eval_hess on the event store (bi_eval_sourcewise_events_hess): value, gradient and analytic Hessian of the unbinned
        likelihood, `dataset` indexing the event sets -> eval_hess's shapes.  ll, the gradient and the status are eval_grad's
        bits on the store; H is nan wherever ll is not finite.  Without a store the library refuses."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        F = self.d + self.S
        ll = np.empty(P, dtype=np.float64)
        grad = np.empty((P, F), dtype=np.float64)
        hess = np.empty((P, F, F), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_events_hess(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(grad), ptr(hess),
                                                           ptr(status)))
        return ll, grad[:, :self.d], grad[:, self.d:], hess, status

    def eval_gof(self, z, rate_scale=None, dataset=None):
        """Goodness of fit of the data term (bi_eval_sourcewise_gof) -> (half-deviance [P], Pearson chi2 [P], status [P]) of point
        p against dataset[p]; +inf / nan where the likelihood is -inf / nan: DeviceContext.eval_gof's shapes."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        half_deviance = np.empty(P, dtype=np.float64)
        pearson = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_gof(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(half_deviance), ptr(pearson),
                                                   ptr(status)))
        return half_deviance, pearson, status

    def expected_counts(self, z, rate_scale=None, per_source=False):
        """The expectation per bin (bi_sourcewise_expected_counts) -> mu [P, B], or r_s tau_s [P, S, B] per source; nan rows for
        points outside the anchor box or with unphysical rates.  No counts are needed."""
        dev = self._dev
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        out = np.empty((P, self.S, self.B) if per_source else (P, self.B), dtype=np.float64)
        dev._check(dev._lib.bi_sourcewise_expected_counts(dev._h, P, ptr(z), ptr(rate_scale), 1 if per_source else 0, ptr(out)))
        return out

    # -- coarse views: the expectation and the data summed over groups of fine bins (bi_sourcewise_set_coarse_binning ...), under
    #    DeviceContext's names and shapes --
    def set_coarse_binning(self, fine_shape=None, groups=None):
        """The coarse binning of the source-wise store: fine_shape [k] fine bins per analysis axis, groups: per axis the ascending
        fine-bin boundaries e_0 < ... < e_m (`CoarseBinning.groups`) -> the number of cells.  No arguments: clear it.  A new model
        releases it.  ValueError (BI_ERR_INVALID) for boundaries that do not fit the model."""
        dev = self._dev
        cells = C.c_int64(0)
        if fine_shape is None:
            self._coarse_key = None
            dev._check(dev._lib.bi_sourcewise_set_coarse_binning(dev._h, 0, None, None, None, C.byref(cells)))
            return 0
        n_fine = np.ascontiguousarray(fine_shape, dtype=np.int32)
        groups = [np.ascontiguousarray(g, dtype=np.int32).ravel() for g in groups]
        if len(groups) != len(n_fine) or not len(n_fine):
            raise ValueError("need the boundaries of every one of the %d axes" % len(n_fine))
        n_groups = np.array([len(g) - 1 for g in groups], dtype=np.int32)
        bounds = np.ascontiguousarray(np.concatenate(groups), dtype=np.int32)
        # the binning the store holds already (begin_model forgets it, as bi_factored_begin releases it): nothing to build or upload
        key = (n_fine.tobytes(), n_groups.tobytes(), bounds.tobytes())
        if self._coarse_key is not None and self._coarse_key[0] == key:
            return self._coarse_key[1]
        self._coarse_key = None
        dev._check(dev._lib.bi_sourcewise_set_coarse_binning(dev._h, len(n_fine), ptr(n_fine), ptr(n_groups), ptr(bounds), C.byref(cells)))
        self._coarse_key = (key, int(cells.value))
        return int(cells.value)

    def expected_coarse(self, n_cells, z, rate_scale=None, per_source=False):
        """The expectation per cell of the coarse binning (bi_sourcewise_expected_coarse) -> (mu [P, C] or [P, S, C], status [P]);
        nan rows and the status bit for points outside the anchor box or with unphysical rates.  No counts are needed."""
        dev = self._dev
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        out = np.empty((P, self.S, int(n_cells)) if per_source else (P, int(n_cells)), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_sourcewise_expected_coarse(dev._h, P, ptr(z), ptr(rate_scale), 1 if per_source else 0, ptr(out), ptr(status)))
        return out, status

    def expected_coarse_jacobian(self, n_cells, z, rate_scale=None, per_source=False):
        """The expectation per cell of the coarse binning and its first derivatives over theta = (z [d], then rate_scale [S])
        (bi_sourcewise_expected_coarse_jacobian) -> (mu [P, C], jac [P, d + S, C], status [P]), or with per_source
        (mu [P, S, C], jac [P, S, d + S, C]): the single terms of every source, which summed over the sources in ascending order
        in long double give the total rows bit for bit.  The total mu has the bits of `expected_coarse`.  nan throughout and the
        status bit for points outside the anchor box or with unphysical rates.  No counts are needed."""
        dev = self._dev
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        C_, F = int(n_cells), self.d + self.S
        mu = np.empty((P, self.S, C_) if per_source else (P, C_), dtype=np.float64)
        jac = np.empty((P, self.S, F, C_) if per_source else (P, F, C_), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_sourcewise_expected_coarse_jacobian(dev._h, P, ptr(z), ptr(rate_scale), 1 if per_source else 0, ptr(mu),
                                                                   ptr(jac), ptr(status)))
        return mu, jac, status

    def coarse_counts(self, n_cells, datasets=None):
        """The counts of the store's datasets -- uploaded, or toys drawn on the device -- per cell of the coarse binning
        (bi_sourcewise_coarse_counts) -> [n, C]; datasets: indices [n] (None: all T)."""
        dev = self._dev
        if datasets is not None:
            datasets = np.ascontiguousarray(np.atleast_1d(datasets), dtype=np.int64)
        n = int(self.T) if datasets is None else len(datasets)
        out = np.empty((n, int(n_cells)), dtype=np.float64)
        dev._check(dev._lib.bi_sourcewise_coarse_counts(dev._h, n, ptr(datasets), ptr(out)))
        return out

    def eval_fisher(self, z, rate_scale=None):
        """The expected (Fisher) information at P truths, no counts needed (bi_eval_sourcewise_fisher) -> (info [P, d + S, d + S],
        total expectation [P], unbounded [P, d + S], status [P]): DeviceContext.eval_fisher's shapes and meaning."""
        dev = self._dev
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        F = self.d + self.S
        info = np.empty((P, F, F), dtype=np.float64)
        total = np.empty(P, dtype=np.float64)
        unbounded = np.zeros((P, F), dtype=np.int64)
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_fisher(dev._h, P, ptr(z), ptr(rate_scale), ptr(info), ptr(total), ptr(unbounded),
                                                      ptr(status)))
        return info, total, unbounded, status

    def fit_batched(self, P, F, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks, gtol, max_iter, x, f, flags, counters,
                    priors=None):
        """bi_fit_batched_factored: DeviceContext.fit_batched with the source-wise likelihood as the objective"""
        dev = self._dev
        mean = sigma = const = None
        if priors is not None:
            mean, sigma, const = dev._gauss_terms(priors, int(F), int(P))
        dev._check(dev._lib.bi_fit_batched_factored(dev._h, int(P), int(F), ptr(kind), ptr(index), ptr(z0) if self.d else None, ptr(scale0),
                                                    ptr(unit), ptr(dataset), ptr(x0), ptr(lo), ptr(hi), ptr(n_kinks), ptr(kinks), float(gtol),
                                                    int(max_iter), ptr(mean), ptr(sigma), ptr(const), ptr(x), ptr(f), ptr(flags), ptr(counters)))
        return 0

    # -- real-valued datasets: a store of its own beside the counts (bi_sourcewise_set_real_counts ... bi_fit_batched_sourcewise_real),
    #    under the names DeviceContext uses, so that blueice_amd.asimov's context proxy works over either --
    def set_real_counts(self, counts):
        """counts: [*bins] (one set) or [T, *bins], every count finite and >= 0 (ValueError otherwise); None drops the store."""
        dev = self._dev
        if counts is None:
            dev._check(dev._lib.bi_sourcewise_set_real_counts(dev._h, 0, None))
            return
        c = as_f64(counts)
        if c.size == 0 or c.size % self.B:
            raise ValueError("counts size %d is not a positive multiple of B=%d" % (c.size, self.B))
        T = c.size // self.B
        dev._check(dev._lib.bi_sourcewise_set_real_counts(dev._h, T, ptr(c.reshape(T, self.B))))

    def set_asimov_counts(self, z, rate_scale=None):
        """H Asimov datasets made on the device (bi_sourcewise_set_asimov_counts): set h holds the expectation at truth (z[h],
        rate_scale[h]), bit for bit the row of `expected_counts`.  ValueError names a truth outside the anchor box, with
        unphysical rates or with an expectation that is not finite; the previous store then stays.  -> H"""
        dev = self._dev
        H, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        dev._check(dev._lib.bi_sourcewise_set_asimov_counts(dev._h, H, ptr(z), ptr(rate_scale)))
        return H

    @property
    def real_count_sets(self):
        return int(self._dev._lib.bi_sourcewise_real_count_sets(self._dev._h))

    def download_real_counts(self, t=0):
        dev = self._dev
        out = np.empty(self.B, dtype=np.float64)
        dev._check(dev._lib.bi_sourcewise_download_real_counts(dev._h, int(t), ptr(out)))
        return out

    def eval_real(self, z, rate_scale=None, dataset=None, gradient=True):
        """Half-deviance against the real-valued store (bi_eval_sourcewise_real) -> (half_deviance [P], d/dz [P, d],
        d/drate_scale [P, S], status [P]); gradient=False: the two slope arrays are None.  +inf outside the box / for unphysical
        rates / where a filled bin expects nothing: DeviceContext.eval_real's shapes and meaning."""
        dev = self._dev
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        half = np.empty(P, dtype=np.float64)
        grad = np.empty((P, self.d + self.S), dtype=np.float64) if gradient else None
        status = np.zeros(P, dtype=np.int32)
        dev._check(dev._lib.bi_eval_sourcewise_real(dev._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(half), ptr(grad), ptr(status)))
        if not gradient:
            return half, None, None, status
        return half, grad[:, :self.d], grad[:, self.d:], status

    def fit_batched_real(self, P, F, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks, gtol, max_iter, x, f, flags, counters,
                         priors=None):
        """bi_fit_batched_sourcewise_real: `fit_batched` with f = half_deviance - p against the real-valued store."""
        dev = self._dev
        mean = sigma = const = None
        if priors is not None:
            mean, sigma, const = dev._gauss_terms(priors, int(F), int(P))
        dev._check(dev._lib.bi_fit_batched_sourcewise_real(dev._h, int(P), int(F), ptr(kind), ptr(index), ptr(z0) if self.d else None,
                                                           ptr(scale0), ptr(unit), ptr(dataset), ptr(x0), ptr(lo), ptr(hi), ptr(n_kinks),
                                                           ptr(kinks), float(gtol), int(max_iter), ptr(mean), ptr(sigma), ptr(const), ptr(x),
                                                           ptr(f), ptr(flags), ptr(counters)))
        return 0

    def interpolate(self, which, z):
        """'mus': the interpolated rates [S] at z [d], from the host copy of the anchors' rates"""
        if which != 'mus':
            raise NotImplementedError("a source-wise model interpolates 'mus' only (the morphed templates are never materialised)")
        z = np.asarray(z, dtype=float).reshape(self.d)
        out = np.zeros(self.S)
        for s, own in enumerate(self.own_axes):
            cells = [_find_cell(self.anchor_z[i], z[i]) for i in own]
            v = 0.0
            for c in range(1 << len(own)):
                w, idx = 1.0, []
                for j, (k, t) in enumerate(cells):
                    up = (c >> (len(own) - 1 - j)) & 1
                    idx.append(k + up)
                    w = w * (t if up else 1 - t)
                v = v + self.mus[s][tuple(idx)] * w
            out[s] = v
        return out


# the bound names that stay refused although the layer behind them exists, and the spellings that work
_REFUSED_SPELLINGS = {
    'hesse': "blueice_amd.inference.hesse(lf, values) (or lf.bestfit_minuit for the errors of a fit)",
    'fisher_information': "lf.fisher_information_points(points), lf.expected_covariance(**truth) or lf.expected_errors(**truth)",
    'simulate_toys': "lf.simulate_toys_points(points, n_toys, seed) with one-row arrays in `points`",
    'bestfit_toys': "blueice_amd.inference.bestfit_toys(lf, ...)",
    'toy_mc_fits': "blueice_amd.inference.toy_mc_fits(lf, n_toys, ...)",
    'gof_statistics': "blueice_amd.inference.gof_statistics(lf, points, datasets=...)",
    'goodness_of_fit': "blueice_amd.inference.goodness_of_fit(lf, n_toys=...)",
    'expected_counts': "blueice_amd.inference.expected_counts_points(lf, points, per_source=) with one-row arrays in `points`",
    'expected_counts_points': "blueice_amd.inference.expected_counts_points(lf, points, per_source=)",
    'expected_coarse': "blueice_amd.coarse.expected_coarse(lf, binning, **params)",
    'expected_coarse_points': "blueice_amd.coarse.expected_coarse_points(lf, binning, points)",
    'coarse_counts': "blueice_amd.coarse.coarse_counts(lf, binning, datasets=)",
    'expected_coarse_jacobian': "blueice_amd.coarse.sourcewise_coarse_jacobian(lf, binning, per_source=, **params)",
    'expected_coarse_jacobian_points': "blueice_amd.coarse.sourcewise_coarse_jacobian_points(lf, binning, points, per_source=)",
    'expected_coarse_band': "blueice_amd.coarse.sourcewise_coarse_band(lf, binning, names, covariance, **params)",
    'coarse_information': "blueice_amd.coarse.sourcewise_coarse_information(lf, binning, **truth)",
    'asimov': "blueice_amd.asimov.asimov(lf, **truth)",
    'real_data': "blueice_amd.asimov.real_data(lf, counts)",
    'expected_upper_limit': "blueice_amd.inference.expected_upper_limit(lf, target, bound)",
    'sample_posterior': "blueice_amd.sampler.sample_posterior(lf, n_walkers=, n_steps=, ...)",
    'bestfit_emcee': "blueice_amd.inference.bestfit_emcee(lf, ...) (or blueice_amd.sampler.sample_posterior(lf, ...) for the chain)",
}


def _refused(name):
    def method(self, *args, **kwargs):
        if name in _REFUSED_SPELLINGS:
            raise NotImplementedError("lf.%s is not bound on a source-wise model (SourceWiseBinnedLogLikelihood); call %s"
                                      % (name, _REFUSED_SPELLINGS[name]))
        raise NotImplementedError("%s is not available for a source-wise model (SourceWiseBinnedLogLikelihood): value, gradient, "
                                  "Hessian, expected information, the fit, scan and interval layers, toys at truth points, "
                                  "goodness of fit, coarse views, Asimov data and the ensemble sampler are, and gridded likelihoods "
                                  "as blueice_amd.grid.grid_scan(lf, ...)" % name)
    method.__name__ = name
    return method


class _SourceWiseLikelihood(DeviceLogLikelihood):
    """What the binned and the unbinned source-wise likelihood share: the context, the models at the projected anchors and the
    upload of one row per own anchor of every source, and the single-point call."""

    supports_gradient = True

    def __init__(self, pdf_base_config, likelihood_config=None, **kwargs):
        super().__init__(pdf_base_config, likelihood_config, **kwargs)
        self.source_wise_interpolation = True
        if self.config.get('model_statistical_uncertainty_handling') is not None:
            raise NotImplementedError("Beeston-Barlow (model_statistical_uncertainty_handling) is not available for a source-wise model")

    def _context(self):
        if self.ctx is None:
            self.ctx = SourceWiseContext(self.config.get('device'))
        return self.ctx

    def _template_building(self):
        from contextlib import nullcontext
        if not self.config.get('device_histograms', True):
            return nullcontext()
        return device_histograms(self._context(), self.config.get('device_histograms_min_events', 32768))

    def _build_projected_anchors(self, n_cores):
        """The limits, then models at the anchors some source needs only (one per distinct projection of a source's own anchors:
        `_build_source_anchors`).  The product grid of all shape parameters is never enumerated."""
        names = list(self.shape_parameters)
        own_params = self.source_shape_parameters
        if any(self.source_allowed_negative):
            raise NotImplementedError("sources that may go negative (allow_negative) are not available for a source-wise model")
        if len(names) > MAX_SHAPE_PARAMETERS or len(self.source_name_list) > MAX_SOURCES:
            raise ValueError("a source-wise model takes at most %d shape parameters and %d sources (got %d and %d)"
                             % (MAX_SHAPE_PARAMETERS, MAX_SOURCES, len(names), len(self.source_name_list)))
        for name, own in own_params.items():
            if len(own) > MAX_OWN_PARAMETERS:
                raise ValueError("source %s responds to %d shape parameters (%s); a source-wise model takes at most %d per source: a source "
                                 "that responds to more belongs on the full grid (%s)"
                                 % (name, len(own), ', '.join(own), MAX_OWN_PARAMETERS, self._full_grid_class))
        self.anchor_models = OrderedDict()
        self.morpher = None
        self.anchor_sources = OrderedDict()
        if own_params:
            self._build_source_anchors(self._anchor_model_builder(n_cores))

    def _own_sources(self, s):
        """the Source objects of source s at its own anchors, in the order of its rows on the device (the source's own morpher
        lists its anchors in C order over its own parameters, each ascending)"""
        name = self.source_name_list[s]
        if name in self.anchor_sources:
            return list(self.anchor_sources[name].values())
        return [self.base_model.sources[s]]

    def _upload_source_rows(self, n_bins, row_of):
        """begin_model ... end_model: row_of(source) -> the [n_bins] row of a Source at one of its own anchors"""
        names = list(self.shape_parameters)
        own_params = self.source_shape_parameters
        anchor_z = [np.array(sorted(anchors.keys()), dtype=float) for anchors, _, _ in self.shape_parameters.values()]
        own_axes = [tuple(names.index(k) for k in own_params.get(name, ())) for name in self.source_name_list]
        ctx = self._context()
        ctx.begin_model(anchor_z, len(self.source_name_list), n_bins, own_axes)
        for s in range(len(self.source_name_list)):
            for local, source in enumerate(self._own_sources(s)):
                ctx.set_anchor(s, local, row_of(source), source.expected_events)
        ctx.end_model()

    @_needs_data
    def __call__(self, livetime_days=None, compute_pdf=False, full_output=False, **kwargs):
        if compute_pdf or full_output:
            raise NotImplementedError("a source-wise model (%s) evaluates the morphed model only: no "
                                      "compute_pdf=True / full_output=True" % type(self).__name__)
        prior, zs, scale = self._host_terms(livetime_days, kwargs)
        if prior is None:
            return -float('inf')
        ll, st = self.ctx.eval(zs if len(zs) else None, scale[None, :])
        return self._finish_call(prior, zs, scale, float(ll[0]), int(st[0]))

    def _call_begin(self, livetime_days=None, **kwargs):
        return self(livetime_days=livetime_days, **kwargs)

    def _call_end(self, token):
        return token


class SourceWiseBinnedLogLikelihood(_SourceWiseLikelihood):
    """Binned Poisson likelihood whose sources each morph over their own shape parameters (see the module's docstring)."""

    _full_grid_class = 'BinnedLogLikelihood'

    _REFUSED = ('best_anchor', 'bestfit_toys', 'toy_mc_fits', 'expected_counts',
                'expected_counts_points', 'gof_statistics', 'goodness_of_fit', 'expected_coarse', 'expected_coarse_points', 'coarse_counts',
                'expected_coarse_jacobian', 'expected_coarse_jacobian_points', 'expected_coarse_band', 'coarse_information',
                'expected_upper_limit',
                'fisher_information', 'hesse', 'sample_posterior', 'bestfit_emcee',
                'grid_scan', 'asimov', 'real_data', 'simulate_toys', 'eval_toys', 'eval_toys_points',
                'ps_interpolator', 'n_model_events_interpolator')

    toys_through_points = True      # inference draws its toys with simulate_toys_points (the bound simulate_toys stays refused)

    @property
    def supports_hessian(self):
        """True once data are set: the analytic Hessian of bi_eval_sourcewise_hess (`hessian_method` is 'analytic')"""
        return self.ctx is not None and bool(self.is_data_set)

    def __init__(self, pdf_base_config, likelihood_config=None, **kwargs):
        super().__init__(pdf_base_config, likelihood_config, **kwargs)
        self._binned = None

    # -- lifecycle -------------------------------------------------------------------------
    def prepare(self, n_cores=1, ipp_client=None):
        """Models at the anchors some source needs only (one per distinct projection of a source's own anchors), then every
        source's rows streamed to the device from there.  The product grid of all shape parameters is never enumerated."""
        self._build_projected_anchors(n_cores)
        self.ps, self.n_model_events = self.base_model.pmf_grids()
        self.bin_shape = self.ps.shape[1:]
        self._upload_source_rows(int(np.prod(self.bin_shape, dtype=np.int64)), lambda source: source.get_pmf_grid()[0])
        self._binned = None
        self.is_data_set = False
        self.is_prepared = True

    def _rebuild_nonempty(self):
        """likelihood_config['nonempty_bins'] after the counts have changed (new counts release the form): False (default) never
        builds it, True always, 'auto' when at most a quarter of the bins of all datasets hold events (the grid model's rule).
        -> whether the form is built"""
        setting = self.config.get('nonempty_bins', False)
        if setting is None or setting is False:
            return False
        ctx = self.ctx
        if setting is True:
            ctx.build_nonempty()
            return True
        if setting != 'auto':
            raise ValueError("likelihood_config['nonempty_bins'] is False, True or 'auto', not %r" % (setting,))
        bins = int(ctx.T) * int(ctx.B)
        if ctx._counts is not None:                     # uploaded counts: the host copy says
            if 4 * int(np.count_nonzero(ctx._counts)) > bins:
                return False
            ctx.build_nonempty()
            return True
        try:                                            # toys on the device: the build counts them
            nnz = ctx.build_nonempty()
        except ValueError:                              # (beyond compact_budget: stay dense)
            return False
        if 4 * int(np.sum(nnz)) > bins:
            ctx.drop_nonempty()
            return False
        return True

    @_needs_preparation
    def set_data(self, d):
        """Bin the events of `d` in the analysis space on the device (numpy.histogramdd semantics) and make the counts
        dataset 0."""
        LogLikelihoodBase.set_data(self, d)
        edges = [e for _, e in self.base_model.config['analysis_space']]
        self.ctx.set_counts(self.ctx.histogram_events(edges, self.base_model.to_analysis_dimensions(d)))
        self._binned = None
        self._rebuild_nonempty()

    @_needs_preparation
    def set_binned_data(self, counts):
        """Upload already-binned counts: [*bins] or [T, *bins] for T datasets.  Dataset 0 is what plain `lf(**params)`
        evaluates."""
        counts = np.asarray(counts, dtype=float)
        if counts.shape[-len(self.bin_shape):] != tuple(self.bin_shape):
            raise ValueError("counts must end in the analysis-space shape %s" % (tuple(self.bin_shape),))
        self._data = None
        self.ctx.set_counts(counts)
        self._binned = None
        self.is_data_set = True
        self._rebuild_nonempty()

    @property
    def data_events_per_bin(self):
        if self._binned is None:
            names, edges = zip(*self.base_model.config['analysis_space'])
            self._binned = Histdd(bins=edges, axis_names=names)
            self._binned.histogram = self.ctx.download_counts(0).reshape(self.bin_shape)
        return self._binned

    @_needs_preparation
    def simulate_toys_points(self, points, n_toys, seed=0, livetime_days=None):
        """Draw toys ON THE DEVICE at H truth points in one generator call (bi_sourcewise_generate_toys) and make them the
        likelihood's data: n_toys[h] toys (an int: the same number everywhere) at truth h, truth-major.  points: dict parameter
        name -> array [H] (scalars broadcast; absent parameters take their defaults), as `eval_points`.  Per bin n ~ Poisson(mu_b),
        always one draw per bin; toy t of the call is toy `toy_offset + t` (the context parameter) of the seed's ensemble, so an
        ensemble over many hypotheses does not depend on how they are grouped into calls -- `BinnedLogLikelihood
        .simulate_toys_points`' contract.  Afterwards `toy_truth` [T] holds the truth index of every dataset.
        -> methods [H]: 0 = drawn bin by bin, -1 = no toys."""
        z, scale, _ = self._batch_terms(points, livetime_days)
        H = max(len(z), np.size(n_toys))
        n_toys = np.ascontiguousarray(np.broadcast_to(np.asarray(n_toys, dtype=np.int64), (H,)))
        z, scale = np.broadcast_to(z, (H, z.shape[1])), np.broadcast_to(scale, (H, scale.shape[1]))
        for i, name in enumerate(self.shape_parameters):
            lo, hi = self.get_bounds(name)
            outside = np.flatnonzero(~((z[:, i] >= lo) & (z[:, i] <= hi)))
            if len(outside):
                raise ValueError("cannot simulate outside the anchor box (truth %d: %s = %r)" % (outside[0], name, z[outside[0], i]))
        methods = self.ctx.generate_toys_points(z if z.shape[1] else None, scale, n_toys, seed)
        self._data = None
        self._binned = None
        self.is_data_set = True
        self.toy_truth = np.repeat(np.arange(H), n_toys)
        self._rebuild_nonempty()
        return methods

    # -- evaluation ------------------------------------------------------------------------
    @_needs_data
    def eval_points_scan(self, points, livetime_days=None, dataset=None):
        """`eval_points` on the matrix-core scan route (bi_eval_sourcewise_scan; see the module's docstring): for batches whose
        points pile up in few cell tuples.  The same arguments, return value and treatment of rejected points; the values agree
        with `eval_points` to rounding, and a point's bits may depend on the batch.  ValueError unless the non-empty-bin form
        is built (likelihood_config['nonempty_bins']) and a point reads at most 32 rows."""
        z, scale, prior = self._batch_terms(points, livetime_days)
        ll, st = self.ctx.eval_scan(z if z.shape[1] else None, scale, dataset)
        bad = st & _capi.ST_UNPHYSICAL
        if np.any(bad) and self.config.get('unphysical_behaviour') == 'error':
            raise ValueError("Unphysical rates at %d of %d points" % (int(np.count_nonzero(bad)), len(st)))
        out = ll + prior
        out[(st & (_capi.ST_OUT_OF_BOUNDS | _capi.ST_UNPHYSICAL)) != 0] = -np.inf
        return out


for _name in SourceWiseBinnedLogLikelihood._REFUSED:
    setattr(SourceWiseBinnedLogLikelihood, _name, _refused(_name))
