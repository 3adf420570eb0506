"""Thin object wrapper over the C ABI (include/blueice_hip.h): one `DeviceContext` = one GPU + stream.

Everything numerical happens in libblueice_hip.so; this module only marshals numpy arrays.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import as_f64, ptr
from .exceptions import DeviceError, NotPreparedException, PlannerRefused

__all__ = ['DeviceContext', 'DeviceBuffer', 'EvalPlan', 'default_device']


def default_device():
    """LOCAL_RANK when launched by torch.distributed.run (one process per GPU), else 0."""
    return int(os.environ.get('BLUEICE_AMD_DEVICE', os.environ.get('LOCAL_RANK', 0)))


class DeviceContext:
    """Owns the anchor tensors and binned data of one likelihood in HBM."""

    def __init__(self, device=None):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        device = default_device() if device is None else int(device)
        rc = self._lib.bi_create(device, C.byref(self._h))
        if rc != 0:
            raise DeviceError("bi_create(device=%d) failed: %s" % (
                device, self._lib.bi_last_error(None).decode()))
        self.device = device
        self._one_out, self._one_st, self._one_ds = C.c_double(), C.c_int32(), C.c_int64()
        self.d = self.S = self.B = None
        self.T = 0
        self.bb_source = -1

    # -- plumbing --------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.bi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == 0:
            return
        msg = self._lib.bi_last_error(self._h).decode()
        if rc == _capi.ERR_STATE:
            raise NotPreparedException(msg)
        if rc == _capi.ERR_INVALID:
            raise ValueError(msg)
        raise DeviceError("libblueice_hip error %d: %s" % (rc, msg))

    def info(self):
        name = C.create_string_buffer(256)
        arch = C.create_string_buffer(256)
        ncu = C.c_int()
        hbm = C.c_int64()
        self._check(self._lib.bi_device_info(self._h, name, arch, 256, C.byref(ncu), C.byref(hbm)))
        return dict(name=name.value.decode(), arch=arch.value.decode(), n_cu=ncu.value, hbm_bytes=hbm.value)

    def set_param(self, name, value):
        self._check(self._lib.bi_set_param(self._h, name.encode(), int(value)))

    def get_param(self, name):
        v = int(self._lib.bi_get_param(self._h, name.encode()))
        if v == -2 ** 63:                      # INT64_MIN: no such (readable) parameter -- never a plausible number
            raise ValueError(self._lib.bi_last_error(self._h).decode())
        return v

    def list_params(self):
        """-> {name: 'rw' | 'r' | 'w'} of every tunable, counter and trigger of the library."""
        n = self._lib.bi_list_params(None, 0)
        buf = C.create_string_buffer(n)
        self._lib.bi_list_params(buf, n)
        return dict(line.split() for line in buf.value.decode().splitlines())

    def sync(self):
        self._check(self._lib.bi_sync(self._h))

    @property
    def stream(self):
        return self._lib.bi_stream(self._h)

    # -- model -----------------------------------------------------------------------------
    def _grid_args(self, anchor_z):
        anchor_z = [np.ascontiguousarray(g, dtype=np.float64) for g in anchor_z]
        n_anchor = np.array([len(g) for g in anchor_z], dtype=np.int32)
        flat = np.concatenate(anchor_z) if len(anchor_z) else np.zeros(0)
        return anchor_z, n_anchor, np.ascontiguousarray(flat, dtype=np.float64)

    def upload_model(self, anchor_z, ps, mus, n_model=None, bb_source=-1):
        """anchor_z: list of d ascending arrays; ps [A.., S, *bins]; mus [A.., S]; n_model like ps."""
        anchor_z, n_anchor, flat = self._grid_args(anchor_z)
        d = len(anchor_z)
        grid_shape = tuple(int(n) for n in n_anchor)
        ps = np.asarray(ps)
        if ps.ndim < d + 2 and not (ps.ndim == d + 1):
            raise ValueError("ps must have shape [A.., S, *bins]")
        S = int(ps.shape[d])
        B = int(np.prod(ps.shape[d + 1:], dtype=np.int64)) if ps.ndim > d + 1 else 1
        ps = as_f64(ps).reshape(grid_shape + (S, B))
        mus = as_f64(mus, grid_shape + (S,))
        if n_model is not None:
            n_model = as_f64(n_model).reshape(grid_shape + (S, B))
        self._check(self._lib.bi_upload_model(self._h, d, ptr(n_anchor), ptr(flat), S, B, ptr(ps), ptr(mus),
                                              ptr(n_model), int(bb_source)))
        self.d, self.S, self.B, self.bb_source = d, S, B, int(bb_source)
        self.anchor_z = anchor_z
        self.T = 0

    def begin_model(self, anchor_z, S, B, bb_source=-1):
        anchor_z, n_anchor, flat = self._grid_args(anchor_z)
        self._check(self._lib.bi_model_begin(self._h, len(anchor_z), ptr(n_anchor), ptr(flat), int(S), int(B),
                                             int(bb_source)))
        self.d, self.S, self.B, self.bb_source = len(anchor_z), int(S), int(B), int(bb_source)
        self.anchor_z = anchor_z
        self.T = 0

    def set_anchor(self, anchor_index, ps, mus, n_model_row=None):
        ps = as_f64(ps).reshape(self.S, self.B)
        mus = as_f64(mus, (self.S,))
        if n_model_row is not None:
            n_model_row = as_f64(n_model_row).reshape(self.B)
        self._check(self._lib.bi_model_set_anchor(self._h, int(anchor_index), ptr(ps), ptr(mus), ptr(n_model_row)))

    def end_model(self):
        self._check(self._lib.bi_model_end(self._h))

    def bb_totals(self, new=None):
        """Per-anchor sums of the Beeston-Barlow source's MC counts; pass `new` to overwrite them with the
        globally reduced values when the bins are sharded over ranks."""
        n_anchor = int(np.prod([len(g) for g in self.anchor_z], dtype=np.int64)) if self.anchor_z else 1
        if new is None:
            out = np.empty(n_anchor, dtype=np.float64)
            self._check(self._lib.bi_get_bb_totals(self._h, ptr(out)))
            return out
        new = as_f64(new, (n_anchor,))
        self._check(self._lib.bi_set_bb_totals(self._h, ptr(new)))
        return new

    def set_allow_negative(self, flags):
        flags = np.ascontiguousarray(flags, dtype=np.int32)
        if flags.shape != (self.S,):
            raise ValueError("need one flag per source")
        self._check(self._lib.bi_set_allow_negative(self._h, ptr(flags)))

    # -- data ------------------------------------------------------------------------------
    def upload_counts(self, counts):
        """counts: [*bins] (one dataset) or [T, *bins]."""
        c = as_f64(counts)
        if c.size % self.B:
            raise ValueError("counts size %d is not a multiple of B=%d" % (c.size, self.B))
        T = c.size // self.B
        c = c.reshape(T, self.B)
        self._check(self._lib.bi_upload_counts(self._h, T, ptr(c)))
        self.T = T

    def set_analysis_space(self, edges):
        """edges: one ascending array of bin edges per analysis dimension."""
        edges = [np.ascontiguousarray(e, dtype=np.float64) for e in edges]
        n_edges = np.array([len(e) for e in edges], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(edges))
        self._check(self._lib.bi_set_analysis_space(self._h, len(edges), ptr(n_edges), ptr(flat)))
        self.space_dims = len(edges)

    def upload_events(self, *coords):
        """Bin events (one coordinate array per analysis dimension) on the device into dataset 0."""
        cols = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64).ravel() for c in coords]))
        if cols.shape[0] != self.space_dims:
            raise ValueError("need %d coordinate arrays" % self.space_dims)
        self._check(self._lib.bi_upload_events(self._h, cols.shape[1], ptr(cols)))
        self.T = 1

    def histogram_events(self, edges, coords):
        """numpy.histogramdd(events, bins=edges)[0] on the device, independent of the context's model and data:
        edges = one ascending array per axis, coords = one coordinate array per axis -> counts [*bins] (float64)."""
        edges = [np.ascontiguousarray(e, dtype=np.float64) for e in edges]
        cols = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64).ravel() for c in coords]))
        if cols.shape[0] != len(edges):
            raise ValueError("need %d coordinate arrays" % len(edges))
        n_edges = np.array([len(e) for e in edges], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(edges))
        counts = np.empty([len(e) - 1 for e in edges], dtype=np.float64)
        self._check(self._lib.bi_histogram_events(self._h, len(edges), ptr(n_edges), ptr(flat), cols.shape[1], ptr(cols),
                                                  ptr(counts)))
        return counts

    @staticmethod
    def _axes_args(method, axes):
        """-> (method code, number of axes k, values per axis [k], the values of all axes back to back)"""
        code = {'piecewise': 0, 'linear': 1}[method]
        axes = [np.ascontiguousarray(a, dtype=np.float64) for a in axes]
        n = np.array([len(a) for a in axes], dtype=np.int32)
        return code, len(axes), n, np.ascontiguousarray(np.concatenate(axes))

    def _made_unbinned(self, target, B, T):
        """`target` now holds this context's model as an unbinned one: B columns (those of its first event set), T event sets"""
        target.d, target.S, target.B, target.bb_source, target.T = self.d, self.S, int(B), -1, int(T)
        target.anchor_z = self.anchor_z

    def score_events(self, target, method, grid, coords, outlier_likelihood=1e-12):
        """This context holds density histograms as its model rows: evaluate all of them at the events and make the
        result the (unbinned) model of `target` -- `Model.score_events` for every anchor, on the device.
        method 'piecewise' (grid = bin edges per axis) or 'linear' (grid = bin centres per axis; coords clipped to
        them and finite)."""
        code, k, n_grid, flat = self._axes_args(method, grid)
        cols = np.ascontiguousarray(np.stack([np.asarray(c, dtype=np.float64).ravel() for c in coords]))
        if cols.shape[0] != k:
            raise ValueError("need %d coordinate arrays" % k)
        target._check(self._lib.bi_score_events(self._h, target._h, code, k, ptr(n_grid), ptr(flat), cols.shape[1],
                                                ptr(cols), float(outlier_likelihood)))
        self._made_unbinned(target, cols.shape[1], 1)

    def simulate_events(self, target, method, edges, z, rate_scale=None, seed=0, outlier_likelihood=1e-12):
        """This context holds density histograms as its model rows: draw an event-level toy dataset from them at (z,
        rate_scale) on the device -- `Model.simulate` for histogram-pdf sources -- and make it the (unbinned) data of
        `target`, scored at every anchor model, without a host hop.  edges: the bin edges of every analysis dimension.
        -> events per source [S]."""
        code, k, n_edges, flat = self._axes_args(method, edges)
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        per_source = np.zeros(self.S, dtype=np.int64)
        target._check(self._lib.bi_simulate_events(self._h, target._h, ptr(z), ptr(rate_scale), code, k, ptr(n_edges),
                                                   ptr(flat), int(seed) & (2**64 - 1), float(outlier_likelihood), ptr(per_source)))
        self._made_unbinned(target, per_source.sum(), 1)
        target._sim_dims = k
        return per_source

    def score_event_sets(self, target, method, grid, coord_sets, outlier_likelihood=1e-12):
        """`score_events` for a stack of T datasets: coord_sets = T lists of coordinate arrays (one per analysis dimension).
        `target` then holds the T event sets side by side (bi_score_event_sets); its dataset t is set t."""
        code, k, n_grid, flat = self._axes_args(method, grid)
        sets = [np.stack([np.asarray(c, dtype=np.float64).ravel() for c in cs]).reshape(k, -1) for cs in coord_sets]
        offsets = np.concatenate([[0], np.cumsum([x.shape[1] for x in sets])]).astype(np.int64)
        cols = np.ascontiguousarray(np.concatenate(sets, axis=1))
        target._check(self._lib.bi_score_event_sets(self._h, target._h, code, k, ptr(n_grid), ptr(flat), len(sets), ptr(offsets),
                                                    ptr(cols), float(outlier_likelihood)))
        self._made_unbinned(target, sets[0].shape[1], len(sets))

    def simulate_event_toys(self, target, method, edges, z, rate_scale=None, n_toys=1, seed=0, outlier_likelihood=1e-12):
        """`simulate_events` for an ensemble: n_toys toys at (z, rate_scale), toy t of the call being toy toy_offset + t (the
        TARGET's parameter) of the seed's ensemble = `simulate_events` with the seed `toy_seed(seed, toy_offset + t)`.
        -> events per toy and source [T, S]."""
        code, k, n_edges, flat = self._axes_args(method, edges)
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        counts = np.zeros((int(n_toys), self.S), dtype=np.int64)
        target._check(self._lib.bi_simulate_event_toys(self._h, target._h, ptr(z), ptr(rate_scale), code, k, ptr(n_edges),
                                                       ptr(flat), int(n_toys), int(seed) & (2**64 - 1), float(outlier_likelihood),
                                                       ptr(counts)))
        self._made_unbinned(target, counts[0].sum(), n_toys)
        target._sim_dims = k
        return counts

    def adopt_event_sets(self, counts):
        """After `set_unbinned` on a model whose columns hold T event sets side by side (even starts): declare them."""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self._check(self._lib.bi_set_event_sets(self._h, len(counts), ptr(counts)))
        self.T, self.B = len(counts), int(counts[0])

    def event_set_offsets(self):
        """-> first column of every event set of this (unbinned) context and, last, the columns in use: [T + 1]."""
        T = int(self._lib.bi_event_set_count(self._h))
        if T < 1:
            raise NotPreparedException("the context holds no unbinned data")
        out = np.zeros(T + 1, dtype=np.int64)
        self._check(self._lib.bi_event_set_offsets(self._h, ptr(out)))
        return out

    def event_set_counts(self):
        """-> events of every event set of this (unbinned) context: [T]."""
        T = int(self._lib.bi_event_set_count(self._h))
        if T < 1:
            raise NotPreparedException("the context holds no unbinned data")
        out = np.zeros(T, dtype=np.int64)
        self._check(self._lib.bi_event_set_counts(self._h, ptr(out)))
        return out

    def download_event_set(self, t=0):
        """-> the resident pdf values of event set t, [anchors, S, N_t]."""
        n = int(self.event_set_counts()[t])
        A = int(np.prod([len(a) for a in self.anchor_z], dtype=np.int64)) if self.d else 1
        out = np.empty((A, self.S, n), dtype=np.float64)
        self._check(self._lib.bi_download_event_set(self._h, int(t), ptr(out)))
        return out

    def download_events(self):
        """The events of the last simulate_events into this context -> (coords [k, N], source index [N])."""
        n = int(self._lib.bi_simulated_event_count(self._h))
        if n < 0:
            raise NotPreparedException("no simulated events are resident")
        coords = np.empty((self._sim_dims, n), dtype=np.float64)
        source = np.empty(n, dtype=np.int32)
        self._check(self._lib.bi_download_events(self._h, ptr(coords), ptr(source)))
        return coords, source

    def set_unbinned(self, outlier_likelihood=1e-12):
        """Treat the uploaded rows as pdf values at the events: extended unbinned likelihood."""
        self._check(self._lib.bi_set_unbinned(self._h, float(outlier_likelihood)))
        self.T = 1

    def counts_to_dense(self):
        """Device-generated toys (non-empty-bin lists) also as the dense [T][B] array, for the paths that visit every bin
        (Beeston-Barlow, sparse = 0)."""
        self._check(self._lib.bi_counts_to_dense(self._h))

    def generate_toys(self, z, rate_scale=None, T=1, seed=0):
        """Replace the data by T Poisson toy datasets drawn on the device at parameter point (z, rate_scale)."""
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        self._check(self._lib.bi_generate_toys(self._h, ptr(z), ptr(rate_scale), int(T), int(seed) & (2**64 - 1)))
        self.T = int(T)

    def generate_toys_points(self, z, rate_scale=None, n_toys=1, seed=0):
        """Replace the data by sum(n_toys) toy datasets, n_toys[h] of them drawn at truth point (z[h], rate_scale[h]),
        truth-major, in one call: the same toys as one `generate_toys` per truth with `toy_offset` advanced.
        -> methods [H]: 1 = drawn event by event, 0 = bin by bin, -1 = a truth without toys."""
        n_toys = np.ascontiguousarray(np.atleast_1d(n_toys), dtype=np.int64)
        H = len(n_toys)
        z = np.ascontiguousarray(as_f64(z).reshape(H, self.d)) if self.d else None
        if rate_scale is not None:
            rate_scale = np.ascontiguousarray(np.broadcast_to(as_f64(np.atleast_2d(rate_scale)), (H, self.S)))
        methods = np.empty(H, dtype=np.int32)
        self._check(self._lib.bi_generate_toys_points(self._h, H, ptr(z), ptr(rate_scale), ptr(n_toys), int(seed) & (2**64 - 1),
                                                      ptr(methods)))
        self.T = int(n_toys.sum())
        return methods

    def download_counts(self, t=0):
        out = np.empty(self.B, dtype=np.float64)
        self._check(self._lib.bi_download_counts(self._h, int(t), ptr(out)))
        return out

    def unpack_rows(self):
        """The packed shadow of the template rows (parameter `packed_rows`) expanded back to doubles -> [anchors x sources,
        padded bins]; raises when the resident model has none (`packed_rows_valid` = 0).  For tests."""
        rows = (int(np.prod([len(g) for g in self.anchor_z], dtype=np.int64)) if self.anchor_z else 1) * self.S
        Bp = self.get_param('padded_bins')
        buf = self.device_alloc(rows * Bp * 8)
        try:
            self._check(self._lib.bi_unpack_rows(self._h, C.c_void_p(buf.ptr)))
            return buf.to_host(np.float64).reshape(rows, Bp)
        finally:
            buf.free()

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

    def eval_one(self, z, rate_scale=None, dataset=0):
        """One point, the call `lf(**kw)` makes inside a minimizer: -> (ll, status) as Python scalars, with as
        little marshalling as ctypes allows (z [d] and rate_scale [S] must be float64 arrays or None)."""
        if z is not None and (z.dtype != np.float64 or not z.flags.c_contiguous or z.size != self.d):
            z = as_f64(z).reshape(self.d)
        if rate_scale is not None and (rate_scale.dtype != np.float64 or not rate_scale.flags.c_contiguous
                                       or rate_scale.size != self.S):
            rate_scale = as_f64(rate_scale).reshape(self.S)
        ds = self._one_ds
        ds.value = dataset
        rc = self._lib.bi_eval(self._h, 1, z.ctypes.data if self.d else None,
                               rate_scale.ctypes.data if rate_scale is not None else None, C.addressof(ds),
                               C.addressof(self._one_out), C.addressof(self._one_st))
        if rc:
            self._check(rc)
        return self._one_out.value, self._one_st.value

    def eval(self, z, rate_scale=None, dataset=None):
        """-> (ll [P], status [P]); z [P, d] (or [d]), rate_scale [P, S] or None, dataset [P] or None."""
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        out = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(out), ptr(status)))
        return out, status

    def eval_begin(self, z, rate_scale=None, dataset=0):
        """First half of a one-point eval: launch and return.  Collect with eval_end(); in between, evaluate other
        contexts (a sum of likelihoods overlaps its terms this way)."""
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        self._check(self._lib.bi_eval_begin(self._h, ptr(z), ptr(rate_scale), int(dataset)))

    def eval_end(self):
        """-> (ll, status) of the evaluation started by eval_begin()."""
        out = C.c_double()
        status = C.c_int32()
        self._check(self._lib.bi_eval_end(self._h, C.byref(out), C.byref(status)))
        return out.value, status.value

    def eval_grad(self, z, rate_scale=None, dataset=None):
        """Value and analytic gradient in one pass -> (ll [P], dll/dz [P, d], dll/drate_scale [P, S], status)."""
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        ll = np.empty(P, dtype=np.float64)
        grad = np.empty((P, self.d + self.S), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_grad(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(grad),
                                           ptr(status)))
        return ll, grad[:, :self.d], grad[:, self.d:], status

    def eval_hess(self, z, rate_scale=None, dataset=None):
        """Value, analytic gradient and Hessian in one pass (bi_eval_hess) -> (ll [P], dll/dz [P, d], dll/drate_scale [P, S],
        H [P, d + S, d + S] over (z, rate_scale), status).  Raises ValueError (BI_ERR_INVALID) where the kernel has no
        analytic Hessian: Beeston-Barlow, unbinned pdfs that are not all finite, too many parameters."""
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        F = self.d + self.S
        ll = np.empty(P, dtype=np.float64)
        grad = np.empty((P, F), dtype=np.float64)
        hess = np.empty((P, F, F), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_hess(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(ll), ptr(grad), ptr(hess),
                                           ptr(status)))
        return ll, grad[:, :self.d], grad[:, self.d:], hess, status

    def eval_gof(self, z, rate_scale=None, dataset=None):
        """Goodness of fit of the data term (bi_eval_gof) -> (half-deviance [P], Pearson chi2 [P], status [P]) of point p
        against dataset[p]; +inf / nan where the likelihood is -inf / nan.  Raises ValueError (BI_ERR_INVALID) for
        Beeston-Barlow and unbinned contexts."""
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        half_deviance = np.empty(P, dtype=np.float64)
        pearson = np.empty(P, dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_gof(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(half_deviance), ptr(pearson),
                                          ptr(status)))
        return half_deviance, pearson, status

    def expected_counts(self, z, rate_scale=None, per_source=False):
        """The expectation per bin (bi_expected_counts) -> mu [P, B], or mu [P, S, B] per source; nan rows for points outside
        the anchor box or with unphysical rates.  Raises ValueError (BI_ERR_INVALID) for Beeston-Barlow and unbinned contexts."""
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        out = np.empty((P, self.S, self.B) if per_source else (P, self.B), dtype=np.float64)
        self._check(self._lib.bi_expected_counts(self._h, P, ptr(z), ptr(rate_scale), 1 if per_source else 0, ptr(out)))
        return out

    def eval_fisher(self, z, rate_scale=None):
        """The expected (Fisher) information over (z, rate_scale) at P truths, no data needed (bi_eval_fisher) ->
        (info [P, d + S, d + S], total expectation [P], unbounded [P, d + S] bins that expect nothing but move with the
        parameter and are left out of `info`, status [P]); nan matrices for points outside the anchor box, with unphysical
        rates or with a negative expectation.  Raises ValueError (BI_ERR_INVALID) for Beeston-Barlow and unbinned contexts
        and for more than 16 coefficient columns."""
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        F = self.d + self.S
        info = np.empty((P, F, F), dtype=np.float64)
        total = np.empty(P, dtype=np.float64)
        unbounded = np.zeros((P, F), dtype=np.int64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_fisher(self._h, P, ptr(z), ptr(rate_scale), ptr(info), ptr(total), ptr(unbounded), ptr(status)))
        return info, total, unbounded, status

    # -- coarse views: the expectation and the data summed over groups of fine bins (bi_set_coarse_binning ...) --
    def set_coarse_binning(self, n_fine=None, groups=None):
        """The context's coarse binning: n_fine [k] fine bins per analysis axis, groups: per axis the ascending fine-bin
        boundaries e_0 < ... < e_m (`CoarseBinning.groups`) -> the number of cells.  No arguments: clear it.  A new model
        releases it.  ValueError (BI_ERR_INVALID) for boundaries that do not fit the model, Beeston-Barlow and unbinned contexts."""
        cells = C.c_int64(0)
        if n_fine is None:
            self._coarse_key = None
            self._check(self._lib.bi_set_coarse_binning(self._h, 0, None, None, None, C.byref(cells)))
            return 0
        n_fine = np.ascontiguousarray(n_fine, dtype=np.int32)
        groups = [np.ascontiguousarray(g, dtype=np.int32).ravel() for g in groups]
        if len(groups) != len(n_fine) or not len(n_fine):
            raise ValueError("need the boundaries of every one of the %d axes" % len(n_fine))
        n_groups = np.array([len(g) - 1 for g in groups], dtype=np.int32)
        bounds = np.ascontiguousarray(np.concatenate(groups), dtype=np.int32)
        # the binning the context holds already (coarse_cells is 0 once a new model has released it): nothing to build or upload
        key = (n_fine.tobytes(), n_groups.tobytes(), bounds.tobytes())
        held = getattr(self, '_coarse_key', None)
        if held is not None and held[0] == key and self.get_param('coarse_cells') == held[1]:
            return held[1]
        self._coarse_key = None
        self._check(self._lib.bi_set_coarse_binning(self._h, len(n_fine), ptr(n_fine), ptr(n_groups), ptr(bounds), C.byref(cells)))
        self._coarse_key = (key, int(cells.value))
        return int(cells.value)

    def expected_coarse(self, n_cells, z, rate_scale=None, per_source=False):
        """The expectation per cell of the coarse binning (bi_expected_coarse) -> (mu [P, C] or [P, S, C], status [P]); nan
        rows and the status bit for points outside the anchor box or with unphysical rates."""
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        out = np.empty((P, self.S, int(n_cells)) if per_source else (P, int(n_cells)), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_expected_coarse(self._h, P, ptr(z), ptr(rate_scale), 1 if per_source else 0, ptr(out), ptr(status)))
        return out, status

    def expected_coarse_jacobian(self, n_cells, z, rate_scale=None):
        """The expectation per cell of the coarse binning and its first derivatives over theta = (z [d], rate_scale [S])
        (bi_expected_coarse_jacobian) -> (mu [P, C], jac [P, d + S, C], status [P]); mu has the bits of `expected_coarse`'s
        total, rows of single-anchor axes are 0, a dead point is nan throughout.  Raises ValueError (BI_ERR_INVALID) for more
        than 16 coefficient columns, and what `expected_coarse` raises."""
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        mu = np.empty((P, int(n_cells)), dtype=np.float64)
        jac = np.empty((P, self.d + self.S, int(n_cells)), dtype=np.float64)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_expected_coarse_jacobian(self._h, P, ptr(z), ptr(rate_scale), ptr(mu), ptr(jac), ptr(status)))
        return mu, jac, status

    def coarse_counts(self, n_cells, datasets=None):
        """The resident datasets' counts per cell of the coarse binning (bi_coarse_counts) -> [n, C]; datasets: indices [n]
        (None: all T)."""
        if datasets is not None:
            datasets = np.ascontiguousarray(np.atleast_1d(datasets), dtype=np.int64)
        n = int(self.T) if datasets is None else len(datasets)
        out = np.empty((n, int(n_cells)), dtype=np.float64)
        self._check(self._lib.bi_coarse_counts(self._h, n, ptr(datasets), ptr(out)))
        return out

    # -- real-valued datasets: a store of its own beside the ordinary data (bi_set_real_counts ... bi_fit_batched_real) --
    def set_real_counts(self, counts):
        """counts: [*bins] (one set) or [T, *bins], every count finite and >= 0 (ValueError otherwise); None drops the store."""
        if counts is None:
            self._check(self._lib.bi_set_real_counts(self._h, 0, None))
            return
        c = as_f64(counts)
        if c.size == 0 or c.size % self.B:
            raise ValueError("counts size %d is not a positive multiple of B=%d" % (c.size, self.B))
        T = c.size // self.B
        self._check(self._lib.bi_set_real_counts(self._h, T, ptr(c.reshape(T, self.B))))

    def set_asimov_counts(self, z, rate_scale=None):
        """H Asimov datasets made on the device (bi_set_asimov_counts): set h holds the expectation at truth (z[h],
        rate_scale[h]), bit for bit the row of `expected_counts`.  ValueError names a truth outside the anchor box, with
        unphysical rates or with a negative / nan expectation; the previous store then stays.  -> H"""
        H, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        self._check(self._lib.bi_set_asimov_counts(self._h, H, ptr(z), ptr(rate_scale)))
        return H

    @property
    def real_count_sets(self):
        return int(self._lib.bi_real_count_sets(self._h))

    def download_real_counts(self, t=0):
        out = np.empty(self.B, dtype=np.float64)
        self._check(self._lib.bi_download_real_counts(self._h, int(t), ptr(out)))
        return out

    def eval_real(self, z, rate_scale=None, dataset=None, gradient=True):
        """Half-deviance against the real-valued store (bi_eval_real) -> (half_deviance [P], d/dz [P, d], d/drate_scale
        [P, S], status [P]); gradient=False: the two slope arrays are None (no limit on 1 + d + S then).  +inf outside the
        box / for unphysical rates / where a filled bin expects nothing, nan where an expectation is negative."""
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        half = np.empty(P, dtype=np.float64)
        grad = np.empty((P, self.d + self.S), dtype=np.float64) if gradient else None
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_real(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), ptr(half), ptr(grad), ptr(status)))
        if not gradient:
            return half, None, None, status
        return half, grad[:, :self.d], grad[:, self.d:], status

    def fit_batched_real(self, P, F, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks, gtol, max_iter, x, f, flags, counters,
                         priors=None):
        """bi_fit_batched_real: `fit_batched` with f = half_deviance - p against the real-valued store."""
        mean = sigma = const = None
        if priors is not None:
            mean, sigma, const = self._gauss_terms(priors, int(F), int(P))
        self._check(self._lib.bi_fit_batched_real(self._h, int(P), int(F), ptr(kind), ptr(index), ptr(z0) if self.d else None, ptr(scale0),
                                                  ptr(unit), ptr(dataset), ptr(x0), ptr(lo), ptr(hi), ptr(n_kinks), ptr(kinks), float(gtol),
                                                  int(max_iter), ptr(mean), ptr(sigma), ptr(const), ptr(x), ptr(f), ptr(flags), ptr(counters)))
        return 0

    @staticmethod
    def _gauss_terms(priors, F, n):
        """priors = (prior_mean [F], prior_sigma [F], prior_const [n] or None) -> the three as C-contiguous float64 arrays"""
        mean, sigma, const = priors
        mean, sigma = as_f64(mean, (F,)), as_f64(sigma, (F,))
        if const is not None:
            const = np.ascontiguousarray(np.broadcast_to(np.asarray(const, dtype=np.float64), (n,)))
        return mean, sigma, const

    def fit_batched(self, P, F, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_kinks, kinks, gtol, max_iter, x, f, flags, counters,
                    priors=None):
        """bi_fit_batched: the batched profile-fit engine's loop with this context's likelihood as the objective (all
        arguments are C-contiguous numpy arrays of the right dtype or None; results are written into x, f, flags, counters).
        priors = (prior_mean [F], prior_sigma [F], prior_const [P] or None): Gaussian constraint terms on the variables
        (bi_fit_batched_gauss)."""
        if priors is not None:
            mean, sigma, const = self._gauss_terms(priors, int(F), int(P))
            self._check(self._lib.bi_fit_batched_gauss(self._h, int(P), int(F), ptr(kind), ptr(index), ptr(z0) if self.d else None, ptr(scale0),
                                                       ptr(unit), ptr(dataset), ptr(x0), ptr(lo), ptr(hi), ptr(n_kinks), ptr(kinks), float(gtol),
                                                       int(max_iter), ptr(mean), ptr(sigma), ptr(const), ptr(x), ptr(f), ptr(flags), ptr(counters)))
            return 0
        self._check(self._lib.bi_fit_batched(self._h, int(P), int(F), ptr(kind), ptr(index), ptr(z0) if self.d else None, ptr(scale0), ptr(unit),
                                             ptr(dataset), ptr(x0), ptr(lo), ptr(hi), ptr(n_kinks), ptr(kinks), float(gtol), int(max_iter),
                                             ptr(x), ptr(f), ptr(flags), ptr(counters)))
        return 0

    def _map_entries(self, E, z0, scale0, unit):
        """the variable map's per-entry arrays with their rows broadcast to E entries -> z0 [E, d], scale0 [E, S], unit [E, S]"""
        def rows(a, n):
            return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1, n), (E, n)))
        return rows(z0, self.d) if self.d else np.zeros((E, 0)), rows(scale0, self.S), rows(unit, self.S)

    def _check_resident(self, rc):
        """`_check` for the loops over resident points: the resident planner's two refusals are a PlannerRefused"""
        if rc == _capi.ERR_INVALID and self._lib.bi_get_param(self._h, b'last_plan_refused') > 0:
            raise PlannerRefused(self._lib.bi_last_error(self._h).decode())
        self._check(rc)

    def sample_stretch(self, W, kind, index, z0, scale0, unit, dataset, x0, lo, hi, n_steps, a=2.0, seed=0, first_ensemble=0, priors=None):
        """bi_sample_stretch: n_steps stretch-move steps of E ensembles of W walkers with this context's likelihood as the
        target.  x0 [E, W, F]; z0 [E, d], scale0 / unit [E, S], dataset [E] or None as `fit_batched`.
        priors = (prior_mean [F], prior_sigma [F], prior_const [E] or None): Gaussian constraint terms on the variables
        (bi_sample_stretch_gauss); the target and the returned ll are then the log density ll + p.
        -> (chain [n_steps, E, W, F], ll [n_steps, E, W], n_accepted [E, W], counters [4])."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        E, W2, F = x0.shape
        if W2 != W:
            raise ValueError("x0 must be [E, W, F]")
        kind, index = np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(index, dtype=np.int32)
        z0, scale0, unit = self._map_entries(E, z0, scale0, unit)
        if dataset is not None:
            dataset = np.ascontiguousarray(np.broadcast_to(np.asarray(dataset, dtype=np.int64), (E,)))
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        if len(kind) != F or len(index) != F or len(lo) != F or len(hi) != F:
            raise ValueError("kind, index, lo and hi must have one entry per variable")
        n_steps = int(n_steps)
        chain = np.empty((max(n_steps, 0), E, W, F))
        ll = np.empty((max(n_steps, 0), E, W))
        n_acc = np.zeros((E, W), dtype=np.int64)
        counters = np.zeros(4, dtype=np.int64)
        head = (self._h, E, int(W), F, ptr(kind), ptr(index), ptr(z0) if self.d else None, ptr(scale0), ptr(unit), ptr(dataset), ptr(x0), ptr(lo),
                ptr(hi), n_steps, float(a), int(seed) & (2 ** 64 - 1), int(first_ensemble))
        tail = (ptr(chain), ptr(ll), ptr(n_acc), ptr(counters))
        if priors is not None:
            mean, sigma, const = self._gauss_terms(priors, F, E)
            rc = self._lib.bi_sample_stretch_gauss(*head, ptr(mean), ptr(sigma), ptr(const), *tail)
        else:
            rc = self._lib.bi_sample_stretch(*head, *tail)
        self._check_resident(rc)
        return chain, ll, n_acc, counters

    def grid_reduce(self, kind, index, z0, scale0, unit, dataset, n_keep, nodes, term=None, logw=None, chunk=0):
        """bi_grid_reduce: this context's likelihood on the tensor-product grid of `nodes` (one 1-d array per variable; kind /
        index as `fit_batched`), reduced over the variables from n_keep on.  z0 [E, d], scale0 / unit [E, S] (rows broadcast),
        dataset [E] or None (one entry, dataset 0); term / logw: None or one array per variable, shaped as its nodes.
        -> (log_marginal [E, K], profile [E, K], argmax [E, K], counters [4]: chunks, evaluations, excluded points, launches)."""
        rc, out = grid_reduce_call(self._lib.bi_grid_reduce, 'bi_grid_reduce', self._h, self.d, self.S, kind, index, z0, scale0, unit, dataset,
                                   n_keep, nodes, term, logw, chunk, 4)
        self._check_resident(rc)
        return out

    def selftest_grid_reduce(self, t, q=None, chunk=0):
        """bi_selftest_grid_reduce: t [cells, R] (and q, or None) through the reduction kernels of `grid_reduce`, in chunks of
        `chunk` values -> (log_marginal [cells], profile [cells], argmax [cells])."""
        t = as_f64(t)
        if t.ndim != 2:
            raise ValueError("t must be [cells, R]")
        q = None if q is None else as_f64(q, t.shape)
        cells, R = t.shape
        log_marginal, profile, argmax = np.empty(cells), np.empty(cells), np.empty(cells, dtype=np.int64)
        self._check(self._lib.bi_selftest_grid_reduce(self._h, cells, R, int(chunk), ptr(t), ptr(q), ptr(log_marginal), ptr(profile),
                                                      ptr(argmax)))
        return log_marginal, profile, argmax

    def eval_datasets(self, z, rate_scale=None, t0=0, t1=None):
        """One parameter point against datasets [t0, t1) -> (ll [t1-t0], status)."""
        t1 = self.T if t1 is None else int(t1)
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        out = np.empty(max(t1 - int(t0), 0), dtype=np.float64)
        status = np.zeros(1, dtype=np.int32)
        self._check(self._lib.bi_eval_datasets(self._h, ptr(z), ptr(rate_scale), int(t0), t1, ptr(out), ptr(status)))
        return out, int(status[0])

    def eval_datasets_device(self, out_ptr, z, rate_scale=None, t0=0, t1=None):
        """eval_datasets with the ll vector left in HBM at device address `out_ptr` -> status."""
        t1 = self.T if t1 is None else int(t1)
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        status = np.zeros(1, dtype=np.int32)
        self._check(self._lib.bi_eval_datasets_device(self._h, ptr(z), ptr(rate_scale), int(t0), t1, C.c_void_p(out_ptr),
                                                      ptr(status)))
        return int(status[0])

    def eval_datasets_points(self, z, rate_scale=None, t0=0, t1=None, out=None):
        """P parameter points against datasets [t0, t1) in one call (the toy-MC form over several hypotheses: the points of a
        pass share the passes over the templates and over the datasets' lists) -> (ll [P, t1 - t0], status [P]).
        `out`: a C-contiguous float64 array of that shape to write into (a loop that reuses it saves the page faults of a
        fresh 8 P T-byte array per call: 0.1 ms at 32 x 10^4)."""
        t1 = self.T if t1 is None else int(t1)
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        shape = (P, max(t1 - int(t0), 0))
        if out is None:
            out = np.empty(shape, dtype=np.float64)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of shape %s" % (shape,))
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_datasets_points(self._h, P, ptr(z), ptr(rate_scale), int(t0), t1, ptr(out), ptr(status)))
        return out, status

    def eval_datasets_points_device(self, out_ptr, z, rate_scale=None, t0=0, t1=None):
        """eval_datasets_points with the [P, t1 - t0] result left in HBM at device address `out_ptr` -> status [P]."""
        t1 = self.T if t1 is None else int(t1)
        P, z, rate_scale, _ = self._point_args(z, rate_scale, None)
        status = np.zeros(P, dtype=np.int32)
        self._check(self._lib.bi_eval_datasets_points_device(self._h, P, ptr(z), ptr(rate_scale), int(t0), t1, C.c_void_p(out_ptr),
                                                             ptr(status)))
        return status

    def interpolate(self, which, z):
        """which: 'ps' -> [S, B], 'mus' -> [S], 'n_model' -> [B] (the Beeston-Barlow source row)."""
        code = {'ps': 0, 'mus': 1, 'n_model': 2}[which]
        shape = {0: (self.S, self.B), 1: (self.S,), 2: (self.B,)}[code]
        z = as_f64(z).reshape(self.d) if self.d else None
        out = np.empty(shape, dtype=np.float64)
        self._check(self._lib.bi_interpolate(self._h, code, ptr(z), ptr(out)))
        return out

    def eval_full(self, z, rate_scale=None, dataset=0):
        """full_output form -> (ll, mus [S], ps [S, B], status)."""
        z = as_f64(z).reshape(self.d) if self.d else None
        if rate_scale is not None:
            rate_scale = as_f64(rate_scale, (self.S,))
        ll = np.zeros(1)
        mus = np.zeros(self.S)
        n = self.B
        if int(dataset) and 0 <= int(dataset) < self.T and int(self._lib.bi_event_set_count(self._h)) > 1:
            n = int(self.event_set_counts()[int(dataset)])          # several event sets: the events of that set
        ps = np.zeros((self.S, n))
        st = np.zeros(1, dtype=np.int32)
        self._check(self._lib.bi_eval_full(self._h, ptr(z), ptr(rate_scale), int(dataset), ptr(ll), ptr(mus), ptr(ps),
                                           ptr(st)))
        return float(ll[0]), mus, ps, int(st[0])

    def plan(self, z, rate_scale=None, dataset=None):
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        h = C.c_void_p()
        self._check(self._lib.bi_plan_points(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), C.byref(h)))
        return EvalPlan(self, h, P)

    def plan_share(self, z, rate_scale=None, dataset=None, rank=0, world=1):
        """This context's share of a scan dealt over `world` GPUs: every rank passes the same points, the device
        planner's (cell, dataset) sort is the dealing.  -> EvalPlan with `.share = (lo, hi)` and `.n_valid`; its run()
        leaves hi - lo results in sorted order, `unsort()` turns the gathered vectors into the caller's order."""
        P, z, rate_scale, dataset = self._point_args(z, rate_scale, dataset)
        h = C.c_void_p()
        self._check(self._lib.bi_plan_points_share(self._h, P, ptr(z), ptr(rate_scale), ptr(dataset), int(rank), int(world),
                                                   C.byref(h)))
        plan = EvalPlan(self, h, P)
        nv, lo, hi = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.bi_plan_share_info(h, C.byref(nv), C.byref(lo), C.byref(hi)))
        plan.n_valid, plan.share, plan.world = nv.value, (lo.value, hi.value), int(world)
        return plan

    def plan_resident(self, P, z, rate_scale=None, dataset=None, rank=0, world=1):
        """plan() / plan_share() for points that are already in HBM: `z` [P][d] (and `rate_scale` [P][S], `dataset`
        [P] int64) are DeviceBuffers (or device addresses) on this GPU, read where they lie.  world > 1: this rank's
        share of a dealt scan, as plan_share.  Always planned on the device: a batch with infinite rates of a source that may go
        negative, or with Beeston-Barlow points that need the host planner's exact totals, is refused (ValueError)."""
        def addr(b, item_bytes, what):
            if b is None:
                return None
            if isinstance(b, DeviceBuffer):
                if b.nbytes < int(P) * item_bytes:
                    raise ValueError("%s holds %d bytes, %d points need %d" % (what, b.nbytes, P, int(P) * item_bytes))
                return C.c_void_p(b.ptr)
            return C.c_void_p(int(b))
        h = C.c_void_p()
        self._check(self._lib.bi_plan_points_resident(self._h, int(P), addr(z, 8 * max(self.d or 0, 0), 'z'),
                                                      addr(rate_scale, 8 * (self.S or 0), 'rate_scale'), addr(dataset, 8, 'dataset'),
                                                      int(rank), int(world), C.byref(h)))
        plan = EvalPlan(self, h, int(P))
        if world > 1:
            nv, lo, hi = C.c_int64(), C.c_int64(), C.c_int64()
            self._check(self._lib.bi_plan_share_info(h, C.byref(nv), C.byref(lo), C.byref(hi)))
            plan.n_valid, plan.share, plan.world = nv.value, (lo.value, hi.value), int(world)
        return plan

    # -- plain device buffers (gather staging) ------------------------------------------------------
    def device_alloc(self, nbytes):
        """-> DeviceBuffer of `nbytes` on this context's GPU.  `.free()` releases it; buffers still alive when the
        context is closed are released with it (the library keeps track of them: `user_allocations`)."""
        h = C.c_void_p()
        self._check(self._lib.bi_device_alloc(self._h, int(nbytes), C.byref(h)))
        return DeviceBuffer(self, h.value, int(nbytes))

    # -- measurement -----------------------------------------------------------------------
    def profile(self, on):
        self._check(self._lib.bi_profile_enable(self._h, 1 if on else 0))

    def read_bandwidth(self, nontemporal=True, blocks_per_cu=32, reps=5):
        """GB/s of a plain streaming sum over the resident template tensor: the device's read-only ceiling."""
        out = C.c_double()
        self._check(self._lib.bi_measure_read_bandwidth(self._h, 1 if nontemporal else 0, int(blocks_per_cu), int(reps),
                                                        C.byref(out)))
        return out.value

    def stream_bandwidth(self, items=8, rows=32, nontemporal=True, blocks_per_cu=8, reps=5):
        """GB/s of `items` work items streaming `rows` template rows each with the morph kernel's access pattern and
        no arithmetic: the ceiling the morph + reduce kernel is held against."""
        out = C.c_double()
        self._check(self._lib.bi_measure_stream_bandwidth(self._h, int(items), int(rows), 1 if nontemporal else 0,
                                                          int(blocks_per_cu), int(reps), C.byref(out)))
        return out.value

    def copy_bandwidth(self, nbytes=1 << 31, reps=3):
        """GB/s (read + written) of a device-to-device copy of the first `nbytes` of the template tensor."""
        out = C.c_double()
        self._check(self._lib.bi_measure_copy_bandwidth(self._h, int(nbytes), int(reps), C.byref(out)))
        return out.value

    def profile_read(self):
        n = C.c_int64()
        ms = C.c_double()
        self._check(self._lib.bi_profile_read(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value


def grid_reduce_call(symbol, who, handle, d, S, kind, index, z0, scale0, unit, dataset, n_keep, nodes, term, logw, chunk, n_counters, extra=()):
    """The arguments and outputs of bi_grid_reduce and bi_grid_reduce_sourcewise (`symbol`; `who` names it in messages) for a model of
    d axes and S sources: the per-variable arrays laid out one after the other, the entries' rows broadcast, the outputs made.
    `extra`: the arguments between `chunk` and the outputs.  -> (return code, (log_marginal [E, K], profile [E, K], argmax [E, K],
    counters [n_counters]))."""
    kind, index = np.ascontiguousarray(kind, dtype=np.int32), np.ascontiguousarray(index, dtype=np.int32)
    nodes = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in nodes]
    F, n_keep = len(nodes), int(n_keep)
    if len(kind) != F or len(index) != F or any(v.ndim != 1 for v in nodes):
        raise ValueError("kind, index and nodes must have one entry per variable, every entry of nodes one-dimensional")
    n_nodes = np.array([len(v) for v in nodes], dtype=np.int32)

    def flat(arrays, what):
        if arrays is None:
            return None
        arrays = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in arrays]
        if len(arrays) != F or any(v.shape != w.shape for v, w in zip(arrays, nodes)):
            raise ValueError("%s must hold one array per variable, shaped as its nodes" % what)
        return np.ascontiguousarray(np.concatenate(arrays)) if F else np.zeros(0)
    term, logw = flat(term, 'term'), flat(logw, 'logw')
    nodes_flat = np.ascontiguousarray(np.concatenate(nodes)) if F else np.zeros(0)
    if dataset is not None:
        dataset = np.ascontiguousarray(np.atleast_1d(np.asarray(dataset, dtype=np.int64)))
    E = 1 if dataset is None else len(dataset)

    def rows(a, n):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1, n), (E, n)))
    z0 = rows(z0, d) if d else None
    scale0, unit = rows(scale0, S), rows(unit, S)
    K = int(np.prod(n_nodes[:max(0, min(n_keep, F))], dtype=np.int64)) if F and np.all(n_nodes >= 1) else 1
    if E * K > 2 ** 24:                                       # (refused by the library too; here before the outputs are made)
        raise ValueError("%s: E * K (%d dataset entries x %d kept points) is more than 2^24 cells" % (who, E, K))
    log_marginal, profile = np.empty((E, K)), np.empty((E, K))
    argmax = np.empty((E, K), dtype=np.int64)
    counters = np.zeros(int(n_counters), dtype=np.int64)
    rc = symbol(handle, E, ptr(dataset), F, n_keep, ptr(kind), ptr(index), ptr(z0), ptr(scale0), ptr(unit), ptr(n_nodes), ptr(nodes_flat),
                ptr(term), ptr(logw), int(chunk), *extra, ptr(log_marginal), ptr(profile), ptr(argmax), ptr(counters))
    return rc, (log_marginal, profile, argmax, counters)


class DeviceBuffer:
    """A plain allocation in HBM: `.ptr` is the device address (an int), e.g. the target of EvalPlan.run or the
    send / receive buffer of an RCCL collective."""

    def __init__(self, ctx, ptr_value, nbytes):
        self.ctx, self.ptr, self.nbytes = ctx, ptr_value, nbytes

    def to_host(self, dtype=np.float64, count=None, offset_bytes=0, out=None):
        """`out`: a C-contiguous array of `count` elements of `dtype` to copy into (a loop that reuses it saves the page faults of a
        fresh array per call: ~0.5 ms per 8 MB, and the runtime's slow path into memory it has not seen)."""
        n = (self.nbytes - offset_bytes) // np.dtype(dtype).itemsize if count is None else int(count)
        if out is None:
            out = np.empty(n, dtype=dtype)
        elif out.size != n or out.dtype != np.dtype(dtype) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous %s array of %d elements" % (np.dtype(dtype), n))
        self.ctx._check(self.ctx._lib.bi_memcpy_to_host(self.ctx._h, ptr(out), C.c_void_p(self.ptr + offset_bytes), out.nbytes))
        return out

    def from_host(self, a, offset_bytes=0):
        a = np.ascontiguousarray(a)
        if a.nbytes + offset_bytes > self.nbytes:
            raise ValueError("array does not fit the device buffer")
        self.ctx._check(self.ctx._lib.bi_memcpy_to_device(self.ctx._h, C.c_void_p(self.ptr + offset_bytes), ptr(a), a.nbytes))

    def free(self):
        if self.ptr and self.ctx._h.value:
            self.ctx._lib.bi_device_free(self.ctx._h, C.c_void_p(self.ptr))
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class EvalPlan:
    """A batch of points whose host-side preparation (cell lookup, rates, grouping) is done and
    resident on the device; `run()` only launches kernels."""

    def __init__(self, ctx, handle, P):
        self.ctx, self._h, self.P = ctx, handle, P

    @property
    def bytes(self):
        return int(self.ctx._lib.bi_plan_bytes(self._h))

    @property
    def launches(self):
        return int(self.ctx._lib.bi_plan_launches(self._h))

    def run(self, out_dev_ptr=None):
        self.ctx._check(self.ctx._lib.bi_run_plan(self.ctx._h, self._h, out_dev_ptr))
        return self

    def unsort(self, gathered_ptr, stride, full_ptr):
        """A share of a dealt scan: gathered [world][stride] (device; rank r's results in sorted order) -> full [P] in
        the caller's point order (device), on the context stream."""
        self.ctx._check(self.ctx._lib.bi_plan_unsort(self.ctx._h, self._h, C.c_void_p(gathered_ptr), int(stride),
                                                     C.c_void_p(full_ptr)))

    def status(self):
        """Bitwise OR of the per-point status words of the last run() (waits for it) -- for callers that leave the
        results in HBM.  Raises DeviceError on BI_ST_INTERNAL (a launch gave up collecting a partial sum: the
        results of that run are not to be used; the library has emptied its mailbox again)."""
        word = C.c_int32()
        self.ctx._check(self.ctx._lib.bi_plan_status(self.ctx._h, self._h, C.byref(word)))
        if word.value & _capi.ST_INTERNAL:
            raise DeviceError("a launch of this plan gave up waiting for a partial sum (BI_ST_INTERNAL): results discarded")
        return word.value

    def read(self):
        out = np.empty(self.P, dtype=np.float64)
        status = np.zeros(self.P, dtype=np.int32)
        self.ctx._check(self.ctx._lib.bi_plan_read(self.ctx._h, self._h, ptr(out), ptr(status)))
        return out, status

    def close(self):
        if self._h is not None and self._h.value and self.ctx._h.value:
            self.ctx._lib.bi_plan_destroy(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
