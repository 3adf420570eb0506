"""Gridded likelihoods: the likelihood (with its priors) on a tensor-product grid of parameters, reduced over some of the
grid's axes -- the marginal likelihood by quadrature and the grid profile.

    res = lf.grid_scan(keep=[('s0_rate_multiplier', np.linspace(0, 5, 101))],
                       reduce=[('shift', np.linspace(-1, 1, 21)), ('s1_rate_multiplier', np.linspace(0.5, 1.5, 21))])
    res.log_marginal                 # log int L pi d(nuisances) at every kept node, by quadrature over the reduce nodes
    res.credible_upper_limit(0.9)    # a Bayesian limit without a chain
    res.profile, res.best            # max over the reduce nodes of log L + log pi, and where it is attained

With g the grid point of kept multi-index k and reduced multi-index r,

    t_g = log L + log pi             profile[k] = max_r t_g,  argmax[k] = the smallest (row-major) r that attains it
    u_g = t_g + sum_j log w_j        log_marginal[k] = log sum_r exp(u_g)

where w_j are the quadrature weights of the reduced axes.  A point of likelihood zero (outside the anchor box, unphysical
rates, a prior of zero) is excluded and counted; a cell with no point left is -inf with argmax -1.  The grid profile is the
global maximum over the nodes: it cannot be trapped at a kink of the morph, and it never lies above the true profile.

Two engines compute the same thing:

    'native'   bi_grid_reduce: the grid is produced, evaluated and reduced on the device in chunks, only the reduced arrays
               come back.  Taken whenever nothing but the device call sits between the parameters and the likelihood: one
               device context, no efficiencies, unphysical_behaviour other than 'error'.  Priors are per-parameter callables,
               hence separable: they are evaluated at the nodes on the host and added on the device, whatever callable they are.
    'host'     the executable specification: `lf.eval_points` over the same grid in chunks, reduced in NumPy -- for anything
               that has `eval_points` (sums, re-parametrisations), and for models whose batches the device planner
               refuses.

A prepared source-wise model (`SourceWiseBinnedLogLikelihood`) runs natively as a function, `blueice_amd.grid.grid_scan(lf, ...)`
(bi_grid_reduce_sourcewise; the bound lf.grid_scan stays refused and names this spelling).  Its chunks are evaluated by the
route `likelihood_config['sourcewise_grid_route']` names: 'points' (one work item per point, the kernels of `eval_points`),
'scan' (the matrix-core scan route of `eval_points_scan`: needs the non-empty-bin form and at most 32 rows per point) or 'auto'
(the default: see SOURCEWISE_AUTO_ROUTE).

So does a prepared unbinned source-wise model with data set (`SourceWiseUnbinnedLogLikelihood`; bi_grid_reduce_sourcewise_events
through the class's `_native_grid_reduce`, `ctx.grid_reduce_events`; `datasets=` indexes the event sets of `set_datasets` or of
`sourcewise_event_toys*`).  The matrix-core scan route does not read the event store: 'auto' means 'points' there
(SOURCEWISE_EVENTS_AUTO_ROUTE) and 'scan' raises ValueError.  No scan route over events exists.  The per-point route against the host
engine (examples/many_nuisances.py --measure-unbinned-grid, profiles/sourcewise_events_scan_measure.txt, one MI355X, d = 4, S = 4, 5
anchors, cache-assisted): 10^4 events, 975 975 grid points 58.0 ms against 183.3 ms (3.2 x); 10^6 events, 66 759 points 547.7 ms against
557.7 ms (1.02 x: the event kernel is all of the time there).
"""
import numpy as np

from .exceptions import PlannerRefused

__all__ = ['grid_scan', 'GridResult', 'trapezoid_weights', 'reduce_cells']

HOST_CHUNK = 1 << 16
# what likelihood_config['sourcewise_grid_route'] = 'auto' asks the library for: -1 = the scan route where the model is eligible
# (the non-empty-bin form built, at most 32 rows per point), else one work item per point
SOURCEWISE_AUTO_ROUTE = -1
SOURCEWISE_EVENTS_AUTO_ROUTE = 0        # ... on an event store: one work item per point, the only route that reads it
_SOURCEWISE_ROUTES = {'auto': None, 'points': 0, 'scan': 1}


def _sourcewise_route(lf):
    """-> the `route` of ctx.grid_reduce for a source-wise model (likelihood_config['sourcewise_grid_route']), None for any other"""
    from .source_wise import SourceWiseBinnedLogLikelihood
    from .source_wise_unbinned import SourceWiseUnbinnedLogLikelihood
    if not isinstance(lf, (SourceWiseBinnedLogLikelihood, SourceWiseUnbinnedLogLikelihood)):
        return None
    setting = lf.config.get('sourcewise_grid_route', 'auto')
    if not isinstance(setting, str) or setting not in _SOURCEWISE_ROUTES:
        raise ValueError("likelihood_config['sourcewise_grid_route'] is 'auto', 'points' or 'scan', not %r" % (setting,))
    route = _SOURCEWISE_ROUTES[setting]
    if route is None:
        return SOURCEWISE_EVENTS_AUTO_ROUTE if isinstance(lf, SourceWiseUnbinnedLogLikelihood) else SOURCEWISE_AUTO_ROUTE
    return route


def trapezoid_weights(x):
    """Weights of the trapezoid rule on the ascending nodes x: half the distance between the neighbours in the interior,
    half-intervals at the ends; a single node has weight 1.  ValueError if x does not ascend strictly."""
    x = np.asarray(x, dtype=float)
    if x.ndim != 1 or len(x) < 1:
        raise ValueError("trapezoid weights need a one-dimensional, non-empty array of nodes")
    if len(x) == 1:
        return np.ones(1)
    if not np.all(np.diff(x) > 0):
        raise ValueError("trapezoid weights need strictly ascending nodes")
    w = np.empty(len(x))
    w[1:-1] = (x[2:] - x[:-2]) / 2
    w[0], w[-1] = (x[1] - x[0]) / 2, (x[-1] - x[-2]) / 2
    return w


def _trapezoid(y, x):
    """sum of trapezoids along the last axis"""
    return np.sum(0.5 * (y[..., 1:] + y[..., :-1]) * np.diff(x), axis=-1)


def reduce_cells(t, q=None):
    """The reduction in NumPy: t [cells, R] (log L + log pi; -inf: excluded), q [R] or [cells, R] or None (log weights).
    -> (log_marginal [cells], profile [cells], argmax [cells], excluded)."""
    t = np.asarray(t, dtype=float)
    cells, R = t.shape
    gone = t == -np.inf
    nan_cell = np.isnan(t).any(axis=1)
    tt = np.where(gone | np.isnan(t), -np.inf, t)
    profile = tt.max(axis=1)
    argmax = np.where(np.isfinite(profile) | (profile == np.inf), tt.argmax(axis=1), -1).astype(np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        u = tt if q is None else tt + np.broadcast_to(q, t.shape)
        m = u.max(axis=1)
        ref = np.where(np.isfinite(m), m, 0.0)
        log_marginal = np.where(m == -np.inf, -np.inf, ref + np.log(np.sum(np.exp(u - ref[:, None]), axis=1)))
    log_marginal[nan_cell] = profile[nan_cell] = np.nan
    argmax[nan_cell] = -1
    return log_marginal, profile, argmax, int(gone.sum())


class GridResult:
    """keep / reduce: [(name, nodes), ...]; log_marginal, profile, argmax: [(E,) n_0, ..., n_keep-1]; best: reduce name ->
    the node at the argmax (nan where a cell has no point); excluded: points of likelihood zero; engine 'native' or 'host';
    counters: chunks, evaluations, excluded points, evaluation launches (and, for a source-wise model, the route taken: 0 points,
    1 scan)."""

    def __init__(self, keep, reduce, log_marginal, profile, argmax, excluded, engine, counters, has_datasets):
        self.keep, self.reduce = keep, reduce
        self.log_marginal, self.profile, self.argmax = log_marginal, profile, argmax
        self.excluded, self.engine, self.counters = int(excluded), engine, counters
        self._lead = 1 if has_datasets else 0
        shape = tuple(len(v) for _, v in reduce)
        at = np.unravel_index(np.maximum(argmax, 0), shape) if shape else ()
        self.best = {name: np.where(argmax >= 0, nodes[i], np.nan) for (name, nodes), i in zip(reduce, at)}

    def likelihood_ratio(self):
        """profile.max - profile: the maximum over the kept nodes (of every dataset by itself)"""
        axes = tuple(range(self._lead, self.profile.ndim))
        return np.max(self.profile, axis=axes, keepdims=True) - self.profile

    def _one_axis(self, what):
        if len(self.keep) != 1 or len(self.keep[0][1]) < 2 or not np.all(np.diff(self.keep[0][1]) > 0):
            raise ValueError("%s needs exactly one kept axis, with at least two ascending nodes" % what)
        return self.keep[0][1]

    def posterior(self):
        """exp(log_marginal) along the one kept axis, normalised to a trapezoid integral of 1"""
        x = self._one_axis('posterior')
        with np.errstate(invalid='ignore'):
            p = np.exp(self.log_marginal - np.max(self.log_marginal, axis=-1, keepdims=True))
        return p / _trapezoid(p, x)[..., None]

    def credible_upper_limit(self, cl=0.9):
        """the kept parameter's value below which the posterior holds `cl`: the cumulative trapezoid sums of `posterior`,
        interpolated linearly between the nodes"""
        if not 0 < cl < 1:
            raise ValueError("credible_upper_limit: cl must lie in (0, 1)")
        x = self._one_axis('credible_upper_limit')
        p = self.posterior()
        steps = 0.5 * (p[..., 1:] + p[..., :-1]) * np.diff(x)
        cdf = np.concatenate([np.zeros(p.shape[:-1] + (1,)), np.cumsum(steps, axis=-1)], axis=-1)
        if cdf.ndim == 1:
            return float(np.interp(cl, cdf, x))
        return np.array([np.interp(cl, row, x) for row in cdf])


def _axes(spec, what):
    out = []
    for item in spec or ():
        try:
            name, nodes = item
        except (TypeError, ValueError):
            raise ValueError("grid_scan: %s must be a list of (name, nodes)" % what)
        nodes = np.atleast_1d(np.asarray(nodes, dtype=float))
        if nodes.ndim != 1 or len(nodes) < 1:
            raise ValueError("grid_scan: the nodes of %s must be a non-empty one-dimensional array" % name)
        if not np.all(np.isfinite(nodes)):
            raise ValueError("grid_scan: the nodes of %s must be finite" % name)
        out.append((str(name), nodes))
    return out


def _log_weights(weights, reduce):
    """-> one array of log weights per reduced axis, or None (a plain sum)"""
    if weights is None:
        return None
    if isinstance(weights, str):
        if weights != 'trapezoid':
            raise ValueError("grid_scan: weights must be 'trapezoid', None or one array per reduced axis")
        ws = []
        for name, nodes in reduce:
            try:
                ws.append(trapezoid_weights(nodes))
            except ValueError:
                raise ValueError("grid_scan: trapezoid weights need strictly ascending nodes (%s)" % name)
    else:
        ws = [np.atleast_1d(np.asarray(w, dtype=float)) for w in weights]
        if len(ws) != len(reduce) or any(w.shape != nodes.shape for w, (_, nodes) in zip(ws, reduce)):
            raise ValueError("grid_scan: weights must hold one array per reduced axis, shaped as its nodes")
        if any(not np.all(np.isfinite(w) & (w >= 0)) for w in ws):
            raise ValueError("grid_scan: weights must be finite and >= 0")
    with np.errstate(divide='ignore'):
        return [np.log(w) for w in ws]


def _native_plan(lf, axes, fixed, livetime_days):
    """What bi_grid_reduce needs to evaluate `lf` on the grid without Python: which variable is which parameter, the other
    settings, the priors at the nodes (term) and the fixed parameters' priors (a constant) -- or None where Python sits
    between the parameters and the device call (the conditions of BatchObjective.native(), without its restriction on priors)."""
    from .likelihood import DeviceLogLikelihood, _prior_of
    from .profile import variable_map
    ok = isinstance(lf, DeviceLogLikelihood) and getattr(lf, 'ctx', None) is not None and \
        (hasattr(lf, '_native_grid_reduce') or hasattr(lf.ctx, 'grid_reduce')) and \
        not any(getattr(lf, 'source_apply_efficiency', [])) and lf.config.get('unphysical_behaviour') != 'error'
    if not ok:
        return None
    var_map = variable_map(lf, [name for name, _ in axes])
    if var_map is None:
        return None
    term = []
    for (name, nodes), kind in zip(axes, var_map[0]):
        prior = lf.rate_parameters.get(name[:-16]) if kind else lf.shape_parameters[name][1]
        term.append(np.zeros(len(nodes)) if prior is None else _prior_of(prior, nodes))
    z0, scale0, _, unit = lf._batch_terms(dict(fixed), livetime_days, want_unit=True)
    # the priors of the parameters that are no axis of the grid, at their values
    names = [n for n, _ in axes]
    const = 0.0
    for i, (name, (_, prior, _)) in enumerate(lf.shape_parameters.items()):
        if prior is not None and name not in names:
            const += float(_prior_of(prior, z0[:1, i])[0])
    for src, prior in lf.rate_parameters.items():
        key = src + '_rate_multiplier'
        if prior is not None and key not in names:
            const += float(_prior_of(prior, np.array([float(fixed.get(key, 1.0))]))[0])
    if any(np.any(np.isnan(t) | (t == np.inf)) for t in term) or not np.isfinite(const):
        return None                                          # (a prior that is nan or +inf somewhere: the host engine reports it)
    if all(not np.any(t) for t in term):
        term = None
    return dict(kind=var_map[0], index=var_map[1], z0=z0, scale0=scale0, unit=unit, term=term, const=const)


def _host_engine(lf, axes, n_keep, logw, datasets, livetime_days, chunk, fixed):
    shape = tuple(len(v) for _, v in axes)
    K = int(np.prod(shape[:n_keep], dtype=np.int64))
    R = int(np.prod(shape[n_keep:], dtype=np.int64))
    E = 1 if datasets is None else len(datasets)
    G = E * K * R
    chunk = int(chunk) if chunk else HOST_CHUNK
    t = np.empty(G)
    counters = np.zeros(4, dtype=np.int64)
    for g0 in range(0, G, chunk):
        g = np.arange(g0, min(G, g0 + chunk))
        at = np.unravel_index(g % (K * R), shape)
        call = {name: nodes[i] for (name, nodes), i in zip(axes, at)}
        call.update(fixed)
        more = {} if datasets is None else {'dataset': datasets[g // (K * R)]}
        t[g] = np.asarray(lf.eval_points(call, livetime_days=livetime_days, **more), dtype=float)
        counters[0] += 1
        counters[1] += len(g)
    q = None
    if logw is not None:
        q = np.zeros(shape[n_keep:])
        for j, lw in enumerate(logw):
            q = q + lw.reshape((1,) * j + (-1,) + (1,) * (len(logw) - j - 1))
        q = q.reshape(R)
    log_marginal, profile, argmax, excluded = reduce_cells(t.reshape(E * K, R), q)
    counters[2] = excluded
    return log_marginal, profile, argmax, counters


def grid_scan(lf, keep=(), reduce=(), weights='trapezoid', datasets=None, livetime_days=None, chunk=None, engine=None, **fixed):
    """The likelihood on the tensor-product grid of the `keep` and `reduce` axes (lists of (parameter name, nodes)), reduced
    over the `reduce` axes: marginal likelihood and grid profile at every kept node (see the module's docstring).

    weights: 'trapezoid' (the trapezoid rule on ascending reduce nodes), None (a plain sum) or one array of weights per
    reduced axis.  datasets: one entry per dataset the likelihood holds (`simulate_toys`, a stack given to
    `set_binned_data`), all in the same call.  fixed (kwargs): parameters held at one value; every other parameter that is
    no axis stays at its default.  chunk: grid points per device call (or per `eval_points` call of the host engine).
    engine: None (native where possible), 'native', 'host'.  -> GridResult."""
    if engine not in (None, 'native', 'host'):
        raise ValueError("grid_scan: engine must be None, 'native' or 'host'")
    keep, reduce = _axes(keep, 'keep'), _axes(reduce, 'reduce')
    axes = keep + reduce
    names = [n for n, _ in axes]
    if not axes:
        raise ValueError("grid_scan: need at least one axis in keep or reduce")
    if len(axes) > 16:
        raise ValueError("grid_scan: at most 16 axes (got %d)" % len(axes))
    if len(set(names)) != len(names) or any(n in fixed for n in names):
        raise ValueError("grid_scan: a parameter can be one axis of the grid or fixed, and only once")
    if chunk is not None and not 1 <= int(chunk) <= 2 ** 26:
        raise ValueError("grid_scan: chunk must lie in [1, 2^26]")
    logw = _log_weights(weights, reduce)
    if datasets is not None:
        datasets = np.atleast_1d(np.asarray(datasets, dtype=np.int64))
        if datasets.ndim != 1 or len(datasets) < 1:
            raise ValueError("grid_scan: datasets must be a non-empty one-dimensional array of dataset indices")
    E = 1 if datasets is None else len(datasets)
    n_keep = len(keep)
    kept_shape = tuple(len(v) for _, v in keep)
    if E * int(np.prod(kept_shape, dtype=np.int64)) > 2 ** 24:
        raise ValueError("grid_scan: more than 2^24 cells (datasets x kept nodes)")

    plan = None
    if engine != 'host':
        if getattr(lf, 'is_data_set', True) is False:
            from .exceptions import NotPreparedException
            raise NotPreparedException("grid_scan requires you to first set the data using set_data()")
        plan = _native_plan(lf, axes, fixed, livetime_days)
        if plan is None and engine == 'native':
            raise ValueError("grid_scan: this likelihood has Python between its parameters and the device call (efficiencies, "
                             "unphysical_behaviour='error', a sum or re-parametrisation), or an axis that is no "
                             "parameter of it: engine='host'")
    result = None
    if plan is not None:
        try:
            full_logw = None if logw is None else [np.zeros(len(v)) for _, v in keep] + logw
            route = _sourcewise_route(lf)
            more = {} if route is None else {'route': route}
            reduce_call = getattr(lf, '_native_grid_reduce', None) or lf.ctx.grid_reduce
            lm, prof, arg, counters = reduce_call(plan['kind'], plan['index'], plan['z0'], plan['scale0'], plan['unit'], datasets, n_keep,
                                                  [v for _, v in axes], term=plan['term'], logw=full_logw, chunk=chunk or 0, **more)
            result = (lm.ravel() + plan['const'], prof.ravel() + plan['const'], arg.ravel(), counters)
            used = 'native'
        except PlannerRefused:
            if engine == 'native':
                raise
    if result is None:
        result = _host_engine(lf, axes, n_keep, logw, datasets, livetime_days, chunk, fixed)
        used = 'host'
    lm, prof, arg, counters = result
    out_shape = (() if datasets is None else (E,)) + kept_shape
    return GridResult(keep, reduce, lm.reshape(out_shape), prof.reshape(out_shape), arg.reshape(out_shape), counters[2], used, counters,
                      datasets is not None)


def _attach():
    from .likelihood import LogAncillaryLikelihood, LogLikelihoodBase, LogLikelihoodReParam, LogLikelihoodSum
    for cls in (LogLikelihoodBase, LogLikelihoodSum, LogAncillaryLikelihood, LogLikelihoodReParam):
        setattr(cls, 'grid_scan', grid_scan)


_attach()
