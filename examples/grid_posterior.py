"""A Bayesian upper limit and a grid profile from one gridded likelihood on the device -- run as

    PYTHONPATH=. python examples/grid_posterior.py [--config C2] [--nodes 101 21] [--reps 7] [--skip-host] [--skip-fits]

The likelihood of a C2-like model (4 sources, three shape parameters) is put on the tensor-product grid of the signal's rate
multiplier (kept, 101 nodes) and the three shape parameters (reduced, 21 nodes each): about 10^6 points.  `lf.grid_scan`
produces, evaluates and reduces them on the device (bi_grid_reduce); what comes back is the marginal likelihood and the grid
profile at the 101 kept nodes.  From them: the 90 % credible upper limit on the signal without a chain, and the grid profile
next to `likelihood_ratio_scan`, which fits the shape parameters at every kept node from starting points.

Timed: the native engine against the host engine (the same grid through `lf.eval_points` in chunks, reduced in NumPy) --
medians and quartiles of alternated calls -- and the host-to-device traffic the native engine avoids: the host engine
uploads d + S doubles per point and downloads one.
"""
import argparse
import time

import numpy as np

from blueice_amd.inference import likelihood_ratio_scan
from blueice_amd.synthetic import SyntheticModel


def quartiles(ts):
    return tuple(1e3 * np.percentile(ts, q) for q in (25, 50, 75))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C2')
    ap.add_argument('--nodes', type=int, nargs=2, default=[101, 21], help='nodes of the kept axis, of every reduced axis')
    ap.add_argument('--reps', type=int, default=7, help='alternated timed calls per engine')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--skip-fits', action='store_true')
    args = ap.parse_args()
    model = SyntheticModel.named(args.config)
    lf = model.likelihood()
    lf.set_binned_data(model.counts().reshape(model.bins))
    n_keep, n_red = args.nodes
    signal = 's0_rate_multiplier'
    fixed = {'s%d_rate_multiplier' % s: 1.0 for s in range(1, model.S)}
    keep = [(signal, np.linspace(0.0, 2.0, n_keep))]
    reduce = [(name, np.linspace(*lf.get_bounds(name), n_red)) for name in lf.shape_parameters]
    G = n_keep * n_red ** len(reduce)
    d, S = len(lf.shape_parameters), model.S
    print('%s: %d x %d^%d = %d grid points; the host engine moves (d + S + 1) x 8 = %d bytes per point over the bus, %.1f MB per call, '
          'the native engine %d bytes of nodes up and %d bytes of results down'
          % (args.config, n_keep, n_red, len(reduce), G, (d + S + 1) * 8, G * (d + S + 1) * 8 / 1e6, 8 * (n_keep + n_red * len(reduce)), 24 * n_keep))

    res = lf.grid_scan(keep=keep, reduce=reduce, **fixed)                       # warm-up: allocations, first launches
    print('engine %s: %d chunks, %d evaluations, %d evaluation launches, %d points excluded' % ((res.engine,) + tuple(res.counters[[0, 1, 3, 2]])))
    t_native, t_host = [], []
    host = None
    if not args.skip_host:
        host = lf.grid_scan(keep=keep, reduce=reduce, engine='host', **fixed)  # warm-up
    for _ in range(args.reps):
        t = time.perf_counter()
        res = lf.grid_scan(keep=keep, reduce=reduce, **fixed)                   # (returns with the results on the host: synchronised)
        t_native.append(time.perf_counter() - t)
        if not args.skip_host:
            t = time.perf_counter()
            host = lf.grid_scan(keep=keep, reduce=reduce, engine='host', **fixed)
            t_host.append(time.perf_counter() - t)
    print('native engine: median %.2f ms (quartiles %.2f / %.2f / %.2f), %.3g evaluations/s'
          % ((quartiles(t_native)[1],) + quartiles(t_native) + (G / np.median(t_native),)))
    if host is not None:
        print('host engine:   median %.2f ms (quartiles %.2f / %.2f / %.2f): x %.1f'
              % ((quartiles(t_host)[1],) + quartiles(t_host) + (np.median(t_host) / np.median(t_native),)))
        scale = np.maximum(1.0, np.abs(host.profile))
        print('largest difference between the engines: profile %.2g, log marginal %.2g (relative to max(1, |ll|)); argmax equal: %s'
              % (np.max(np.abs(res.profile - host.profile) / scale), np.max(np.abs(res.log_marginal - host.log_marginal) / scale),
                 np.array_equal(res.argmax, host.argmax)))

    print('90 %% credible upper limit on %s (flat prior, shape parameters marginalised): %.4f' % (signal, res.credible_upper_limit(0.9)))
    at = int(np.argmax(res.profile))
    print('grid profile: maximum %.4f at %s = %.3f, %s' % (res.profile[at], signal, keep[0][1][at],
                                                           ', '.join('%s = %.3f' % (n, res.best[n][at]) for n, _ in reduce)))
    if not args.skip_fits:
        sub = slice(None, None, max(1, (n_keep - 1) // 10))
        t = time.perf_counter()
        fitted = likelihood_ratio_scan(lf, (signal, keep[0][1][sub]), **fixed)
        t_fit = time.perf_counter() - t
        grid = np.max(res.profile[sub]) - res.profile[sub]
        print('likelihood_ratio_scan at %d of the kept nodes: %.1f ms; fitted minus grid -log likelihood ratio: %s'
              % (len(fitted), 1e3 * t_fit, np.array2string(fitted - grid, precision=4)))
        print('(both relative to their best among these nodes.  The grid profile is the maximum over the %d^%d reduce nodes and never lies '
              'above the true profile: where the fitted shape parameters fall between two nodes it lies below the fitted one -- finer or '
              'narrower reduce axes close the gap)' % (n_red, len(reduce)))


if __name__ == '__main__':
    main()
