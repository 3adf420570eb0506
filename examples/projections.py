"""The fitted model the way an analysis shows it: projections with the components stacked and a band from the posterior, and
goodness of fit at a binning where the test has power.  Run as

    PYTHONPATH=. python examples/projections.py [--anchors 5] [--samples 2000] [--toys 200] [--measure] [--plot proj.png]

on a C2-like synthetic model (4 sources, three shape parameters with --anchors anchors each, 100^3 bins, ~10^4 events): the
data are fitted, `sample_posterior` draws samples, and for each of the three analysis dimensions `expected_coarse_points`
returns the per-source 1-D projection at every sample -- summed over the other two dimensions on the device, a few hundred
numbers per sample instead of the 4 x 10^6 of `expected_counts_points` -- from which the 16 / 50 / 84 % bands are taken.
`goodness_of_fit(binning=)` then tests the fit on 10^3 cells of 10^3 fine bins each.

--measure times `expected_coarse_points` for 64 points (total and per source) against the only route to the same numbers
without it, `expected_counts_points` followed by the NumPy reduction, for the three projections, the 10^3 rebinning, everything summed into one cell and a
signal box: the calls alternate, medians with quartiles are printed, and the fused kernel's achieved bytes/s (template bytes inside the
cells over the time between the device events around its launches) stands against `stream_bandwidth` for the same rows.
"""
import argparse
import time

import numpy as np

from blueice_amd.coarse import CoarseBinning
from blueice_amd.synthetic import SyntheticModel

ap = argparse.ArgumentParser()
ap.add_argument('--anchors', type=int, default=5, help='anchors per shape parameter (5: the C2 tensor, 4 GB)')
ap.add_argument('--samples', type=int, default=2000, help='posterior samples the bands are made of')
ap.add_argument('--toys', type=int, default=200)
ap.add_argument('--seed', type=int, default=1)
ap.add_argument('--measure', action='store_true')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--plot', default=None, help='write the projections to this file (needs matplotlib)')
args = ap.parse_args()

m = SyntheticModel(4, (args.anchors,) * 3, (100, 100, 100))
t = time.perf_counter()
lf = m.likelihood()
lf.set_binned_data(m.counts().reshape(m.bins))
print('model on the device: %.1f s' % (time.perf_counter() - t))
S, dims = m.S, ['x0', 'x1', 'x2']
projections = {d: CoarseBinning(lf, keep=[d]) for d in dims}
rebinned = CoarseBinning(lf, rebin={d: 10 for d in dims})

# fit, then posterior samples of the floating parameters (the four rates and shape0)
fixed = dict(shape1=0., shape2=0.)
best, ll = lf.bestfit_device(**fixed)
print('best fit (ll = %.2f): ' % ll + ', '.join('%s = %.4g' % kv for kv in best.items()))
W = 32
steps = max(2, -(-2 * args.samples // W))
res = lf.sample_posterior(n_walkers=W, n_steps=steps, seed=args.seed, **fixed)
flat = res.flat(discard=steps // 2)[-args.samples:]
samples = {n: flat[:, i] for i, n in enumerate(res.names)}
samples.update({k: np.full(len(flat), v) for k, v in fixed.items()})
print('%d posterior samples (%s engine, acceptance %.2f)' % (len(flat), res.engine, res.acceptance_fraction.mean()))

t = time.perf_counter()
bands = {}
for d in dims:
    mu = lf.expected_coarse_points(projections[d], samples, per_source=True)                 # [samples, S, 100]
    stacked = np.cumsum(mu, axis=1)                                                           # components stacked
    bands[d] = np.percentile(stacked, [16, 50, 84], axis=0)                                   # [3, S, 100]
n_proj = {d: lf.coarse_counts(projections[d])[0] for d in dims}
dt = time.perf_counter() - t
print('three per-source projections at %d samples, bands and data: %.3f s (%.1f MB over the bus; the fine expectations would be %.1f GB)'
      % (len(flat), dt, 3 * len(flat) * S * 100 * 8 / 1e6, 3 * len(flat) * S * 1e6 * 8 / 1e9))
at_best = {d: lf.expected_coarse(projections[d], per_source=True, **dict(fixed, **best)) for d in dims}
for d in dims:
    total = bands[d][:, -1]
    worst = int(np.argmax(np.abs(n_proj[d] - total[1]) / np.sqrt(np.maximum(total[1], 1e-300))))
    print('  %s: %d events, expected %.1f (%s per source); widest band %.2f events; largest pull in bin %d: n = %d, mu = %.1f [%.1f, %.1f]'
          % (d, n_proj[d].sum(), at_best[d].sum(), ', '.join('%.1f' % v for v in at_best[d].sum(axis=1)),
             np.max(total[2] - total[0]), worst, n_proj[d][worst], total[1][worst], total[0][worst], total[2][worst]))

# goodness of fit on 10 x 10 x 10 cells, against the fine binning's
t = time.perf_counter()
gof = lf.goodness_of_fit(n_toys=args.toys, seed=args.seed, binning=rebinned, **fixed)
dt = time.perf_counter() - t
print('rebinned goodness of fit, %d toys in %.2f s: deviance = %.1f over %d cells, p-value from toys %.3f, from chi2(%d) %.3f'
      % (args.toys, dt, gof.observed, rebinned.n_cells, gof.p_value, gof.ndof, gof.p_value_chi2))


def quartiles(times):
    q = np.percentile(np.asarray(times) * 1e3, [25, 50, 75])
    return '%8.2f ms [%.2f, %.2f]' % (q[1], q[0], q[2])


if args.measure:
    P = 64
    rng = np.random.default_rng(5)
    pts = {'shape0': rng.uniform(-0.5, 0.5, P), 'shape1': rng.uniform(-0.5, 0.5, P), 'shape2': rng.uniform(-0.5, 0.5, P)}
    pts.update({'s%d_rate_multiplier' % s: rng.uniform(0.8, 1.2, P) for s in range(S)})
    ctx = lf.ctx
    NS = S * 2 ** sum(1 for g in ctx.anchor_z if len(g) > 1)
    ceiling = ctx.stream_bandwidth(items=P, rows=NS)
    print('stream_bandwidth(items = %d, rows = %d): %.0f GB/s' % (P, NS, ceiling))
    box = CoarseBinning(lf, keep=[], ranges={d: (40., 60.) for d in dims})        # a signal box: one cell of 20^3 fine bins
    for label, b in list(projections.items()) + [('10^3', rebinned), ('all', CoarseBinning(lf, keep=[])), ('box', box)]:
        cell = b.bin_map()
        inside = cell >= 0
        for per_source in (False, True):
            def fused():
                return lf.expected_coarse_points(b, pts, per_source=per_source)

            def through_the_host():
                mu = lf.expected_counts_points(pts, per_source=per_source)
                mu = mu.reshape(mu.shape[:-3] + (-1,))
                out = np.zeros(mu.shape[:-1] + (b.n_cells,))
                flat_mu, flat_out = mu.reshape(-1, mu.shape[-1]), out.reshape(-1, b.n_cells)
                for i in range(len(flat_mu)):
                    flat_out[i] = np.bincount(cell[inside], weights=flat_mu[i, inside], minlength=b.n_cells)
                return out.reshape(out.shape[:-1] + b.shape)

            a, c = fused(), through_the_host()                                      # warm-up, and the same numbers
            assert np.allclose(a, c, rtol=1e-10, atol=0)
            times = {'fused': [], 'host': []}
            for _ in range(args.reps):                                              # alternating
                for key, f in (('fused', fused), ('host', through_the_host)):
                    t = time.perf_counter()
                    f()
                    times[key].append(time.perf_counter() - t)
            ctx.profile(True)
            ctx.profile_read()
            fused()
            launches, ms = ctx.profile_read()
            ctx.profile(False)
            gbytes = P * NS * np.count_nonzero(inside) * 8 / 1e9
            print('%-5s %-10s fused %s   expected_counts_points + numpy %s   kernels %.2f ms in %d launches: %.0f GB/s (%.0f %% of the stream ceiling)'
                  % (label, 'per source' if per_source else 'total', quartiles(times['fused']), quartiles(times['host']), ms, launches,
                     gbytes / (ms * 1e-3), 100 * gbytes / (ms * 1e-3) / ceiling))

if args.plot:
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig, axes = plt.subplots(1, 3, figsize=(15, 4))
    centres = np.arange(100) + 0.5
    for ax, d in zip(axes, dims):
        for s in range(S):
            ax.fill_between(centres, bands[d][0, s], bands[d][2, s], alpha=0.4, step='mid')
            ax.step(centres, bands[d][1, s], where='mid', label='up to s%d' % s)
        ax.errorbar(centres, n_proj[d], yerr=np.sqrt(n_proj[d]), fmt='k.', label='data')
        ax.set_xlabel(d)
    axes[0].legend()
    fig.savefig(args.plot)
