"""The fitted model the way an analysis shows it: projections with the components stacked and a band from the posterior, and
goodness of fit at a binning where the test has power.  Run as

    PYTHONPATH=. python examples/projections.py [--anchors 5] [--samples 2000] [--toys 200] [--measure] [--plot proj.png]

on a C2-like synthetic model (4 sources, three shape parameters with --anchors anchors each, 100^3 bins, ~10^4 events): the
data are fitted, `sample_posterior` draws samples, and for each of the three analysis dimensions `expected_coarse_points`
returns the per-source 1-D projection at every sample -- summed over the other two dimensions on the device, a few hundred
numbers per sample instead of the 4 x 10^6 of `expected_counts_points` -- from which the 16 / 50 / 84 % bands are taken.
Next to the posterior's bands stand the ones `expected_coarse_band` makes from `hesse`'s covariance -- sigma_C^2 = J_C^T Sigma J_C with
J_C = d mu_C / d theta summed over the cells on the device, no chain -- and the impact table of the expectation in a signal box.
`goodness_of_fit(binning=)` then tests the fit on 10^3 cells of 10^3 fine bins each.

--measure times `expected_coarse_points` for 64 points (total and per source) against the only route to the same numbers
without it, `expected_counts_points` followed by the NumPy reduction, for the three projections, the 10^3 rebinning, everything summed into one cell and a
signal box: the calls alternate, medians with quartiles are printed, and the fused kernel's achieved bytes/s (template bytes inside the
cells over the time between the device events around its launches) stands against `stream_bandwidth` for the same rows.
A second leg times `expected_coarse_jacobian_points` at the same points against `expected_coarse_points` (the value alone: the
floor) and against the 2F + 1 calls of central differences, with the kernels' time the same way (--sources 9 --anchors 3: the
16-column variant).
"""
import argparse
import time

import numpy as np

from blueice_amd.coarse import CoarseBinning
from blueice_amd.synthetic import SyntheticModel

ap = argparse.ArgumentParser()
ap.add_argument('--anchors', type=int, default=5, help='anchors per shape parameter (5: the C2 tensor, 4 GB)')
ap.add_argument('--sources', type=int, default=4, help='sources (9 with three shape parameters: the 16-column variant of the Jacobian kernel)')
ap.add_argument('--samples', type=int, default=2000, help='posterior samples the bands are made of')
ap.add_argument('--toys', type=int, default=200)
ap.add_argument('--seed', type=int, default=1)
ap.add_argument('--measure', action='store_true')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--plot', default=None, help='write the projections to this file (needs matplotlib)')
args = ap.parse_args()

m = SyntheticModel(args.sources, (args.anchors,) * 3, (100, 100, 100))
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

# the same bands without a chain: hesse's covariance carried to the cells by d mu_C / d theta (expected_coarse_band: one pass over
# the corner rows per projection), and the impact table of the background estimate in a signal box
t = time.perf_counter()
cov_names, cov = lf.hesse(best, **fixed)
at = dict(fixed, **best)
linear = {d: lf.expected_coarse_band(projections[d], cov_names, cov, **at) for d in dims}
signal_box = CoarseBinning(lf, keep=[], ranges={d: (40., 60.) for d in dims})                  # one cell of 20^3 fine bins
box_mu, box_sigma, box_impacts = lf.expected_coarse_band(signal_box, cov_names, cov, **at)
dt = time.perf_counter() - t
print('hesse, three post-fit bands and the signal box: %.3f s' % dt)
for d in dims:
    chain = 0.5 * (bands[d][2, -1] - bands[d][0, -1])                                         # half the 16-84 % width of the total
    mu_d, sigma_d, _ = linear[d]
    widest = int(np.argmax(sigma_d))
    print('  %s: widest band in bin %d: sigma = %.3f events from hesse, %.3f from the posterior samples (mu = %.1f)'
          % (d, widest, sigma_d[widest], chain[widest], mu_d[widest]))
box_chain = lf.expected_coarse_points(signal_box, samples)
print('signal box: %.2f +- %.2f events expected (posterior samples: %.2f +- %.2f); impacts, largest first:'
      % (box_mu, box_sigma, np.median(box_chain), 0.5 * np.diff(np.percentile(box_chain, [16, 84]))[0]))
for name, shift in sorted(box_impacts.items(), key=lambda kv: -abs(kv[1])):
    print('  %-22s %+8.3f events per sigma (%.1f %% of the estimate)' % (name, shift, 100 * abs(shift) / box_mu))

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

    # The derivatives of the same views.  expected_coarse_jacobian_points against (a) expected_coarse_points (total) at the same
    # points -- the value kernel over the same bytes: the floor -- and (b) the only route to the same numbers without it, central
    # differences: 2F + 1 calls of expected_coarse_points, each of which streams every corner row again.
    names = lf._parameter_names()
    F = len(names)
    d_eff = sum(1 for g in ctx.anchor_z if len(g) > 1)
    G = 4 if 1 + d_eff + S <= 4 else 8 if 1 + d_eff + S <= 8 else 16
    print('derivatives: F = %d parameters, G = %d coefficient columns per corner row (1 + %d + %d padded)' % (F, G, d_eff, S))
    step = 1e-6
    for label, b in list(projections.items()) + [('10^3', rebinned), ('all', CoarseBinning(lf, keep=[])), ('box', box)]:
        inside = b.bin_map() >= 0

        def jacobian():
            return lf.expected_coarse_jacobian_points(b, pts)

        def value():
            return lf.expected_coarse_points(b, pts)

        def differences():
            out = [lf.expected_coarse_points(b, pts)]
            for k in names:
                h = step * (pts[k] if k.endswith('_rate_multiplier') else 1.0)
                up, down = dict(pts), dict(pts)
                up[k], down[k] = pts[k] + h, pts[k] - h
                out.append((lf.expected_coarse_points(b, up) - lf.expected_coarse_points(b, down))
                           / (up[k] - down[k]).reshape((P,) + (1,) * len(b.shape)))
            return out

        (_, mu, J), fd = jacobian(), differences()                                 # warm-up, and the same numbers
        assert np.array_equal(mu, value())
        off = max(np.max(np.abs(J[:, f] - fd[1 + f])) / np.max(np.abs(J[:, f])) for f in range(F))
        times = {'jacobian': [], 'value': [], 'differences': []}
        for _ in range(args.reps):                                                  # alternating
            for key, f in (('jacobian', jacobian), ('value', value), ('differences', differences)):
                t = time.perf_counter()
                f()
                times[key].append(time.perf_counter() - t)
        kernel = {}
        for key, f in (('jacobian', jacobian), ('value', value)):
            ctx.profile(True)
            ctx.profile_read()
            f()
            kernel[key] = ctx.profile_read()[1]
            ctx.profile(False)
        gbytes = P * NS * np.count_nonzero(inside) * 8 / 1e9
        med = {k: np.median(v) for k, v in times.items()}
        print('%-5s jacobian %s   value alone %s (x %.2f)   %d-call differences %s (x %.1f)   kernels %.2f ms: %.0f GB/s (%.0f %% of the '
              'stream ceiling; the value kernel %.2f ms, %.0f %%)   largest |J - differences| / max |J| %.1e'
              % (label, quartiles(times['jacobian']), quartiles(times['value']), med['jacobian'] / med['value'], 2 * F + 1,
                 quartiles(times['differences']), med['differences'] / med['jacobian'], kernel['jacobian'],
                 gbytes / (kernel['jacobian'] * 1e-3), 100 * gbytes / (kernel['jacobian'] * 1e-3) / ceiling,
                 kernel['value'], 100 * gbytes / (kernel['value'] * 1e-3) / ceiling, off))

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
