"""Does the fitted model describe the data?  Run as

    PYTHONPATH=. python examples/goodness_of_fit.py [--toys 1000] [--chunk 256] [--anchors 3] [--statistic deviance] [--plot gof.png]

on a C2-like synthetic model (4 sources, three shape parameters, 100^3 bins, ~10^4 events per dataset): the data are
fitted, the goodness-of-fit statistic (the deviance against the saturated model, or Pearson's chi2) is evaluated at the
fit, and its distribution comes from toys that are drawn at the fitted values, fitted like the data and evaluated each at
its own fit -- all on the device (`lf.goodness_of_fit`).  With 10^6 bins and 10^4 events nearly every bin is empty, so the
asymptotic chi2(n_bins - n_floating) reading is far off and the toys are the answer; the script prints both, the
histogram of the toys' statistic against that chi2, and the largest pulls per bin from `lf.expected_counts`.
"""
import argparse
import time

import numpy as np
from scipy import stats

from blueice_amd.synthetic import SyntheticModel

ap = argparse.ArgumentParser()
ap.add_argument('--toys', type=int, default=1000)
ap.add_argument('--chunk', type=int, default=256)
ap.add_argument('--anchors', type=int, default=3, help='anchors per shape parameter (C2 itself has 5: a 4 GB tensor)')
ap.add_argument('--statistic', default='deviance', choices=('deviance', 'pearson'))
ap.add_argument('--seed', type=int, default=1)
ap.add_argument('--plot', default=None, help='write the histogram of the toys to this file (needs matplotlib)')
args = ap.parse_args()

m = SyntheticModel(4, (args.anchors,) * 3, (100, 100, 100))
t = time.perf_counter()
lf = m.likelihood()
lf.set_binned_data(m.counts().reshape(m.bins))
print('model on the device: %.1f s' % (time.perf_counter() - t))

fixed = dict(shape1=0., shape2=0.)                       # floating: the four rates and shape0
lf.goodness_of_fit(n_toys=8, statistic=args.statistic, chunk=8, seed=args.seed + 1, **fixed)      # (warm-up: buffers, first launches)

t = time.perf_counter()
res = lf.goodness_of_fit(n_toys=args.toys, statistic=args.statistic, chunk=args.chunk, seed=args.seed, **fixed)
dt = time.perf_counter() - t
print('%d toys drawn, fitted and evaluated in chunks of %d: %.3f s, %d fits failed' % (args.toys, args.chunk, dt, res.n_failed))
print('best fit: ' + ', '.join('%s = %.4g' % kv for kv in res.best.items()))
print('%s = %.2f with %d bins, %d floating parameters' % (res.statistic, res.observed, res.ndof + len(res.best), len(res.best)))
print('p-value from toys:       %.4f   (toys: mean %.1f, rms %.1f)' % (res.p_value, res.toys.mean(), res.toys.std()))
print('p-value from chi2(%d): %.4g   (asymptotic; chi2 mean %d -- unreliable with bins this sparse)' % (res.ndof, res.p_value_chi2, res.ndof))

# the toys' statistic against the asymptotic chi2
edges = np.linspace(min(res.toys.min(), res.observed), max(res.toys.max(), res.observed), 21)
hist, _ = np.histogram(res.toys, bins=edges)
expect = args.toys * np.diff(stats.chi2.cdf(edges, res.ndof))
print('%12s %12s %8s %12s' % ('from', 'to', 'toys', 'chi2(ndof)'))
for lo, hi, h, e in zip(edges[:-1], edges[1:], hist, expect):
    print('%12.1f %12.1f %8d %12.3g%s' % (lo, hi, h, e, '   <- observed' if lo <= res.observed <= hi else ''))

# pulls per bin at the best fit: (n - mu) / sqrt(mu) from the device's own expectation
t = time.perf_counter()
mu = lf.expected_counts(**dict(fixed, **res.best))
parts = lf.expected_counts(per_source=True, **dict(fixed, **res.best))
dt = time.perf_counter() - t
n = lf.ctx.download_counts(0).reshape(mu.shape)
with np.errstate(all='ignore'):
    pull = np.where(mu > 0, (n - mu) / np.sqrt(mu), 0.0)
print('expected counts (total and per source) read back in %.3f s: sum mu = %.1f (%s per source), %d events' % (
    dt, mu.sum(), ', '.join('%.1f' % v for v in parts.reshape(len(parts), -1).sum(axis=1)), n.sum()))
for flat in np.argsort(-np.abs(pull), axis=None)[:5]:
    idx = np.unravel_index(flat, mu.shape)
    print('  bin %s: n = %d, mu = %.3g, pull = %+.2f' % (idx, n[idx], mu[idx], pull[idx]))

if args.plot:
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    centres = 0.5 * (edges[1:] + edges[:-1])
    plt.hist(res.toys, bins=edges, histtype='step', label='%d toys' % args.toys)
    plt.plot(centres, expect, label='chi2(%d)' % res.ndof)
    plt.axvline(res.observed, color='k', label='observed, p = %.3f' % res.p_value)
    plt.xlabel(res.statistic)
    plt.legend()
    plt.savefig(args.plot)
