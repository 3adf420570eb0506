"""A toy-calibrated (Neyman) band for one rate multiplier -- run as

    PYTHONPATH=. python examples/neyman_band.py [--hypotheses 16] [--toys 256] [--chunk 1024] [--anchors 3]

on a C2-like synthetic model (4 sources, three shape parameters, 100^3 bins, ~10^4 events per dataset): at each of H
hypotheses of `s0_rate_multiplier`, n toys are drawn and the profile-likelihood-ratio test statistic of every toy is
fitted; its empirical quantile is the critical value a Neyman construction uses where Wilks' theorem would say
norm.ppf(cl)**2.  Two routes to the same ensemble are timed:

(1) `neyman_thresholds`: toys of several hypotheses per generator call (`simulate_toys_points`), `chunk` toys per call of
    the fit engine, whatever hypothesis they belong to;
(2) hypothesis by hypothesis: `simulate_toys` + the same two fits per hypothesis, toy_offset advanced by hand -- the
    route the API offered before, whose calls hold the n toys of one hypothesis each.

Both draw the same toys (toy D = i n + j of the seed's ensemble), so the tables agree to the rounding of the fits.
"""
import argparse
import time

import numpy as np

from blueice_amd.inference import ToyThresholds
from blueice_amd.synthetic import SyntheticModel

ap = argparse.ArgumentParser()
ap.add_argument('--hypotheses', type=int, default=16)
ap.add_argument('--toys', type=int, default=256)
ap.add_argument('--chunk', type=int, default=1024)
ap.add_argument('--anchors', type=int, default=3, help='anchors per shape parameter (C2 itself has 5: a 4 GB tensor)')
ap.add_argument('--seed', type=int, default=1)
args = ap.parse_args()

m = SyntheticModel(4, (args.anchors,) * 3, (100, 100, 100))
t = time.perf_counter()
lf = m.likelihood()
lf.set_binned_data(m.counts().reshape(m.bins))
print('model on the device: %.1f s' % (time.perf_counter() - t))

target, cl = 's0_rate_multiplier', 0.9
fixed = dict(shape1=0., shape2=0., s2_rate_multiplier=1., s3_rate_multiplier=1.)     # profiled: s1's rate and shape0
hyp = np.linspace(0.8, 1.4, args.hypotheses)
H, n = len(hyp), args.toys

lf.toy_test_statistics(target, hyp[:2], 8, seed=args.seed + 1, kind='upper', **fixed)     # (warm-up: buffers, first launches)

t = time.perf_counter()
stats = lf.toy_test_statistics(target, hyp, n, seed=args.seed, kind='upper', chunk=args.chunk, **fixed)
dt_points = time.perf_counter() - t
table = ToyThresholds.from_statistics(stats)
print('(1) toys at mixed truths: %d hypotheses x %d toys in chunks of %d: %.3f s, %d engine calls, %d fits failed' % (
    H, n, args.chunk, dt_points, stats.engine_calls, stats.n_failed))

t = time.perf_counter()
rows, calls = [], 0
try:
    for i, h in enumerate(hyp):
        row = []
        for j0 in range(0, n, args.chunk):
            k = min(args.chunk, n - j0)
            lf.ctx.set_param('toy_offset', i * n + j0)
            lf.simulate_toys(k, seed=args.seed, **{target: h})
            ds = np.arange(k)
            start, ll_cond, info_c = lf.bestfit_batched(points={target: np.full(k, h)}, datasets=ds, return_info=True, **fixed)
            best, ll_free, info_f = lf.bestfit_batched(datasets=ds, also_from=[dict(start, **{target: np.full(k, h)})],
                                                       return_info=True, **fixed)
            calls += info_c['calls'] + info_f['calls']
            row.append(np.where(best[target] >= h, 0.0, 2 * (ll_free - ll_cond)))
        rows.append(np.concatenate(row))
finally:
    lf.ctx.set_param('toy_offset', 0)
dt_each = time.perf_counter() - t
print('(2) hypothesis by hypothesis: %d x (simulate_toys(%d) + two fits): %.3f s, %d engine calls' % (H, min(n, args.chunk), dt_each, calls))
print('    largest difference of the two tables of t: %.2e; time ratio (2) / (1): %.2f' % (
    np.abs(np.stack(rows) - stats.t).max(), dt_each / dt_points))

lf.set_binned_data(m.counts().reshape(m.bins))
print('critical values at %.0f %% (Wilks: %.3f):' % (100 * cl, 1.6424))
for h, c in zip(table.hypotheses, table.critical_values(cl)):
    print('    %s = %.3f: %.3f' % (target, h, c))
limit = lf.one_parameter_interval(target, bound=float(hyp[-1]), kind='upper', confidence_level=cl, t_ppf=table, **fixed)
wilks = lf.one_parameter_interval(target, bound=float(hyp[-1]), kind='upper', confidence_level=cl, **fixed)
print('upper limit on %s at %.0f %%: %.4f with thresholds from toys, %.4f with Wilks' % (target, 100 * cl, limit, wilks))
