"""The expected upper limit of a C2-like model and its band, two ways -- run as

    PYTHONPATH=. python examples/asimov_sensitivity.py [--toys 256] [--hypotheses 12] [--anchors 3]

on a C2-like synthetic model (4 sources, three shape parameters, 100^3 bins, ~10^4 events per dataset), with source s0 as
the signal (`s0_rate_multiplier`: 0 = background only), s1's rate and shape0 profiled:

(1) the Asimov route: `lf.expected_upper_limit(...)` -- the background-only Asimov dataset (n_b = mu_b, made on the device),
    ONE profile scan over it per band edge, sqrt(q_A(mu)) = Phi^-1(cl) + N;
(2) the toy route: n background-only toys (`simulate_toys`), every toy profiled at every hypothesis of a grid
    (`bestfit_batched`, one call per hypothesis over all toys), the limit of every toy where its t crosses Wilks' critical
    value, and the band as the quantiles Phi(N) of those limits.

The two agree within the toys' sampling error where the asymptotic formulae hold (next to the boundary at 0, the -1 sigma
edge, they need not).  (1) needs no ensemble and has no sampling error; it is not the faster one on a model with many more
bins than events: Asimov data fill every bin, so its evaluations are dense, while toys run on their non-empty bins.
"""
import argparse
import time

import numpy as np
from scipy import stats

from blueice_amd.synthetic import SyntheticModel

ap = argparse.ArgumentParser()
ap.add_argument('--toys', type=int, default=256)
ap.add_argument('--hypotheses', type=int, default=12)
ap.add_argument('--anchors', type=int, default=3, help='anchors per shape parameter (C2 itself has 5: a 4 GB tensor)')
ap.add_argument('--bound', type=float, default=0.6, help='far end of the search, in units of the signal multiplier')
ap.add_argument('--seed', type=int, default=1)
args = ap.parse_args()

m = SyntheticModel(4, (args.anchors,) * 3, (100, 100, 100))
t0 = time.perf_counter()
lf = m.likelihood()
lf.set_binned_data(m.counts().reshape(m.bins))
print('model on the device: %.1f s' % (time.perf_counter() - t0))

target, cl = 's0_rate_multiplier', 0.9
fixed = dict(shape1=0., shape2=0., s2_rate_multiplier=1., s3_rate_multiplier=1.)     # profiled: s1's rate and shape0
sigmas = (-1, 0, 1, 2)

lf.expected_upper_limit(target, args.bound, confidence_level=cl, n_sigma=(0,), **fixed)     # (warm-up: buffers, first launches)
t0 = time.perf_counter()
band = lf.expected_upper_limit(target, args.bound, confidence_level=cl, n_sigma=sigmas, **fixed)
dt_asimov = time.perf_counter() - t0
z = lf.expected_discovery_significance(target, dict(s0_rate_multiplier=1.0), **fixed)
print('(1) Asimov: expected %.0f %% upper limits on %s: %s  (%.3f s); median discovery significance at 1: %.2f sigma' % (
    100 * cl, target, ', '.join('%+d sigma: %.4f' % (n, band[n]) for n in sigmas), dt_asimov, z))

# (2) background-only toys, every toy profiled at every hypothesis
hyp = np.linspace(0.0, args.bound, args.hypotheses + 1)[1:]
n = args.toys
crit = stats.norm.ppf(cl) ** 2
t0 = time.perf_counter()
lf.simulate_toys(n, seed=args.seed, **{target: 0.0})
ds = np.arange(n)
best, ll_free = lf.bestfit_batched(datasets=ds, **fixed)
t = np.empty((len(hyp), n))
for i, h in enumerate(hyp):
    _, ll_cond = lf.bestfit_batched(points={target: np.full(n, h)}, datasets=ds, also_from=[{k: v for k, v in best.items() if k != target}], **fixed)
    t[i] = np.where(best[target] >= h, 0.0, 2 * (ll_free - ll_cond))
limits = np.full(n, np.nan)
for j in range(n):
    above = np.flatnonzero(t[:, j] >= crit)
    if len(above):
        k = above[0]
        h_lo, t_lo = (hyp[k - 1], t[k - 1, j]) if k else (0.0, 0.0)
        limits[j] = h_lo + (crit - t_lo) * (hyp[k] - h_lo) / (t[k, j] - t_lo)
dt_toys = time.perf_counter() - t0
lf.set_binned_data(m.counts().reshape(m.bins))
ok = np.isfinite(limits)
print('(2) toys: %d background-only toys x %d hypotheses: %.3f s; %d toys with a limit inside the grid' % (n, len(hyp), dt_toys, ok.sum()))
for k in sigmas:
    q = np.quantile(np.where(ok, limits, np.inf), stats.norm.cdf(k), method='higher')
    print('    %+d sigma: toys %.4f, Asimov %.4f' % (k, q, band[k]))
print('time ratio (2) / (1): %.1f' % (dt_toys / dt_asimov))
