"""Expected errors before any data exist: the Fisher information of a C2-like model -- run as

    PYTHONPATH=. python examples/expected_errors.py [--anchors 3] [--truths 64] [--check 4] [--measure]

on a C2-like synthetic model (4 sources, three shape parameters, 100^3 bins), with source s0 as the signal.  No dataset is
ever set.

(1) the expected sigma of the signal multiplier and its correlation with the nuisances (the other rates and the shape
    parameters, all floating) at a few truths and live times: `lf.expected_covariance(livetime_days=..., **truth)`;
(2) `lf.fisher_information_points` over many truths in ONE device call (one pass over the corner rows of every truth, 16
    numbers per parameter pair back), against the same matrices from central differences of `lf.expected_counts_points` --
    8 MB per displaced point over the bus, 2 F of them per truth, reduced in NumPy -- for the first --check truths;
(3) --measure: `bi_eval_fisher` against `bi_eval_real` with its gradient (the same dense rows, the same columns) and
    `bi_eval_hess` forced onto the dense rows, 64 points per call and one, medians of alternated calls with quartiles.
"""
import argparse
import time

import numpy as np

from blueice_amd.synthetic import SyntheticModel

ap = argparse.ArgumentParser()
ap.add_argument('--anchors', type=int, default=3, help='anchors per shape parameter (C2 itself has 5: a 4 GB tensor)')
ap.add_argument('--truths', type=int, default=64)
ap.add_argument('--check', type=int, default=4, help='truths whose matrix is also formed from differences of expected counts')
ap.add_argument('--measure', action='store_true', help='time the C ABI calls instead (part 3)')
ap.add_argument('--rounds', type=int, default=31)
args = ap.parse_args()

m = SyntheticModel(4, (args.anchors,) * 3, (100, 100, 100))


def quartiles(t):
    q = np.percentile(np.asarray(t) * 1e3, [50, 25, 75])
    return '%.3f ms [%.3f, %.3f]' % tuple(q)


if args.measure:
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', 0)                   # the Hessian on the dense rows, as the other two
    m.upload(ctx, threads=4)
    ctx.upload_counts(m.counts(dense=True))      # ~10 events per bin: data that fill the bins
    z, r = m.random_points(64, seed=1)
    ctx.set_asimov_counts(z[:1], r[:1])
    for P in (64, 1):
        calls = [('bi_eval_fisher', lambda: ctx.eval_fisher(z[:P], r[:P])), ('bi_eval_real + gradient', lambda: ctx.eval_real(z[:P], r[:P])),
                 ('bi_eval_hess, dense rows', lambda: ctx.eval_hess(z[:P], r[:P]))]
        times = {name: [] for name, _ in calls}
        for rnd in range(3 + args.rounds):          # three warm-up rounds; the calls alternate inside every round
            for name, call in calls:
                t0 = time.perf_counter()
                call()                               # (every one of them ends in a stream synchronise)
                if rnd >= 3:
                    times[name].append(time.perf_counter() - t0)
        for name, _ in calls:
            print('%2d points per call, %-26s %s' % (P, name, quartiles(times[name])))
    raise SystemExit(0)

t0 = time.perf_counter()
lf = m.likelihood(livetime_days=1.0)
print('model on the device: %.1f s (no data set)' % (time.perf_counter() - t0))
target = 's0_rate_multiplier'

# (1) sigma of the signal multiplier, everything floating, and its correlations
lf.expected_covariance(**{target: 1.0})          # (warm-up)
print('(1) expected sigma(%s) and its correlations, every rate and shape parameter floating' % target)
for signal in (0.5, 1.0, 2.0):
    for days in (1.0, 4.0, 16.0):
        names, cov = lf.expected_covariance(livetime_days=days, **{target: signal})
        sigma = np.sqrt(np.diag(cov))
        j = names.index(target)
        rho = cov[j] / (sigma[j] * sigma)
        print('    signal %.1f, %4.0f days: sigma %.5f; rho with %s' % (
            signal, days, sigma[j], ', '.join('%s %+.3f' % (n.replace('_rate_multiplier', ''), c) for n, c in zip(names, rho) if n != target)))
alone = lf.expected_errors(floating=[target], **{target: 1.0})[target]
print('    signal 1.0, 1 day, the nuisances held fixed: sigma %.5f' % alone)

# (2) many truths in one call, against differences of the expected counts
rng = np.random.default_rng(3)
P = args.truths
truths = {target: rng.uniform(0.2, 2.0, P), 's1_rate_multiplier': rng.uniform(0.8, 1.2, P)}
for i, g in enumerate(m.anchor_z):
    truths['shape%d' % i] = rng.uniform(g[0], g[-1], P)
lf.fisher_information_points(truths, priors=False)
t0 = time.perf_counter()
names, info, unbounded = lf.fisher_information_points(truths, priors=False)
dt = time.perf_counter() - t0
print('(2) fisher_information_points: %d truths, %d x %d matrices, one call: %.2f ms; unbounded anywhere: %s' % (
    P, len(names), len(names), 1e3 * dt, bool(unbounded.any())))
worst, dt_diff = 0.0, 0.0
for p in range(min(args.check, P)):
    t0 = time.perf_counter()
    at = {k: float(v[p]) for k, v in truths.items()}
    x = np.array([at.get(n, 1.0) for n in names])
    h = 1e-4
    pts = {n: np.repeat(x[j], 2 * len(names) + 1) for j, n in enumerate(names)}
    for j, n in enumerate(names):          # rows 1 + 2 j and 2 + 2 j: truth displaced along parameter j (mu is multilinear in a cell)
        pts[n][1 + 2 * j] += h
        pts[n][2 + 2 * j] -= h
    mu = lf.expected_counts_points(pts).reshape(2 * len(names) + 1, -1)
    dmu = (mu[1::2] - mu[2::2]) / (2 * h)
    want = np.einsum('qb,rb->qr', dmu / mu[0], dmu)
    dt_diff += time.perf_counter() - t0
    worst = max(worst, float(np.max(np.abs(info[p] - want) / np.sqrt(np.outer(np.diag(want), np.diag(want))))))
n = max(1, min(args.check, P))
print('    the same from differences of expected_counts_points: %.1f ms per truth (%d truths checked; %.1f s for all %d), '
      'largest deviation %.2g of sqrt(I_qq I_rr)' % (1e3 * dt_diff / n, n, dt_diff / n * P, P, worst))
