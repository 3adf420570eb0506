"""Posterior samples of a binned likelihood's parameters on the device -- run as

    PYTHONPATH=. python examples/posterior.py [--config C2] [--walkers 40 1024] [--steps 200] [--toys 0] [--skip-host]

The reference's `bestfit_emcee` hands emcee a scalar likelihood callable: n_walkers x n_steps calls, one after the other
(blueice/inference.py:254-321).  Here a stretch move's half ensemble is one device batch, and with `sample_posterior`'s
native engine the proposals, the accept step and the chain stay on the device as well (bi_sample_stretch).

Three ways to run the same chain length are timed: the native engine, the host engine (the same algorithm and random
stream in NumPy, one `lf.eval_points` per half-step), and `eval_points_loop` below -- the plain stretch-move loop a user
could write against `lf.eval_points` before `sample_posterior` existed.
"""
import argparse
import time

import numpy as np

from blueice_amd.synthetic import SyntheticModel


def eval_points_loop(lf, names, p0, n_steps, a=2.0, seed=0, dataset=None):
    """Goodman & Weare's stretch move over `lf.eval_points`, NumPy's generator for the draws: x [W, F] -> chain [n_steps, W, F].
    dataset: index of the dataset every point is evaluated against (None: the likelihood's first)."""
    rng = np.random.default_rng(seed)
    x = np.array(p0, dtype=float)
    W, F = x.shape
    half = W // 2
    more = (lambda n: {}) if dataset is None else (lambda n: {'dataset': np.full(n, dataset, dtype=np.int64)})
    ll = np.asarray(lf.eval_points({n: x[:, v] for v, n in enumerate(names)}, **more(W)))
    chain = np.empty((n_steps, W, F))
    for t in range(n_steps):
        for h in (0, 1):
            k = np.arange(h * half, (h + 1) * half)
            j = (1 - h) * half + rng.integers(0, half, half)
            z = ((a - 1.0) * rng.random(half) + 1.0) ** 2 / a
            y = x[j] + z[:, None] * (x[k] - x[j])
            ll_y = np.asarray(lf.eval_points({n: y[:, v] for v, n in enumerate(names)}, **more(half)))
            with np.errstate(invalid='ignore'):
                take = np.isfinite(ll_y) & (np.log(rng.random(half)) < (F - 1) * np.log(z) + ll_y - ll[k])
            x[k] = np.where(take[:, None], y, x[k])
            ll[k] = np.where(take, ll_y, ll[k])
        chain[t] = x
    return chain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C2')
    ap.add_argument('--walkers', type=int, nargs='+', default=[40])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--toys', type=int, default=0, help='also: one ensemble of the first --walkers per toy dataset, in one call')
    ap.add_argument('--skip-host', action='store_true')
    args = ap.parse_args()
    model = SyntheticModel.named(args.config)
    lf = model.likelihood()
    lf.set_binned_data(model.counts().reshape(model.bins))
    names = ['s%d_rate_multiplier' % s for s in range(model.S)] + list(lf.shape_parameters)
    F = len(names)
    for W in args.walkers:
        p0 = np.random.default_rng(1).uniform(0.95, 1.05, (W, F)) * np.array([1.0] * model.S + [0.0] * (F - model.S)) + \
            np.array([0.0] * model.S + [1.0] * (F - model.S)) * np.random.default_rng(2).uniform(-0.2, 0.2, (W, 1))
        lf.sample_posterior(n_walkers=W, n_steps=2, p0=p0)                         # warm-up: allocations, first launches
        t = time.perf_counter()
        res = lf.sample_posterior(n_walkers=W, n_steps=args.steps, p0=p0)
        t_native = time.perf_counter() - t
        line = 'W = %6d, %d steps: native %.3f s (%s engine, acceptance %.2f, %d launches)' % (
            W, args.steps, t_native, res.engine, res.acceptance_fraction.mean(), res.counters[3])
        if not args.skip_host:
            t = time.perf_counter()
            lf.sample_posterior(n_walkers=W, n_steps=args.steps, p0=p0, engine='host')
            t_host = time.perf_counter() - t
            t = time.perf_counter()
            eval_points_loop(lf, names, p0, args.steps)
            t_loop = time.perf_counter() - t
            line += ', host engine %.3f s, eval_points loop %.3f s' % (t_host, t_loop)
        print(line, flush=True)
    if args.toys:
        W = args.walkers[0]
        p0 = np.random.default_rng(1).uniform(0.95, 1.05, (W, F)) * np.array([1.0] * model.S + [0.0] * (F - model.S)) + \
            np.array([0.0] * model.S + [1.0] * (F - model.S)) * np.random.default_rng(2).uniform(-0.2, 0.2, (W, 1))
        lf.simulate_toys(args.toys, seed=3)
        ds = np.arange(args.toys)
        lf.sample_posterior(n_walkers=W, n_steps=2, p0=p0, datasets=ds)
        t = time.perf_counter()
        res = lf.sample_posterior(n_walkers=W, n_steps=args.steps, p0=p0, datasets=ds)
        t_native = time.perf_counter() - t
        line = 'E = %d toys x W = %d, %d steps: native %.3f s (%s engine)' % (args.toys, W, args.steps, t_native, res.engine)
        if not args.skip_host:
            t = time.perf_counter()
            lf.sample_posterior(n_walkers=W, n_steps=args.steps, p0=p0, datasets=ds, engine='host')
            t_host = time.perf_counter() - t
            t = time.perf_counter()
            for e in range(min(args.toys, 4)):
                eval_points_loop(lf, names, p0, args.steps, dataset=e)
            t_loop = (time.perf_counter() - t) * args.toys / min(args.toys, 4)
            line += ', host engine %.3f s, eval_points loop %.3f s (from %d toys, one after the other)' % (t_host, t_loop, min(args.toys, 4))
        print(line, flush=True)


if __name__ == '__main__':
    main()
