"""Fits and posteriors of a likelihood with Gaussian constraint terms -- run as

    PYTHONPATH=. python examples/constrained_fit.py [--priors gaussian|scipy] [--repeats 5] [--points 1024] [--toys 256]

Almost every real nuisance parameter carries a Gaussian constraint (`add_rate_uncertainty`, `add_shape_uncertainty`, or a
normal `log_prior=`).  Registered as `blueice_amd.GaussianPrior` -- directly, or through the two methods under
likelihood_config['gaussian_priors_on_device'] -- the term is added inside the native loops (bi_fit_batched_gauss,
bi_sample_stretch_gauss): no Python between the iterations of a fit, proposals and accept steps of the sampler on the
device.  Any other callable (`--priors scipy`: scipy's frozen `logpdf`, what the reference registers) is called on the host:
the C++ optimiser with a Python callback per iteration, and the NumPy engine of the sampler.

Three cases are timed on the C2 model (4 sources, 5^3 anchors, 100^3 bins) with 10 % constraints on the rates of s1, s2 and
s3: a profile of --points hypotheses over s0's rate, --toys toy fits, and a posterior of 40 walkers x 200 steps.  Every case
is run once to warm up, then --repeats times: median and range are printed.
"""
import argparse
import time

import numpy as np
from scipy import stats

from blueice_amd.synthetic import SyntheticModel

SIGMA = 0.1
SHAPES = {'shape0': 0.3, 'shape1': -0.7, 'shape2': 0.6}


def timed(label, fun, repeats):
    fun()                                                  # warm-up: allocations, first launches, plans
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        out = fun()
        ts.append(time.perf_counter() - t)
    print('%-44s median %.4f s, range %.4f - %.4f s over %d runs' % (label, np.median(ts), min(ts), max(ts), repeats), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--priors', choices=['gaussian', 'scipy'], default='gaussian')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--toys', type=int, default=256)
    ap.add_argument('--config', default='C2')
    args = ap.parse_args()
    model = SyntheticModel.named(args.config)
    lf = model.likelihood()
    lf.set_binned_data(model.counts().reshape(model.bins))
    for s in range(1, model.S):
        if args.priors == 'gaussian':
            from blueice_amd import GaussianPrior
            prior = GaussianPrior(1, SIGMA)
        else:
            prior = stats.norm(1, SIGMA).logpdf
        lf.add_rate_parameter('s%d' % s, log_prior=prior)  # (registers the source's rate again, now with its constraint)
    shapes = {k: v for k, v in SHAPES.items() if k in lf.shape_parameters}
    print('%s, constraints as %s' % (args.config, 'GaussianPrior' if args.priors == 'gaussian' else "scipy's logpdf"), flush=True)

    grid = np.linspace(0.9, 1.1, args.points)
    best, ll = timed('%d profile points (bestfit_batched)' % args.points,
                     lambda: lf.bestfit_batched(points={'s0_rate_multiplier': grid}, **shapes), args.repeats)
    print('    max ll %.6f at s0_rate_multiplier = %.4f; nuisances there: %s' % (
        ll.max(), grid[np.argmax(ll)], {k: round(float(v[np.argmax(ll)]), 5) for k, v in best.items()}))

    F = model.S
    p0 = np.random.default_rng(1).uniform(0.99, 1.01, (40, F))
    res = timed('posterior, 40 walkers x 200 steps', lambda: lf.sample_posterior(n_walkers=40, n_steps=200, p0=p0, seed=2, **shapes), args.repeats)
    print('    %s engine, acceptance %.2f, posterior means %s' % (res.engine, res.acceptance_fraction.mean(), np.round(res.flat(50).mean(axis=0), 5)))

    lf.simulate_toys(args.toys, seed=3, **shapes)
    best, ll = timed('%d toy fits (bestfit_toys)' % args.toys, lambda: lf.bestfit_toys(**shapes), args.repeats)
    print('    fitted rates: mean %s, spread %s' % ({k: round(float(v.mean()), 5) for k, v in best.items()}, {k: round(float(v.std()), 5) for k, v in best.items()}))


if __name__ == '__main__':
    main()
