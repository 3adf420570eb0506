"""An unbinned toy-MC ensemble with a fit per toy, two ways -- run as

    PYTHONPATH=. python examples/unbinned_toys.py [n_toys]

(1) the loop an unbinned analysis had to write so far: per toy `simulate_toy` (one toy drawn and scored on the device, into a
    context that holds one dataset) and `bestfit_device` (a single-problem fit);
(2) the ensemble: `toy_mc_fits` draws all toys in one call (`simulate_toys`: toy D is `simulate_toy(seed=toy_seed(seed, D))`
    event for event), keeps them side by side in one context and fits one problem per toy on the native loop.
Both draw the same toys, so the fitted maxima agree; the script prints both wall times (one warm-up run each first).
"""
import sys
import time

import numpy as np

from blueice_amd import UnbinnedLogLikelihood, toy_seed
from blueice_amd.inference import bestfit_device, toy_mc_fits
from blueice_amd.test_helpers import conf_for_test

n_toys = int(sys.argv[1]) if len(sys.argv) > 1 else 256
np.random.seed(1)
conf = conf_for_test(n_sources=2, mc=True, n_events_for_pdf=int(2e5), events_per_day=1000.,
                     analysis_space=[['x', np.linspace(-6, 6, 241)]])
conf['sources'] = [dict(name='signal', sigma=0.6, events_per_day=200.), dict(name='background', sigma=2.5)]
lf = UnbinnedLogLikelihood(conf)
lf.add_rate_parameter('signal')
lf.add_rate_parameter('background')
lf.add_shape_parameter('mu', (-1., 0., 1.))
lf.prepare()
truth = dict(mu=0.2, signal_rate_multiplier=1.1)
seed = 7


def loop(n):
    out = []
    for D in range(n):
        lf.simulate_toy(seed=toy_seed(seed, D), **truth)
        out.append(bestfit_device(lf)[1])
    return np.array(out)


def ensemble(n):
    return toy_mc_fits(lf, n, chunk=n, seed=seed, truth=truth)[1]


for name, run in (('loop of simulate_toy + bestfit_device', loop), ('toy_mc_fits (one ensemble)', ensemble)):
    run(min(8, n_toys))                                      # warm-up
    t = time.perf_counter()
    ll = run(n_toys)
    dt = time.perf_counter() - t
    print('%-40s %d toys (about %d events each): %.3f s, %.2f ms per toy; mean max ll %.4f' % (
        name, n_toys, int(np.mean(lf.n_events_per_dataset)), dt, dt / n_toys * 1e3, ll.mean()))
