"""The constrained model of the Gaussian-constraint tests: the geometry of model_zoo.d2_nonuniform (three sources, two shape
parameters on non-uniform anchors, a 6 x 5 space, live time 2) with a 30 % rate constraint on s1 and a normal prior
(mean 0.5, sigma 0.4) on `shift`.  Built on the reference's classes by tests/golden/make_golden_constrained.py (scipy
callables) and on blueice_amd's by tests/test_gaussian_priors_gpu.py (GaussianPrior, or scipy callables for the twin that
takes the trusted host paths).  Test infrastructure only."""
from collections import OrderedDict

import numpy as np
from scipy import stats

import model_zoo

RATE_SIGMA = 0.3                      # add_rate_uncertainty('s1', 0.3): normal(1, 0.3) on s1_rate_multiplier
SHIFT_MEAN, SHIFT_SIGMA = 0.5, 0.4
CONSTRAINED = ('s1_rate_multiplier', 'shift')

PROFILE_AXIS = ('s0_rate_multiplier', np.linspace(0.3, 2.5, 60))
PROFILE_FIXED = {'s2_rate_multiplier': 1., 'stretch': 1.5}


def constrained_d2(ns, priors='scipy'):
    """priors: 'scipy' (stats.norm(...).logpdf bound methods), 'gaussian' (blueice_amd.priors.GaussianPrior) or None (the
    unconstrained twin)."""
    rng = np.random.default_rng(12)
    space = [['x', np.array([-3., -1.5, -0.5, 0., 0.4, 1.1, 3.])], ['y', np.linspace(0, 5, 6)]]
    lf = model_zoo.morph_lf(ns, rng, 3, space, OrderedDict(shift=(-1., -0.25, 0.5, 2.), stretch=(0., 1., 4.)), 3000, 500, livetime=2.)
    if priors is None:
        return lf
    if priors == 'gaussian':
        from blueice_amd.priors import GaussianPrior
        on_rate, on_shift = GaussianPrior(1, RATE_SIGMA), GaussianPrior(SHIFT_MEAN, SHIFT_SIGMA)
    else:
        on_rate, on_shift = stats.norm(1, RATE_SIGMA).logpdf, stats.norm(SHIFT_MEAN, SHIFT_SIGMA).logpdf
    lf.add_rate_parameter('s1', log_prior=on_rate)                    # (re-registers s1: the order of the parameters stays)
    anchors, _, base_value = lf.shape_parameters['shift']
    lf.shape_parameters['shift'] = (anchors, on_shift, base_value)
    return lf


def calls():
    """~40 parameter points: the anchor box and its cells, rate multipliers (zeros among them), another live time, and
    points outside the box"""
    out = [{}]
    for z0 in (-1., -0.6, -0.25, 0.1, 0.5, 1.3, 2.):
        for z1 in (0., 1., 2.5, 4.):
            out.append(dict(shift=z0, stretch=z1))
    out += [dict(shift=0.3, stretch=3.3, s0_rate_multiplier=0.5, s1_rate_multiplier=2., s2_rate_multiplier=1.1),
            dict(shift=0.3, stretch=3.3, livetime_days=5.),
            dict(shift=0.7, stretch=0.2, s1_rate_multiplier=0.),
            dict(shift=-0.9, stretch=1.7, s0_rate_multiplier=0., s1_rate_multiplier=0.4),
            dict(s0_rate_multiplier=0., s1_rate_multiplier=0., s2_rate_multiplier=0.),
            dict(shift=1.9, stretch=3.9, s1_rate_multiplier=1.6, s2_rate_multiplier=0.7),
            dict(s1_rate_multiplier=1.),
            dict(shift=0.5, s1_rate_multiplier=0.1),
            dict(shift=2.01, stretch=1.), dict(shift=0., stretch=-0.01), dict(shift=-1.5, stretch=5., s1_rate_multiplier=1.3),
            dict(shift=1., stretch=2., s2_rate_multiplier=-1.)]
    return out
