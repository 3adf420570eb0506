#!/usr/bin/env python3
"""Golden vectors for a likelihood with Gaussian constraint terms, from the REAL reference (development container only):

    cd <an empty scratch directory> && PYTHONDONTWRITEBYTECODE=1 \
        PYTHONPATH=<repository>/tools/oracle_shims:<reference checkout>:<repository>/tests:<repository>/tests/golden:<repository> \
        python <repository>/tests/golden/make_golden_constrained.py

The model is tests/constrained_zoo.py: model_zoo.d2_nonuniform's geometry with `add_rate_uncertainty('s1', 0.3)`-style and
`log_prior=stats.norm(0.5, 0.4).logpdf` constraints, built on the reference's own classes with scipy callables.
tests/golden/constrained_d2.npz holds
    the fields of every case fixture (make_golden.py: anchor tensors, counts, call_z / call_mult / call_livetime /
    call_scale and call_ll) of the UNCONSTRAINED twin at the points of constrained_zoo.calls() -- "logL given tensors", so
    the file reads as one more binned case --, and
    constrained_ll [N]                   lf(**kw) of the constrained likelihood at the same points
    profile_axis_name / profile_axis_values, profile_fixed_names / profile_fixed_values, profile_float_names
    profile_ll [60] / profile_ll_default [60] / profile_best [60, F]
                                         bestfit_scipy per point of a scan over s0_rate_multiplier, with minimize_kwargs = TIGHT
                                         and with its default settings, as make_golden_profile.py does (nan where the
                                         reference raises OptimizationFailed)
    global_names / global_values / global_ll / global_ll_default     the fit with only PROFILE_FIXED held
"""
import os

import numpy as np

import blueice
import constrained_zoo as cz
import model_zoo
from make_golden import tensors_of
from make_golden_profile import TIGHT

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    ns = model_zoo.namespace_of('blueice')
    lf, twin = cz.constrained_d2(ns, 'scipy'), cz.constrained_d2(ns, None)
    calls = cz.calls()
    t = tensors_of(twin)
    shape_names = list(lf.shape_parameters)
    zs, mults, lts, scales = [], [], [], []
    for kw in calls:
        lt = kw.get('livetime_days', np.nan)
        mult, settings = lf._kwargs_to_settings(**{k: v for k, v in kw.items() if k != 'livetime_days'})
        zs.append([settings[n] for n in shape_names])
        mults.append(mult)
        lts.append(lt)
        scales.append(np.array(mult, dtype=float) * (1.0 if np.isnan(lt) else lt / lf.pdf_base_config['livetime_days']))
    t.update(call_z=np.asarray(zs, dtype=float), call_mult=np.asarray(mults, dtype=float), call_livetime=np.asarray(lts, dtype=float),
             call_scale=np.asarray(scales, dtype=float), call_ll=np.array([twin(**kw) for kw in calls], dtype=float),
             constrained_ll=np.array([lf(**kw) for kw in calls], dtype=float),
             allow_negative=np.array([1 if a else 0 for a in lf.source_allowed_negative]))
    name, grid = cz.PROFILE_AXIS
    fixed = cz.PROFILE_FIXED
    ll, ll_default, best, float_names = np.empty(len(grid)), np.empty(len(grid)), None, None
    for i, v in enumerate(grid):
        kw = dict(fixed, **{name: float(v)})
        # (on this model the reference's default settings can fail as well: its Nelder-Mead fallback runs out of evaluations)
        try:
            res_default, ll_default[i] = lf.bestfit_scipy(**kw)
        except blueice.exceptions.OptimizationFailed:
            res_default, ll_default[i] = None, np.nan
        try:
            res, val = lf.bestfit_scipy(minimize_kwargs=TIGHT, **kw)
        except blueice.exceptions.OptimizationFailed:
            res, val = res_default, np.nan
        if best is None:
            float_names = list(res.keys())
            best = np.full((len(grid), len(float_names)), np.nan)
        ll[i] = val
        if res is not None:
            best[i] = [res[k] for k in float_names]
    gres, gll = lf.bestfit_scipy(minimize_kwargs=TIGHT, **fixed)
    t.update(profile_axis_name=np.array(name), profile_axis_values=np.asarray(grid, dtype=float),
             profile_fixed_names=np.array(list(fixed.keys())), profile_fixed_values=np.array(list(fixed.values()), dtype=float),
             profile_float_names=np.array(float_names), profile_ll=ll, profile_ll_default=ll_default, profile_best=best,
             global_names=np.array(list(gres.keys())), global_values=np.array(list(gres.values()), dtype=float), global_ll=gll,
             global_ll_default=lf.bestfit_scipy(**fixed)[1])
    print('%d / %d profile points without a TIGHT / default fit' % (int(np.isnan(ll).sum()), int(np.isnan(ll_default).sum())))
    np.savez_compressed(os.path.join(OUT, 'constrained_d2.npz'), **t)
    print('constrained_d2: %d calls (%d finite), profile ll in [%.6f, %.6f] (%d nan), global %.9f; default settings differ by up to %.2e' % (
        len(calls), int(np.isfinite(t['constrained_ll']).sum()), np.nanmin(ll), np.nanmax(ll), int(np.isnan(ll).sum()), gll,
        np.nanmax(np.abs(ll - ll_default))))


if __name__ == '__main__':
    import scipy
    print('reference blueice', blueice.__version__, 'numpy', np.__version__, 'scipy', scipy.__version__, flush=True)
    main()
