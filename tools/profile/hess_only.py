"""bi_eval_hess next to bi_eval_grad on C2 at one point (kernel times from the context's profiler), and `hesse` over a 256-toy
ensemble next to the `bestfit_toys` call that fitted it -- the command for trace and counter passes on k_morph_hess.
usage: python tools/profile/hess_only.py [calls] [--no-toys]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
from blueice_amd.device import DeviceContext
from blueice_amd.inference import bestfit_toys, hesse
from blueice_amd.synthetic import SyntheticModel

calls = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
m = SyntheticModel.named('C2')
ctx = DeviceContext(0)
m.upload(ctx, threads=8)
ctx.upload_counts(m.counts())
z, r = m.random_points(1, seed=3)
times = {}
for name, fn in (('bi_eval_grad', ctx.eval_grad), ('bi_eval_hess', ctx.eval_hess)):
    fn(z, r)
    ctx.profile(True)
    t = time.perf_counter()
    for _ in range(calls):
        fn(z, r)
    dt = (time.perf_counter() - t) / calls
    n, ms = ctx.profile_read()
    ctx.profile(False)
    times[name] = ms / calls
    print('%s, C2, one point: %.3f ms per call, kernels %.3f ms (%d launches per call)' % (name, dt * 1e3, ms / calls, n // calls), flush=True)
print('Hessian / gradient kernel time: %.2f' % (times['bi_eval_hess'] / times['bi_eval_grad']), flush=True)
ctx.close()

if '--no-toys' not in sys.argv:
    lf = m.likelihood()
    lf.ctx.set_param('compact_budget', 64 << 30)
    fixed = {'s%d_rate_multiplier' % s: 1 for s in range(1, m.S)}
    lf.simulate_toys(64, seed=1)
    best, _ = lf.bestfit_toys(**fixed)
    hesse(lf, best, datasets=np.arange(64), **fixed)
    for rep in range(2):
        lf.simulate_toys(256, seed=5 + rep)
        t0 = time.perf_counter()
        best, ll = bestfit_toys(lf, **fixed)
        t1 = time.perf_counter()
        names, cov = hesse(lf, best, datasets=np.arange(256), **fixed)
        t2 = time.perf_counter()
        err = np.sqrt(np.diagonal(cov, axis1=1, axis2=2))
        print('256 C2 toys: bestfit_toys %.3f s, hesse %.3f s (+%.1f %%); %d of 256 covariances finite; median errors %s' % (
            t1 - t0, t2 - t1, 100 * (t2 - t1) / (t1 - t0), int(np.isfinite(cov).all(axis=(1, 2)).sum()),
            dict(zip(names, np.round(np.nanmedian(err, axis=0), 5)))), flush=True)
