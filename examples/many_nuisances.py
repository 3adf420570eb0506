"""A binned likelihood with many nuisance shape parameters, each moving one source -- run as

    PYTHONPATH=. python examples/many_nuisances.py [--bins 20] [--scan 33] [--toys 200] [--asimov] [--band] [--posterior] [--grid]
        [--unbinned | --unbinned-toys | --measure-unbinned | --measure-unbinned-hessian | --measure-unbinned-toys]
        [--measure | --measure-toys | --measure-asimov | --measure-coarse | --measure-coarse-jacobian | --measure-sampler [--rounds 31]]

Eight shape parameters with five anchors each and four sources that respond to two of them each.  On one tensor-product
grid that is 5^8 = 390 625 anchor models and 4 x 2^8 = 1024 template rows per evaluation, and the gradient path stops at
1 + d + S = 16 columns; `SourceWiseBinnedLogLikelihood` keeps one 5 x 5 grid per source -- 100 rows resident, 16 rows per
evaluation -- and the native fit loop floats all twelve parameters.

(1) prepare(): models at the 100 projected anchors only; set_data(): the events binned on the device;
(2) bestfit_batched: every rate and every constrained shape parameter floating;
(3) likelihood_ratio_scan over the signal's rate multiplier: --scan hypotheses profiled in lock-step (bi_fit_batched_factored);
(4) bestfit_minuit: the fit with its parabolic errors from the analytic Hessian (bi_eval_sourcewise_hess), the correlation matrix
    (inference.hesse), and expected_errors at the truth before any data (bi_eval_sourcewise_fisher);
(5) goodness_of_fit: the deviance of the data at their fit and its p-value from --toys toys drawn at the fit on the device
    (bi_sourcewise_generate_toys), each fitted in lock-step and scored (bi_eval_sourcewise_gof), beside the asymptotic reading;
(6) neyman_thresholds: the test statistic's critical values from toys at a few hypotheses of the signal's rate multiplier,
    handed to one_parameter_interval in place of Wilks' chi-square.

--asimov prints, instead of (2) - (6), the expected 90 % upper limit on the signal's rate multiplier without any data: the
-1 sigma ... +2 sigma band from the background-only Asimov dataset (blueice_amd.inference.expected_upper_limit: one profile
search per band edge on the view of blueice_amd.asimov, bi_fit_batched_sourcewise_real), and beside it the same band from
--toys background-only toys drawn on the device, every toy profiled at a ladder of hypotheses in lock-step and its own limit
read off where its test statistic crosses Wilks' threshold, then the toy-calibrated one of neyman_thresholds; wall times of all.

--measure times the C ABI instead, at a shape BOTH routes can hold: d = 4, S = 4, one own axis per source, 5 anchors, 100^3
bins, dense data, 64 points per call -- bi_eval_factored with its gradient (8 rows per point) against bi_eval_grad on the
expanded 5^4 grid (64 rows per point; 20 GB of templates), alternated calls, medians with quartiles, and the kernel's bytes
per second against the stream_bandwidth(items = 64, rows = 8) probe of the same device.  Then the second-order calls at the same
shape: bi_eval_sourcewise_hess against the (2 F + 1) P gradient points of the central differences it replaces (one bi_eval_factored
call, as the class takes them) and against bi_eval_hess on the expanded grid, bi_eval_sourcewise_fisher against bi_eval_fisher
there; and both on a panelled class (8 sources x 2 own axes of the same 4, four Gram panels), which only the source-wise route holds.

--measure-toys times, at the same source-wise shape (no expanded grid is built), bi_eval_sourcewise_gof against bi_eval_factored
values-only, bi_sourcewise_expected_counts against the bytes it must write, and bi_sourcewise_generate_toys for 64 toys against
numpy.random.Generator.poisson on the same expectation on the host plus the upload through bi_factored_set_counts.

--measure-asimov times, at the same source-wise shape, bi_eval_sourcewise_real with and without its gradient against
bi_eval_factored with and without its gradient and against bi_eval_sourcewise_gof, all on the same rows (the same counts in the
real-valued store and in the ordinary one), at 64 points per call and at one, and the kernels alone by device events.

--measure-coarse times, at the same source-wise shape, bi_sourcewise_expected_coarse (the projection on the first analysis axis, the
10^3 rebinning and everything in one cell; total and per source) against bi_sourcewise_expected_counts plus the NumPy reduction it
replaces, and k_sourcewise_coarse with its finish kernel alone, by device events, against k_sourcewise_expect on the same points.

--band prints, after the fit (2) and inference.hesse over all twelve parameters, the post-fit uncertainty band of the projection on
the first analysis axis and the impact table of a signal box -- which nuisance moves which source's events in the box by how much
-- from ONE device call each (blueice_amd.coarse.sourcewise_coarse_band, sourcewise_coarse_jacobian(per_source=True);
bi_sourcewise_expected_coarse_jacobian), beside the same numbers from central differences of expected_coarse_points.

--measure-coarse-jacobian times, at the same source-wise shape, bi_sourcewise_expected_coarse_jacobian (total and per source) for the x0
projection, the 10^3 rebinning, one cell and a box, against bi_sourcewise_expected_coarse on the same points and against the
(2 F + 1) P-point bi_sourcewise_expected_coarse call of the central differences it replaces, and the kernel pairs alone by device events.

--posterior draws, instead of (2) - (6), a chain over all twelve parameters with their constraints (blueice_amd.sampler.sample_posterior:
bi_sample_stretch_sourcewise, the proposals planned on the device) and prints the 90 % credible upper limit on the signal's
multiplier beside one_parameter_interval's, and the posterior band of the projection on the first analysis axis from one
blueice_amd.coarse.expected_coarse_points call over draws of the chain.

--measure-sampler times, at the same source-wise shape, bi_sample_stretch_sourcewise against the host engine (the same move in
NumPy, one bi_eval_factored call per half-step) at 40 and 1024 walkers for 50 steps, and bi_eval_sourcewise_planned against
bi_eval_factored values-only at 1, 64 and 4096 points per call; the lines go to profiles/sourcewise_sampler_measure.txt too.

--measure-nonempty times, at the same shape, the non-empty-bin form of the data (bi_sourcewise_build_nonempty) against the dense
store on the same context at 10^3 ... 2.5 10^5 events in the 10^6 bins: bi_eval_factored, its kernels alone, the build, the
sampler and a lock-step iteration over 256 toys; the lines go to profiles/sourcewise_nonempty_measure.txt too.

--grid computes, instead of (2) - (6), the 90 % credible upper limit on the signal's multiplier from a gridded likelihood
(blueice_amd.grid.grid_scan on the source-wise model: bi_grid_reduce_sourcewise, on the matrix-core scan route and on the per-point
route), marginalised over one nuisance parameter and two background multipliers with the others fixed, and prints it beside the
same quantile of a chain over the same four parameters (blueice_amd.sampler.sample_posterior).

--measure-grid times, at the measured source-wise shape with Poisson data of 10^4 events, bi_grid_reduce_sourcewise on its two routes
against the host engine on a grid of about 10^6 points, bi_eval_sourcewise_scan against bi_eval_factored values-only at 4096 and 10^6
points of one cell tuple, and the planner's share of a call by device events; the lines go to profiles/sourcewise_scan_measure.txt too.

--unbinned fits, instead of (2) - (6), the same twelve parameters over the EVENTS (SourceWiseUnbinnedLogLikelihood: the event store of
bi_sourcewise_score_events, k_sourcewise_events) with the sources' pdfs taken from histograms, and runs one profile scan of the
signal's multiplier, then bestfit_minuit with the errors of all twelve parameters from both routes: the analytic Hessian over the event
store (likelihood_config['analytic_hessian'] = True: bi_eval_sourcewise_events_hess) and differences of the analytic gradient (the
default).  The full-grid unbinned route would hold 5^8 anchors x 4 sources x N values.

--measure-unbinned times, at the measured source-wise shape with 10^4 and 10^6 events, bi_eval_factored on the event store against
bi_eval_grad / bi_eval on the same model expanded to the 5^4 unbinned grid model, and bi_sourcewise_score_events against
bi_score_events on the expanded templates; the lines go to profiles/sourcewise_events_measure.txt too.

--measure-unbinned-hessian times, at the same shape and numbers of events, bi_eval_sourcewise_events_hess against the one bi_eval_factored
gradient call over the (2 F + 1) P points it replaces and against bi_eval_hess on the expanded unbinned grid model, and the kernels alone by
device events; the lines go to profiles/sourcewise_events_curv_measure.txt too.

--unbinned-toys draws a small ensemble of event-level toys of the twelve-nuisance model (twelve shape parameters of five anchors, six
histogram sources: no grid model exists) on the device, fits all of them, and prints the toy-calibrated critical value of an upper
limit on one rate multiplier beside Wilks' (sourcewise_event_toys, inference.bestfit_toys, inference.neyman_thresholds).

--measure-unbinned-toys times, at the measured source-wise shape, bi_sourcewise_simulate_event_toys (256 toys of 10^4 expected events,
one toy of 10^6) against bi_simulate_event_toys on the expanded 5^4 grid model and against the host route, and the device time of
the call's four parts; the lines go to profiles/sourcewise_event_toys_measure.txt too.

--unbinned-posterior computes, instead of (2) - (6), the 90 % credible upper limit on the signal's multiplier of the EVENT model from a
gridded likelihood (blueice_amd.grid.grid_scan on SourceWiseUnbinnedLogLikelihood: bi_grid_reduce_sourcewise_events), on the native and
on the host engine, beside the same quantile of a chain (blueice_amd.sampler.sample_posterior: bi_sample_stretch_sourcewise_events).

--measure-unbinned-grid and --measure-unbinned-sampler time, at the measured source-wise shape with 10^4 and 10^6 events,
bi_grid_reduce_sourcewise_events and bi_sample_stretch_sourcewise_events (40 and 1024 walkers) against the host engines on the same
event store; the lines go to profiles/sourcewise_events_scan_measure.txt and profiles/sourcewise_events_sampler_measure.txt too.
"""
import argparse
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--bins', type=int, default=20, help='bins per analysis axis (two axes)')
ap.add_argument('--scan', type=int, default=33, help='hypotheses of the profile scan')
ap.add_argument('--measure', action='store_true', help='time bi_eval_factored against bi_eval_grad on the expanded grid')
ap.add_argument('--measure-toys', action='store_true', help='time the goodness-of-fit, expected-counts and toy-generator calls')
ap.add_argument('--measure-asimov', action='store_true', help='time bi_eval_sourcewise_real against bi_eval_factored on the same rows')
ap.add_argument('--measure-coarse', action='store_true', help='time bi_sourcewise_expected_coarse against expected_counts + the NumPy reduction')
ap.add_argument('--measure-coarse-jacobian', action='store_true',
                help='time bi_sourcewise_expected_coarse_jacobian against bi_sourcewise_expected_coarse and the central differences it replaces')
ap.add_argument('--posterior', action='store_true', help='a posterior chain over all twelve parameters: credible limit and projection band')
ap.add_argument('--measure-sampler', action='store_true',
                help='time bi_sample_stretch_sourcewise against the host engine, and bi_eval_sourcewise_planned against bi_eval_factored')
ap.add_argument('--measure-nonempty', action='store_true',
                help='time the non-empty-bin form of the data against the dense store on the same context (sourcewise_form)')
ap.add_argument('--grid', action='store_true',
                help='a credible upper limit on the signal multiplier from a gridded likelihood, marginalised over three nuisances, beside the chain\'s')
ap.add_argument('--measure-grid', action='store_true',
                help='time bi_grid_reduce_sourcewise on its two routes against the host engine, and bi_eval_sourcewise_scan against bi_eval_factored')
ap.add_argument('--unbinned', action='store_true', help='fit the twelve parameters over events (unbinned source-wise likelihood) and scan the signal multiplier')
ap.add_argument('--measure-unbinned', action='store_true',
                help='time bi_eval_factored on the event store against the expanded unbinned grid model, and the two scoring calls')
ap.add_argument('--measure-unbinned-hessian', action='store_true',
                help='time bi_eval_sourcewise_events_hess against the gradient differences it replaces and bi_eval_hess on the expanded unbinned grid model')
ap.add_argument('--unbinned-toys', action='store_true',
                help='draw and fit a small ensemble of event-level toys of the twelve-nuisance model: a toy-calibrated threshold beside Wilks\'')
ap.add_argument('--measure-unbinned-toys', action='store_true',
                help='time bi_sourcewise_simulate_event_toys against the expanded grid model\'s generator and the host route')
ap.add_argument('--unbinned-posterior', action='store_true',
                help='a credible upper limit on the signal multiplier of the event model from grid_scan, beside one from sample_posterior')
ap.add_argument('--measure-unbinned-grid', action='store_true',
                help='time bi_grid_reduce_sourcewise_events against the host engine on the same event store')
ap.add_argument('--measure-unbinned-sampler', action='store_true',
                help='time bi_sample_stretch_sourcewise_events against the host engine on the same event store')
ap.add_argument('--band', action='store_true', help='the post-fit band of a projection and the impact table of a signal box')
ap.add_argument('--asimov', action='store_true', help='the expected upper-limit band from the Asimov dataset, and from toys')
ap.add_argument('--toys', type=int, default=200, help='toys of the goodness-of-fit p-value; a fifth as many per Neyman hypothesis')
ap.add_argument('--rounds', type=int, default=31)
ap.add_argument('--measure-bins', type=int, default=100, help='bins per axis (three axes) of the measured shape')
args = ap.parse_args()


def quartiles(t):
    q = np.percentile(np.asarray(t) * 1e3, [50, 25, 75])
    return '%.3f ms [%.3f, %.3f]' % tuple(q)


def measure():
    from blueice_amd.device import DeviceContext
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, B, P = 5, args.measure_bins ** 3, 64
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = 2.5e6 * (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])          # ~10 events per bin in all
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    full = DeviceContext(0)
    t0 = time.perf_counter()
    full.begin_model([g] * d, S, B)
    for lin, idx in enumerate(np.ndindex(*(n_a,) * d)):          # the same likelihood on the product grid: source s from ITS anchor
        full.set_anchor(lin, np.stack([rows[s, idx[s]] for s in range(S)]), np.array([mus[s, idx[s]] for s in range(S)]))
    full.end_model()
    print('expanded grid resident: %d anchor models, %.1f GB, %.1f s to stream; source-wise: %d rows, %.2f GB'
          % (n_a ** d, n_a ** d * S * B * 8 / 1e9, time.perf_counter() - t0, S * n_a, S * n_a * B * 8 / 1e9), flush=True)
    z = rng.uniform(-1.9, 1.9, (P, d))
    r = rng.uniform(0.8, 1.2, (P, S))
    mid = n_a // 2
    counts = rng.poisson(sum(mus[s, mid] * rows[s, mid] for s in range(S))).astype(float)
    fac.set_counts(counts)
    full.upload_counts(counts)
    a, b = fac.eval_grad(z, r), full.eval_grad(z, r)
    print('agreement of the two routes over %d points: max |ll difference| / |ll| %.2g, max |gradient difference| %.2g of the largest entry'
          % (P, np.max(np.abs(a[0] - b[0]) / np.abs(b[0])), max(np.max(np.abs(a[1] - b[1])), np.max(np.abs(a[2] - b[2]))) /
             max(np.max(np.abs(b[1])), np.max(np.abs(b[2])))))
    calls = [('bi_eval_factored + gradient', lambda: fac.eval_grad(z, r)), ('bi_eval_grad, expanded 5^%d grid' % d, lambda: full.eval_grad(z, r)),
             ('bi_eval_factored, values', lambda: fac.eval(z, r)), ('bi_eval, expanded grid', lambda: full.eval(z, r))]
    times = {name: [] for name, _ in calls}
    for rnd in range(3 + args.rounds):              # three warm-up rounds; the calls alternate inside every round
        for name, call in calls:
            t0 = time.perf_counter()
            call()                                   # (every one of them ends in a stream synchronise)
            if rnd >= 3:
                times[name].append(time.perf_counter() - t0)
    for name, _ in calls:
        print('%2d points per call, %-34s %s' % (P, name, quartiles(times[name])))
    # the kernels alone, from device events around the launches, in a pass of their own
    Bp = (B + 511) // 512 * 512
    for name, ctx, call, n_rows in (('k_morph_factored', fac._dev, calls[0][1], 2 * S + 1), ('expanded route', full, calls[1][1], S * 2 ** d + 1)):
        ctx.profile(True)
        ks = []
        for _ in range(args.rounds):
            call()
            ks.append(ctx.profile_read()[1] * 1e-3)
        ctx.profile(False)
        med = np.median(ks)
        print('%-18s kernels %s per call: %d rows (counts included) x %d bins x 8 bytes x %d points = %.2f GB -> %.2f TB/s'
              % (name, quartiles(ks), n_rows, Bp, P, n_rows * Bp * 8 * P / 1e9, n_rows * Bp * 8 * P / med / 1e12))
    for nt in (True, False):
        print('stream_bandwidth(items = 64, rows = 8, nontemporal = %s): %.2f TB/s' % (nt, full.stream_bandwidth(items=64, rows=8, nontemporal=nt) / 1e3))
    measure_curvature(fac, full, z, r, d, S, P, rng, g, B)


def alternate(calls, P):
    times = {name: [] for name, _ in calls}
    for rnd in range(3 + args.rounds):              # three warm-up rounds; the calls alternate inside every round
        for name, call in calls:
            t0 = time.perf_counter()
            call()
            if rnd >= 3:
                times[name].append(time.perf_counter() - t0)
    for name, _ in calls:
        print('%2d points per call, %-58s %s' % (P, name, quartiles(times[name])), flush=True)


def measure_curvature(fac, full, z, r, d, S, P, rng, g, B):
    F = d + S
    a, b = fac.eval_hess(z, r), full.eval_hess(z, r)
    i1, i2 = fac.eval_fisher(z, r), full.eval_fisher(z, r)
    print('agreement over %d points: max |Hessian difference| %.2g, max |information difference| %.2g of the largest entry'
          % (P, np.max(np.abs(a[3] - b[3])) / np.max(np.abs(b[3])), np.max(np.abs(i1[0] - i2[0])) / np.max(np.abs(i2[0]))))
    # the points of central gradient differences: every point itself and displaced along each of the F parameters, both ways
    zz, rr = np.tile(z, (2 * F + 1, 1)), np.tile(r, (2 * F + 1, 1))
    for j in range(F):
        for k, sign in enumerate((1.0, -1.0)):
            rows = slice((1 + 2 * j + k) * P, (2 + 2 * j + k) * P)
            if j < d:
                zz[rows, j] = np.clip(zz[rows, j] + sign * 1e-4, -2.0, 2.0)
            else:
                rr[rows, j - d] += sign * 1e-5
    alternate([('bi_eval_sourcewise_hess', lambda: fac.eval_hess(z, r)),
               ('bi_eval_factored + gradient at (2 F + 1) P = %d points' % len(zz), lambda: fac.eval_grad(zz, rr)),
               ('bi_eval_hess, expanded 5^%d grid' % d, lambda: full.eval_hess(z, r)),
               ('bi_eval_sourcewise_fisher', lambda: fac.eval_fisher(z, r)),
               ('bi_eval_fisher, expanded grid', lambda: full.eval_fisher(z, r))], P)
    full.close()
    fac.close()
    # a panelled class: 8 sources that own two of the four axes each (24 basis columns, four Gram panels of two sources)
    from blueice_amd.source_wise import SourceWiseContext
    own = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0, 1), (2, 3)]
    n_a = len(g)
    pan = SourceWiseContext(0)
    pan.begin_model([g] * d, 8, B, own)
    total = np.zeros(B)
    for s in range(8):
        for k in range(n_a * n_a):
            row = rng.random(B) + 0.05
            row /= row.sum()
            mu = 1.25e6 * (1 + s % 4) * (1 + 0.02 * g[k // n_a]) * (1 + 0.01 * g[k % n_a])
            pan.set_anchor(s, k, row, mu)
            if k == (n_a * n_a) // 2:
                total += mu * row
    pan.end_model()
    pan.set_counts(rng.poisson(total).astype(float))
    r8 = rng.uniform(0.8, 1.2, (P, 8))
    print('panelled class <8, 2>: %d rows, %.2f GB resident, 32 rows per point, four launches per call' % (8 * n_a * n_a, 8 * n_a * n_a * B * 8 / 1e9))
    alternate([('bi_eval_sourcewise_hess, <8, 2> in four panels', lambda: pan.eval_hess(z, r8)),
               ('bi_eval_factored + gradient, <8, 2>', lambda: pan.eval_grad(z, r8)),
               ('bi_eval_sourcewise_fisher, <8, 2> in four panels', lambda: pan.eval_fisher(z, r8))], P)
    pan.close()


def measure_toys():
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, B, P = 5, args.measure_bins ** 3, 64
    Bp = (B + 511) // 512 * 512
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = 2.5e6 * (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])          # ~10 events per bin in all
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    z = rng.uniform(-1.9, 1.9, (P, d))
    r = rng.uniform(0.8, 1.2, (P, S))
    mid = n_a // 2
    fac.set_counts(rng.poisson(sum(mus[s, mid] * rows[s, mid] for s in range(S))).astype(float))
    print('source-wise model: %d rows, %.2f GB resident (it stays in the 256 MB Infinity Cache: every figure below is cache-assisted)'
          % (S * n_a, S * n_a * Bp * 8 / 1e9), flush=True)
    half, pearson, _ = fac.eval_gof(z, r)
    ll, _ = fac.eval(z, r)
    print('deviance of the %d points: %.6g .. %.6g; ll %.6g .. %.6g' % (P, 2 * half.min(), 2 * half.max(), ll.min(), ll.max()))
    truth_z, truth_r = np.tile(z[:1], (1, 1)), np.tile(r[:1], (1, 1))

    def host_toys():
        mu = fac.expected_counts(truth_z, truth_r)[0]
        fac.set_counts(np.random.default_rng(5).poisson(mu, size=(64, B)).astype(float))

    def host_toys_draw_only():
        np.random.default_rng(5).poisson(mu_host, size=(64, B))

    mu_host = fac.expected_counts(truth_z, truth_r)[0]
    alternate([('bi_eval_sourcewise_gof', lambda: fac.eval_gof(z, r)),
               ('bi_eval_factored, values', lambda: fac.eval(z, r)),
               ('bi_sourcewise_expected_counts (with its download of %.2f GB)' % (P * B * 8 / 1e9), lambda: fac.expected_counts(z, r)),
               ('bi_sourcewise_expected_counts, one point', lambda: fac.expected_counts(truth_z, truth_r))], P)
    rounds, args.rounds = args.rounds, max(3, args.rounds // 10)         # the host route takes seconds per call
    alternate([('bi_sourcewise_generate_toys, 64 toys at one truth', lambda: fac.generate_toys_points(truth_z, truth_r, [64], 7)),
               ('numpy poisson of 64 x B on the host + bi_factored_set_counts', host_toys),
               ('    of which numpy.random.Generator.poisson alone', host_toys_draw_only)], 1)
    args.rounds = rounds
    # the kernels alone, from device events around the launches, in a pass of their own
    dev = fac._dev
    for name, call, gb in (('k_sourcewise_gof', lambda: fac.eval_gof(z, r), (2 * S + 1) * Bp * 8 * P / 1e9),
                           ('k_morph_factored, values', lambda: fac.eval(z, r), (2 * S + 1) * Bp * 8 * P / 1e9),
                           ('k_sourcewise_expect', lambda: fac.expected_counts(z, r), (2 * S + 1) * Bp * 8 * P / 1e9),
                           ('toy generator kernels', lambda: fac.generate_toys_points(truth_z, truth_r, [64], 7), (2 * 64 + 2 * S + 4) * Bp * 8 / 1e9)):
        dev.profile(True)
        ks = []
        for _ in range(args.rounds):
            call()
            ks.append(dev.profile_read()[1] * 1e-3)
        dev.profile(False)
        print('%-26s kernels %s per call; %.2f GB read and written -> %.2f TB/s' % (name, quartiles(ks), gb, gb / np.median(ks) / 1e3), flush=True)
    print('(bytes: gof and values read 2 S rows and the counts per point; expect reads 2 S rows and writes one; the generator writes 64 rows, '
          'reads them once for the lgamma sums, and reads 2 S rows and reads and writes mu and exp(-mu))')
    print('not measured: the panelled classes <8, 2> and <8, 3>, per_source = 1, more than one truth per generator call')
    fac.close()


def measure_coarse():
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    nb = args.measure_bins
    n_a, B, P = 5, nb ** 3, 64
    Bp = (B + 511) // 512 * 512
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = 2.5e6 * (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])          # ~10 events per bin in all
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    z = rng.uniform(-1.9, 1.9, (P, d))
    r = rng.uniform(0.8, 1.2, (P, S))
    print('source-wise model: %d rows, %.2f GB resident (it stays in the 256 MB Infinity Cache: every figure below is cache-assisted)'
          % (S * n_a, S * n_a * Bp * 8 / 1e9), flush=True)
    shape = (nb, nb, nb)
    fine, whole = np.arange(nb + 1), np.array([0, nb])
    k = max(nb // 10, 1)
    tens = np.array(list(range(0, nb, k)) + [nb])
    m = len(tens) - 1
    even = nb % k == 0
    views = [('x0 projection (%d cells)' % nb, [fine, whole, whole], lambda mu: mu.reshape(mu.shape[:-1] + shape).sum(axis=(-2, -1))),
             ('%d^3 rebinning' % m, [tens, tens, tens],
              (lambda mu: mu.reshape(mu.shape[:-1] + (m, k, m, k, m, k)).sum(axis=(-5, -3, -1)).reshape(mu.shape[:-1] + (m ** 3,))) if even else None),
             ('everything in one cell', [whole, whole, whole], lambda mu: mu.sum(axis=-1, keepdims=True))]
    dev = fac._dev
    gb = 2 * S * Bp * 8 * P / 1e9                     # the rows a call reads: two corner rows per source and point
    for label, groups, reduce_host in views:
        cells = fac.set_coarse_binning(shape, groups)
        got, _ = fac.expected_coarse(cells, z, r)
        if reduce_host is not None:
            want = reduce_host(fac.expected_counts(z, r))
            print('%s: max |device - host reduction| / value %.2g' % (label, np.max(np.abs(got - want) / want)), flush=True)
        calls = [('expected_coarse, %s' % label, lambda: fac.expected_coarse(cells, z, r)),
                 ('expected_coarse per source, %s' % label, lambda: fac.expected_coarse(cells, z, r, per_source=True))]
        if reduce_host is not None:
            calls.append(('expected_counts (%.2f GB down) + numpy sum, %s' % (P * B * 8 / 1e9, label), lambda: reduce_host(fac.expected_counts(z, r))))
        alternate(calls, P)
        for name, call in (('k_sourcewise_coarse + finish', calls[0][1]), ('k_sourcewise_coarse<PS> + finish', calls[1][1]),
                           ('k_sourcewise_expect', lambda: fac.expected_counts(z, r))):
            dev.profile(True)
            ks = []
            for _ in range(args.rounds):
                call()
                ks.append(dev.profile_read()[1] * 1e-3)
            dev.profile(False)
            print('%-32s kernels %s per call; %.2f GB of rows read -> %.2f TB/s' % (name, quartiles(ks), gb, gb / np.median(ks) / 1e3), flush=True)
    rounds, args.rounds = args.rounds, max(3, args.rounds // 10)         # the per-source fine route moves 2 GB and takes a second per call
    project = views[0][2]
    fac.set_coarse_binning(shape, views[0][1])
    alternate([('expected_coarse per source, x0 projection', lambda: fac.expected_coarse(nb, z, r, per_source=True)),
               ('expected_counts per source (%.2f GB down) + numpy sum' % (P * S * B * 8 / 1e9), lambda: project(fac.expected_counts(z, r, per_source=True)))], P)
    args.rounds = rounds
    print('(k_sourcewise_expect also writes %.2f GB, which k_sourcewise_coarse does not)' % (P * Bp * 8 / 1e9))
    print('not measured: the other kernel classes (more sources, more own axes), other shapes, coarse_counts, ranges and irregular groups')
    fac.close()


def measure_coarse_jacobian():
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    F = d + S
    nb = args.measure_bins
    n_a, B, P = 5, nb ** 3, 64
    Bp = (B + 511) // 512 * 512
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = 2.5e6 * (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])          # ~10 events per bin in all
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    z = rng.uniform(0.1, 0.9, (P, d)) + rng.integers(-2, 2, (P, d))              # strictly inside cells: the differences stay in them
    r = rng.uniform(0.8, 1.2, (P, S))
    print('source-wise model: %d rows, %.2f GB resident (it stays in the 256 MB Infinity Cache: every figure below is cache-assisted)'
          % (S * n_a, S * n_a * Bp * 8 / 1e9), flush=True)
    # the points of central differences: every point itself and displaced along each of the F parameters, both ways
    hz, hr = 1e-3, 1e-3
    zz, rr = np.tile(z, (2 * F + 1, 1)), np.tile(r, (2 * F + 1, 1))
    for j in range(F):
        for k, sign in enumerate((1.0, -1.0)):
            at = slice((1 + 2 * j + k) * P, (2 + 2 * j + k) * P)
            if j < d:
                zz[at, j] += sign * hz
            else:
                rr[at, j - d] += sign * hr
    shape = (nb, nb, nb)
    fine, whole = np.arange(nb + 1), np.array([0, nb])
    k = max(nb // 10, 1)
    tens = np.array(list(range(0, nb, k)) + [nb])
    box = np.array([nb // 4, max(3 * nb // 4, nb // 4 + 1)])
    views = [('x0 projection (%d cells)' % nb, [fine, whole, whole]), ('%d^3 rebinning' % (len(tens) - 1), [tens, tens, tens]),
             ('everything in one cell', [whole, whole, whole]), ('a box of %d^3 bins' % (box[1] - box[0]), [box, box, box])]
    dev = fac._dev
    slower = []
    for label, groups in views:
        cells = fac.set_coarse_binning(shape, groups)
        inside = np.prod([float(e[-1] - e[0]) / nb for e in groups])
        gb = 2 * S * B * inside * 8 * P / 1e9         # the bins a call reads: two corner rows per source and point, inside the binning's ranges
        mu, jac, _ = fac.expected_coarse_jacobian(cells, z, r)
        mu_s, jac_s, _ = fac.expected_coarse_jacobian(cells, z, r, per_source=True)
        stencil = fac.expected_coarse(cells, zz, rr)[0].reshape(2 * F + 1, P, cells)
        diff = np.stack([(stencil[1 + 2 * j] - stencil[2 + 2 * j]) / (2 * (hz if j < d else hr)) for j in range(F)], axis=1)
        print('%s: mu bitwise bi_sourcewise_expected_coarse: %s; max |jac - central difference| %.2g of the largest entry; max |sum of the '
              'sources - total| %.2g of it' % (label, np.array_equal(mu, stencil[0]), np.max(np.abs(jac - diff)) / np.max(np.abs(diff)),
                                               np.max(np.abs(jac_s.sum(axis=1) - jac)) / np.max(np.abs(jac))), flush=True)
        calls = [('expected_coarse_jacobian, %s' % label, lambda: fac.expected_coarse_jacobian(cells, z, r)),
                 ('expected_coarse_jacobian per source, %s' % label, lambda: fac.expected_coarse_jacobian(cells, z, r, per_source=True)),
                 ('expected_coarse, %s' % label, lambda: fac.expected_coarse(cells, z, r)),
                 ('expected_coarse at (2 F + 1) P = %d points, %s' % (len(zz), label), lambda: fac.expected_coarse(cells, zz, rr))]
        times = {name: [] for name, _ in calls}
        for rnd in range(3 + args.rounds):              # three warm-up rounds; the calls alternate inside every round
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                if rnd >= 3:
                    times[name].append(time.perf_counter() - t0)
        for name, _ in calls:
            print('%2d points per call, %-72s %s' % (P, name, quartiles(times[name])), flush=True)
        med = [np.median(times[name]) for name, _ in calls]
        print('    Jacobian / mu alone %.2f (per source %.2f); central differences / Jacobian %.2f' % (med[0] / med[2], med[1] / med[2], med[3] / med[0]))
        if not med[0] < med[3]:
            slower.append(label)
        for name, call in (('k_sourcewise_coarse_jac + finish', calls[0][1]), ('k_sourcewise_coarse + finish', calls[2][1]),
                           ('k_sourcewise_coarse + finish, (2 F + 1) P points', calls[3][1])):
            dev.profile(True)
            ks = []
            for _ in range(args.rounds):
                call()
                ks.append(dev.profile_read()[1] * 1e-3)
            dev.profile(False)
            n_gb = gb * (2 * F + 1 if name.endswith('points') else 1)
            print('%-50s kernels %s per call; %.2f GB of rows read -> %.2f TB/s' % (name, quartiles(ks), n_gb, n_gb / np.median(ks) / 1e3), flush=True)
    print('the Jacobian call is faster than the central-difference call at every binning: %s' % ('yes' if not slower else 'NO (%s)' % ', '.join(slower)))
    print('not measured: the other kernel classes (more sources, more own axes: up to 33 sums per lane in three passes through LDS), '
          'shapes beyond the Infinity Cache, more shape parameters than sources own (they cost the host contraction alone)')
    fac.close()


def band():
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood, coarse, inference
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins))
    lf = SourceWiseBinnedLogLikelihood(conf)
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(3)
    lf.set_data(lf.base_model.simulate())
    best, ll = inference.bestfit_device(lf)
    cov_names, cov = inference.hesse(lf, best)
    print('fit of %d parameters: max ll %.4f; covariance from the analytic Hessian (inference.hesse)' % (len(best), ll))
    space = lf.base_model.config['analysis_space']
    (x, ex), (y, ey) = [(str(n), np.asarray(e, dtype=float)) for n, e in space]
    nb = args.bins

    def differences(binning, per_source):
        """central differences of expected_coarse_points around the fit, h = 1e-3 (of the value for a multiplier): 2 F points"""
        h = {k: 1e-3 * (best[k] if k.endswith('_rate_multiplier') else 1.0) for k in cov_names}
        pts = {k: np.concatenate([np.full(2, best[k]) + (np.array([h[f], -h[f]]) if f == k else 0.0) for f in cov_names]) for k in cov_names}
        mu = coarse.expected_coarse_points(lf, binning, pts, per_source=per_source)
        return np.stack([(mu[2 * i] - mu[2 * i + 1]) / (2 * h[k]) for i, k in enumerate(cov_names)])

    # the post-fit band of the projection on the first analysis axis
    proj = coarse.CoarseBinning(lf, keep=[x], rebin={x: max(nb // 10, 1)})
    t0 = time.perf_counter()
    mu, sigma, impacts = coarse.sourcewise_coarse_band(lf, proj, cov_names, cov, **best)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    sigma_fd, _ = coarse.propagate_covariance(cov_names, differences(proj, False), cov_names, cov)
    dt_fd = time.perf_counter() - t0
    n = coarse.coarse_counts(lf, proj)[0]
    print('post-fit band of the projection on %s (%d cells): one device call, %.4f s; from central differences (%d points), %.4f s'
          % (x, proj.n_cells, dt, 2 * len(cov_names), dt_fd))
    print('    %-16s %10s %10s %10s %12s' % (x, 'observed', 'expected', '+- band', 'differences'))
    for c in range(proj.n_cells):
        print('    [%5.2f, %5.2f) %10d %10.2f %10.3f %12.3f' % (proj.edges[0][c], proj.edges[0][c + 1], n[c], mu[c], sigma[c], sigma_fd[c]))
    print('    largest impact per cell: ' + ', '.join(max(impacts, key=lambda k: abs(impacts[k][c])).replace('_rate_multiplier', '')
                                                       for c in range(proj.n_cells)))

    # the impact table of a signal box around the first source, per source: which nuisance moves which component by how much
    q = max(nb // 5, 1)
    box = coarse.CoarseBinning(lf, keep=[], ranges={x: (ex[q], ex[min(2 * q + q // 2 + 1, nb)]), y: (ey[q], ey[min(2 * q + q // 2 + 1, nb)])})
    t0 = time.perf_counter()
    all_names, mu_s, J_s = coarse.sourcewise_coarse_jacobian(lf, box, per_source=True, **best)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    J_fd = differences(box, True)                                                 # [F, S]
    dt_fd = time.perf_counter() - t0
    order = [all_names.index(k) for k in cov_names]
    std = np.sqrt(np.diag(cov))
    table = J_s[:, order] * std[None, :]                                          # [S, F]: the shift of source s when the parameter moves by its sigma
    print('impact table of the box %s in [%.2f, %.2f), %s in [%.2f, %.2f): one device call, %.4f s; from central differences, %.4f s'
          % (x, box.groups[0][0] / nb, box.groups[0][1] / nb, y, box.groups[1][0] / nb, box.groups[1][1] / nb, dt, dt_fd))
    print('    expected in the box: ' + ', '.join('s%d %.2f' % (s, mu_s[s]) for s in range(4)) + '; total %.2f, observed %d'
          % (mu_s.sum(), coarse.coarse_counts(lf, box)[0]))
    print('    %-10s %8s ' % ('parameter', 'sigma') + ' '.join('%9s' % ('d s%d' % s) for s in range(4)) + ' %9s %12s' % ('d total', 'differences'))
    for i, k in enumerate(cov_names):
        print('    %-10s %8.4f ' % (k.replace('_rate_multiplier', ''), std[i]) + ' '.join('%9.3f' % table[s, i] for s in range(4))
              + ' %9.3f %12.3f' % (table[:, i].sum(), J_fd[i].sum() * std[i]))
    _, sigma_box, _ = coarse.sourcewise_coarse_band(lf, box, cov_names, cov, **best)
    print('    post-fit uncertainty of the total in the box (with the correlations): +- %.3f' % float(sigma_box))


def measure_asimov():
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, B, P = 5, args.measure_bins ** 3, 64
    Bp = (B + 511) // 512 * 512
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = 2.5e6 * (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])          # ~10 events per bin in all
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    z = rng.uniform(-1.9, 1.9, (P, d))
    r = rng.uniform(0.8, 1.2, (P, S))
    mid = n_a // 2
    counts = rng.poisson(sum(mus[s, mid] * rows[s, mid] for s in range(S))).astype(float)
    fac.set_counts(counts)                        # the same rows in both stores
    fac.set_real_counts(counts)
    print('source-wise model: %d rows, %.2f GB resident (it stays in the 256 MB Infinity Cache: every figure below is cache-assisted)'
          % (S * n_a, S * n_a * Bp * 8 / 1e9), flush=True)
    half, gz, gs, _ = fac.eval_real(z, r)
    half_gof, _, _ = fac.eval_gof(z, r)
    ll, lz, ls, _ = fac.eval_grad(z, r)
    print('agreement over %d points: max |half-deviance - that of bi_eval_sourcewise_gof| / it %.2g; max |gradient + d ll| %.2g of the largest entry'
          % (P, np.max(np.abs(half - half_gof) / half_gof), max(np.max(np.abs(gz + lz)), np.max(np.abs(gs + ls))) /
             max(np.max(np.abs(lz)), np.max(np.abs(ls)))))
    for n in (P, 1):
        zn, rn = z[:n], r[:n]
        alternate([('bi_eval_sourcewise_real + gradient', lambda: fac.eval_real(zn, rn)),
                   ('bi_eval_factored + gradient', lambda: fac.eval_grad(zn, rn)),
                   ('bi_eval_sourcewise_real, values', lambda: fac.eval_real(zn, rn, gradient=False)),
                   ('bi_eval_factored, values', lambda: fac.eval(zn, rn)),
                   ('bi_eval_sourcewise_gof', lambda: fac.eval_gof(zn, rn))], n)
    # the kernels alone, from device events around the launches, in a pass of their own
    dev = fac._dev
    gb = (2 * S + 1) * Bp * 8 * P / 1e9
    for name, call in (('k_sourcewise_real, gradient', lambda: fac.eval_real(z, r)), ('k_morph_factored, gradient', lambda: fac.eval_grad(z, r)),
                       ('k_sourcewise_real, values', lambda: fac.eval_real(z, r, gradient=False)), ('k_morph_factored, values', lambda: fac.eval(z, r)),
                       ('k_sourcewise_gof', lambda: fac.eval_gof(z, r))):
        dev.profile(True)
        ks = []
        for _ in range(args.rounds):
            call()
            ks.append(dev.profile_read()[1] * 1e-3)
        dev.profile(False)
        print('%-28s kernels %s per call of %d points; %.2f GB read -> %.2f TB/s' % (name, quartiles(ks), P, gb, gb / np.median(ks) / 1e3), flush=True)
    print('(bytes: every kernel reads 2 S rows and the counts per point)')
    print('not measured: the other kernel classes (more sources, more own axes, the one-bin-in-flight classes), shapes beyond the '
          'Infinity Cache, several real-valued datasets per call')
    fac.close()


def asimov_band():
    from scipy import stats
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood, inference
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins))
    lf = SourceWiseBinnedLogLikelihood(conf)
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    target, sigmas = 's0_rate_multiplier', (-1, 0, 1, 2)
    t0 = time.perf_counter()
    limits = inference.expected_upper_limit(lf, target, 3.0, confidence_level=0.9, n_sigma=sigmas)
    dt_asimov = time.perf_counter() - t0
    print('expected 90 %% upper limit on %s, background only, %d x %d bins, 11 nuisances profiled' % (target, args.bins, args.bins))
    print('    Asimov dataset (expected_upper_limit, no data): ' + ', '.join('%+d sigma %.4f' % (n, limits[n]) for n in sigmas)
          + '   %.3f s' % dt_asimov, flush=True)
    # the same band from toys: background-only toys, each profiled at a ladder of hypotheses, its limit where t crosses the threshold
    N, hyps = args.toys, np.linspace(0.0, 1.6 * limits[2], 14)[1:]
    t0 = time.perf_counter()
    lf.simulate_toys_points({target: np.array([0.0])}, [N], seed=4)
    best, ll_free = lf.bestfit_batched(datasets=np.arange(N))
    _, ll_cond = lf.bestfit_batched(points={target: np.repeat(hyps, N)}, datasets=np.tile(np.arange(N), len(hyps)))
    t = 2.0 * (ll_free[None, :] - ll_cond.reshape(len(hyps), N))
    t[best[target][None, :] >= hyps[:, None]] = 0.0                 # one-sided: no exclusion below the best fit

    def band_of(crit):
        """every toy's limit: where its t first crosses crit [H] along the ladder -> the band's quantiles, toys without a crossing"""
        per_toy = np.full(N, np.inf)
        for j in range(N):
            above = np.flatnonzero(t[:, j] >= crit)
            if len(above) and above[0] > 0:
                i = above[0]
                lo, hi = t[i - 1, j] - crit[i - 1], t[i, j] - crit[i]
                per_toy[j] = hyps[i - 1] - lo * (hyps[i] - hyps[i - 1]) / (hi - lo)
            elif len(above):
                per_toy[j] = hyps[0]
        return np.quantile(per_toy, stats.norm.cdf(sigmas)), int(np.sum(~np.isfinite(per_toy)))

    wilks, beyond = band_of(np.full(len(hyps), stats.norm.ppf(0.9) ** 2))
    dt_toys = time.perf_counter() - t0
    print('    %d toys x %d hypotheses in lock-step, Wilks\' threshold:  ' % (N, len(hyps)) + ', '.join('%+d sigma %.4f' % (n, v) for n, v in zip(sigmas, wilks))
          + '   %.3f s   (%d toys with a limit beyond the ladder)' % (dt_toys, beyond), flush=True)
    # ... and with the threshold itself from toys at every hypothesis of the ladder (neyman_thresholds): no asymptotics left
    n_per = max(N // 5, 20)
    t0 = time.perf_counter()
    table = lf.neyman_thresholds(target, hyps, n_per, kind='upper', seed=2)
    neyman, beyond = band_of(table.critical_values(0.9))
    dt_neyman = time.perf_counter() - t0
    print('    ... thresholds from %d toys at each hypothesis (neyman_thresholds): ' % n_per + ', '.join('%+d sigma %.4f' % (n, v) for n, v in zip(sigmas, neyman))
          + '   + %.3f s   (%d beyond the ladder)' % (dt_neyman, beyond))
    print('    median expected limit: Asimov %.4f in %.3f s; toys %.4f (Wilks) in %.3f s, %.4f (toy-calibrated) in %.3f s'
          % (limits[0], dt_asimov, wilks[1], dt_toys, neyman[1], dt_toys + dt_neyman))


def measure_sampler():
    """The ensemble sampler at the measured source-wise shape, on the C ABI: bi_sample_stretch_sourcewise (propose, device planner,
    evaluation, accept queued on one stream) against the host engine of blueice_amd.sampler -- the same stretch move in NumPy with
    one bi_eval_factored call per half-step, which is what sample_posterior(engine='host') runs and what the code before the device
    planner ran -- alternated calls, medians with quartiles; then bi_eval_sourcewise_planned against bi_eval_factored values-only.
    Written to profiles/sourcewise_sampler_measure.txt as well."""
    import os
    from blueice_amd import sampler
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, B, steps = 5, args.measure_bins ** 3, 50
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = 2.5e6 * (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])          # ~10 events per bin in all
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    mid = n_a // 2
    fac.set_counts(rng.poisson(sum(mus[s, mid] * rows[s, mid] for s in range(S))).astype(float))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say('# examples/many_nuisances.py --measure-sampler --measure-bins %d --rounds %d on %s' % (args.measure_bins, args.rounds, fac.info()['arch']))
    say('# d = %d, S = %d, one own axis per source (class <4, 1>), %d anchors, %d bins, dense data; every other class: not measured' % (d, S, n_a, B))
    kind = np.array([1] * S + [0] * d, dtype=np.int32)
    index = np.array(list(range(S)) + list(range(d)), dtype=np.int32)
    names = ['r%d' % s for s in range(S)] + ['z%d' % i for i in range(d)]
    lo, hi = np.array([0.] * S + [-2.] * d), np.array([np.inf] * S + [2.] * d)
    z0, one = np.zeros(d), np.ones(S)

    class HostLikelihood:
        """what _host_engine asks of a likelihood: eval_points over the variables' columns, through bi_eval_factored"""
        def eval_points(self, call, livetime_days=None):
            return fac.eval(np.stack([call[n] for n in names[S:]], axis=1), np.stack([call[n] for n in names[:S]], axis=1))[0]

    for W in (40, 1024):
        x0 = np.concatenate([rng.uniform(0.999, 1.001, (W, S)), rng.uniform(-0.01, 0.01, (W, d))], axis=1)[None]
        native = lambda: fac.sample_stretch(W, kind, index, z0, one, one, None, x0, lo, hi, steps, seed=7)
        host = lambda: sampler._host_engine(HostLikelihood(), names, {}, None, None, x0.copy(), lo, hi, steps, 2.0, 7, 0)
        a, b = native(), host()
        same = np.mean(a[0] == b[0])
        say('W = %4d, %d steps: counters of the device loop %s (half-steps, evaluations, accepted, launches, stream waits in the loop); '
            'accepted on the host %d; %.1f %% of the chain entries equal bit for bit' % (W, steps, [int(v) for v in a[3]], b[3][2], 100 * same))
        times = {'native': [], 'host': []}
        for rnd in range(2 + args.rounds):
            for name, call in (('native', native), ('host', host)):
                t0 = time.perf_counter()
                call()
                if rnd >= 2:
                    times[name].append(time.perf_counter() - t0)
        for name, what in (('native', 'bi_sample_stretch_sourcewise'), ('host', 'host engine, bi_eval_factored per half-step')):
            say('W = %4d, %d steps, %-46s %s per call, %.1f us per half-step' % (W, steps, what, quartiles(times[name]),
                                                                                np.median(times[name]) * 1e6 / (2 * steps)))
    for P in (1, 64, 4096):
        z, r = rng.uniform(-1.9, 1.9, (P, d)), rng.uniform(0.8, 1.2, (P, S))
        assert np.array_equal(fac.eval_planned(z, r)[0], fac.eval(z, r)[0])
        times = {'planned': [], 'host': []}
        for rnd in range(3 + args.rounds):
            for name, call in (('planned', lambda: fac.eval_planned(z, r)), ('host', lambda: fac.eval(z, r))):
                t0 = time.perf_counter()
                call()
                if rnd >= 3:
                    times[name].append(time.perf_counter() - t0)
        say('%4d points per call, bi_eval_sourcewise_planned  %s' % (P, quartiles(times['planned'])))
        say('%4d points per call, bi_eval_factored, values    %s' % (P, quartiles(times['host'])))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_sampler_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    fac.close()


def measure_nonempty():
    """The non-empty-bin form of the data (bi_sourcewise_build_nonempty) against the dense store on the same context, toggled with
    the parameter sourcewise_form, at the measured source-wise shape and Poisson data of about 10^3, 10^4, 10^5 and 2.5 10^5 events
    in its 10^6 bins (the last at the quarter rule of nonempty_bins='auto'): bi_eval_factored values-only and with the gradient
    at 1, 64 and 4096 points per call, the kernels alone by device events, the build for one dataset and for 256 toys, and
    bi_sample_stretch_sourcewise at 40 and 1024 walkers.  Alternated calls, medians with quartiles.  Written to
    profiles/sourcewise_nonempty_measure.txt as well."""
    import os
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, B, steps = 5, args.measure_bins ** 3, 50
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])                   # relative rates; the scale is per dataset
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    mid = n_a // 2
    shape = sum(mus[s, mid] * rows[s, mid] for s in range(S))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def form(v):
        fac.set_param('sourcewise_form', v)

    def alternated(pairs, rounds):
        """pairs: (name, form, call); the form is set outside the timed region -> {name: times}"""
        times = {name: [] for name, _, _ in pairs}
        for rnd in range(3 + rounds):
            for name, v, call in pairs:
                form(v)
                t0 = time.perf_counter()
                call()
                if rnd >= 3:
                    times[name].append(time.perf_counter() - t0)
        form(1)
        return times

    say('# examples/many_nuisances.py --measure-nonempty --measure-bins %d --rounds %d on %s' % (args.measure_bins, args.rounds, fac.info()['arch']))
    say('# d = %d, S = %d, one own axis per source (class <4, 1>), %d anchors, %d bins; every other class: not measured' % (d, S, n_a, B))
    for events in (1e3, 1e4, 1e5, 2.5e5):
        scale = events / shape.sum()
        counts = rng.poisson(scale * shape).astype(float)
        rs_scale = scale                                      # the rate scales carry the dataset's normalisation
        fac.set_counts(counts)
        t_build = []
        for _ in range(5):
            t0 = time.perf_counter()
            nnz = fac.build_nonempty()
            t_build.append(time.perf_counter() - t0)
        say('%.1e events: %d listed bins of %d (%.1f %%), compacted copies %.2f MB, bi_sourcewise_build_nonempty (T = 1) %s'
            % (events, int(nnz[0]), B, 100.0 * nnz[0] / B, fac.get_param('sourcewise_nonempty_bytes') / 1e6, quartiles(t_build)))
        for P in (1, 64, 4096):
            z, r = rng.uniform(-1.9, 1.9, (P, d)), rs_scale * rng.uniform(0.8, 1.2, (P, S))
            form(1)
            a = fac.eval_grad(z, r)
            form(0)
            b = fac.eval_grad(z, r)
            rel = np.max(np.abs(a[0] - b[0]) / np.abs(b[0]))
            rounds = args.rounds if P < 4096 else max(5, args.rounds // 4)
            t = alternated([('listed, values', 1, lambda: fac.eval(z, r)), ('dense, values', 0, lambda: fac.eval(z, r)),
                            ('listed, gradient', 1, lambda: fac.eval_grad(z, r)), ('dense, gradient', 0, lambda: fac.eval_grad(z, r))], rounds)
            for what in ('values', 'gradient'):
                lt, dt = t['listed, ' + what], t['dense, ' + what]
                say('%.1e events, %4d points per call, bi_eval_factored %-8s non-empty %s   dense %s   ratio %.2f   (max |ll difference| / |ll| %.1e)'
                    % (events, P, what, quartiles(lt), quartiles(dt), np.median(dt) / np.median(lt), rel))
        # the kernels alone at 64 points, from device events around the launches
        z, r = rng.uniform(-1.9, 1.9, (64, d)), rs_scale * rng.uniform(0.8, 1.2, (64, S))
        for name, v in (('k_sourcewise_nonempty', 1), ('k_morph_factored', 0)):
            form(v)
            fac._dev.profile(True)
            ks = []
            for _ in range(args.rounds):
                fac.eval_grad(z, r)
                ks.append(fac._dev.profile_read()[1] * 1e-3)
            fac._dev.profile(False)
            say('%.1e events, 64 points, with gradient, kernels alone (%s + k_finish): %s' % (events, name, quartiles(ks)))
        form(1)
        if events == 1e4:
            kind = np.array([1] * S + [0] * d, dtype=np.int32)
            index = np.array(list(range(S)) + list(range(d)), dtype=np.int32)
            lo, hi = np.array([0.] * S + [-2.] * d), np.array([np.inf] * S + [2.] * d)
            z0, one = np.zeros(d), np.ones(S)
            for W in (40, 1024):
                x0 = np.concatenate([rs_scale * rng.uniform(0.98, 1.02, (W, S)), rng.uniform(-0.1, 0.1, (W, d))], axis=1)[None]
                call = lambda: fac.sample_stretch(W, kind, index, z0, one, one, None, x0, lo, hi, steps, seed=7)
                t = alternated([('listed', 1, call), ('dense', 0, call)], max(3, args.rounds // 4))
                say('%.1e events, bi_sample_stretch_sourcewise W = %4d, %d steps: non-empty %s   dense %s   ratio %.2f'
                    % (events, W, steps, quartiles(t['listed']), quartiles(t['dense']), np.median(t['dense']) / np.median(t['listed'])))
            # 256 toys of this size: the build for all of them
            fac.generate_toys_points(np.zeros((1, d)), np.full((1, S), rs_scale), 256, seed=3)
            t_build = []
            for _ in range(3):
                t0 = time.perf_counter()
                nnz = fac.build_nonempty()
                t_build.append(time.perf_counter() - t0)
            say('%.1e events, 256 toys: %d listed bins in all, compacted copies %.1f MB, bi_sourcewise_build_nonempty (T = 256) %s'
                % (events, int(nnz.sum()), fac.get_param('sourcewise_nonempty_bytes') / 1e6, quartiles(t_build)))
            P = 256
            z, r = rng.uniform(-0.5, 0.5, (P, d)), rs_scale * rng.uniform(0.9, 1.1, (P, S))
            ds = np.arange(P)
            t = alternated([('listed', 1, lambda: fac.eval_grad(z, r, ds)), ('dense', 0, lambda: fac.eval_grad(z, r, ds))], max(5, args.rounds // 4))
            say('%.1e events, 256 toys, one point per toy with gradient (an iteration of a lock-step fit): non-empty %s   dense %s   ratio %.2f'
                % (events, quartiles(t['listed']), quartiles(t['dense']), np.median(t['dense']) / np.median(t['listed'])))
    say('# not measured: inference.toy_mc_fits through the likelihood class, every class but <4, 1>, other shapes')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_nonempty_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    fac.close()


def posterior():
    """A chain over all twelve parameters with their constraints on the device; the credible upper limit on the signal's
    multiplier beside one_parameter_interval's; the posterior band of the projection on the first analysis axis."""
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood, coarse, sampler
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins))
    lf = SourceWiseBinnedLogLikelihood(conf)
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(3)
    lf.set_data(lf.base_model.simulate())
    _, floating, _, _ = lf.make_objective(minus=False)
    rng = np.random.default_rng(1)
    W, steps, burn = 48, 1500, 500
    p0 = np.array([rng.uniform(0.95, 1.05, W) if n.endswith('_rate_multiplier') else rng.uniform(-0.2, 0.2, W) for n in floating]).T
    t0 = time.perf_counter()
    run = sampler.sample_posterior(lf, n_walkers=W, n_steps=steps, seed=4, p0=p0)
    dt = time.perf_counter() - t0
    kept = run.flat(discard=burn)
    print('posterior over %d parameters: %d walkers x %d steps on the %s engine in %.3f s (%d launches, %d stream waits in the loop), '
          'acceptance %.3f' % (len(run.names), W, steps, run.engine, dt, run.counters[3], run.counters[4] if len(run.counters) > 4 else -1,
                               run.acceptance_fraction.mean()))
    s0 = kept[:, run.names.index('s0_rate_multiplier')]
    limit = lf.one_parameter_interval('s0_rate_multiplier', 3.0, confidence_level=0.9, kind='upper')
    print('    90 %% upper limit on s0_rate_multiplier: credible (posterior quantile, flat prior on the multiplier) %.4f; '
          'one_parameter_interval (profile likelihood, Wilks) %.4f' % (np.quantile(s0, 0.9), limit))
    (x, _), _ = lf.base_model.config['analysis_space']
    proj = coarse.CoarseBinning(lf, keep=[str(x)], rebin={str(x): max(args.bins // 10, 1)})
    draws = kept[rng.choice(len(kept), 512, replace=False)]
    mu = coarse.expected_coarse_points(lf, proj, {n: draws[:, v] for v, n in enumerate(run.names)})
    q16, q50, q84 = np.quantile(mu.reshape(len(draws), -1), [0.1587, 0.5, 0.8413], axis=0)
    print('    posterior band of the projection on %s from 512 draws (one expected_coarse_points call): cell, median, -1 sigma, +1 sigma' % x)
    for c in range(len(q50)):
        print('      %2d  %10.2f  %+8.2f  %+8.2f' % (c, q50[c], q16[c] - q50[c], q84[c] - q50[c]))


def measure_grid():
    """The gridded likelihood of a source-wise model at the measured shape with Poisson data of 10^4 events, on the context:
    bi_grid_reduce_sourcewise on route 1 (the matrix-core scan route) and route 0 (one work item per point) against the host engine
    (blueice_amd.grid._host_engine over a likelihood whose eval_points is bi_eval_factored, reduced by reduce_cells) on the same
    grid; bi_eval_sourcewise_scan against bi_eval_factored values-only at 4096 and 10^6 points of one cell tuple; the planner's
    share of a call from device events.  Alternated calls, medians with quartiles.  Written to
    profiles/sourcewise_scan_measure.txt as well."""
    import os
    from blueice_amd import grid
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, B = 5, args.measure_bins ** 3
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05
    rows /= rows.sum(axis=-1, keepdims=True)
    mus = (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    mid = n_a // 2
    shape = sum(mus[s, mid] * rows[s, mid] for s in range(S))
    scale = 1e4 / shape.sum()
    fac.set_counts(rng.poisson(scale * shape).astype(float))
    nnz = fac.build_nonempty()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def alternated(calls, rounds):
        times = {name: [] for name, _ in calls}
        for rnd in range(2 + rounds):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                if rnd >= 2:
                    times[name].append(time.perf_counter() - t0)
        return times

    say('# examples/many_nuisances.py --measure-grid --measure-bins %d --rounds %d on %s' % (args.measure_bins, args.rounds, fac.info()['arch']))
    say('# d = %d, S = %d, one own axis per source (class <4, 1>: 8 rows per point), %d anchors, %d bins, %d listed bins (10^4 events); '
        'every other class: not measured' % (d, S, n_a, B, int(nnz[0])))
    # the grid: the multiplier of source 0 kept, two shape parameters and the multiplier of source 1 reduced
    names = ['r0', 'z0', 'z1', 'r1']
    kind, index = np.array([1, 0, 0, 1], dtype=np.int32), np.array([0, 0, 1, 1], dtype=np.int32)
    nodes = [np.linspace(0.5, 1.5, 33), np.linspace(-1.9, 1.9, 65), np.linspace(-1.9, 1.9, 65), np.linspace(0.8, 1.2, 7)]
    z0, scale0, unit = np.zeros((1, d)), np.full((1, S), scale), np.full((1, S), scale)
    G = int(np.prod([len(v) for v in nodes]))
    logw = [np.zeros(len(nodes[0]))] + [np.log(grid.trapezoid_weights(v)) for v in nodes[1:]]

    class HostLikelihood:
        """what _host_engine asks of a likelihood: eval_points over the axes' columns, through bi_eval_factored"""
        def eval_points(self, call, livetime_days=None):
            P = len(call['r0'])
            z, r = np.zeros((P, d)), np.full((P, S), scale)
            z[:, 0], z[:, 1], r[:, 0], r[:, 1] = call['z0'], call['z1'], scale * call['r0'], scale * call['r1']
            return fac.eval(z, r)[0]

    axes = list(zip(names, nodes))
    run = {route: (lambda route=route: fac.grid_reduce(kind, index, z0, scale0, unit, None, 1, nodes, logw=logw, route=route)) for route in (1, 0)}
    host = lambda: grid._host_engine(HostLikelihood(), axes, 1, logw[1:], None, None, None, {})
    a, b, h = run[1](), run[0](), host()
    say('grid of 33 x 65 x 65 x 7 = %d points, 16 cell tuples: route scan %d chunk(s), %d launches; route points %d launches'
        % (G, a[3][0], a[3][3], b[3][3]))
    say('    max |log_marginal difference|: scan - points %.2e, scan - host %.2e; argmax equal: %s, %s'
        % (np.max(np.abs(a[0] - b[0])), np.max(np.abs(a[0].ravel() - h[0])), np.array_equal(a[2], b[2]), np.array_equal(a[2].ravel(), h[2])))
    rounds = max(5, args.rounds // 4)
    t = alternated([('scan', run[1]), ('points', run[0])], rounds)
    th = alternated([('host', host)], 3)
    for name, tt in (('route scan  ', t['scan']), ('route points', t['points']), ('engine host ', th['host'])):
        say('    bi_grid_reduce_sourcewise %s %s   %.2f M points/s' % (name, quartiles(tt), G / np.median(tt) / 1e6))
    say('    ratio points / scan %.2f, host / scan %.2f' % (np.median(t['points']) / np.median(t['scan']), np.median(th['host']) / np.median(t['scan'])))
    # one cell tuple: bi_eval_sourcewise_scan against bi_eval_factored values-only
    for P in (4096, 10 ** 6):
        z, r = rng.uniform(0.05, 0.95, (P, d)), scale * rng.uniform(0.8, 1.2, (P, S))
        ll_s, ll_e = fac.eval_scan(z, r)[0], fac.eval(z, r)[0]
        c = fac.last_scan_counters
        rounds = args.rounds if P == 4096 else 5
        t = alternated([('scan', lambda: fac.eval_scan(z, r)), ('factored', lambda: fac.eval(z, r))], rounds)
        say('%7d points of one cell tuple (%d groups, %d items, nslots %d): bi_eval_sourcewise_scan %s   bi_eval_factored values-only %s   '
            'ratio %.2f   (max |ll difference| / |ll| %.1e)' % (P, c[0], c[1], fac.get_param('last_scan_nslots'), quartiles(t['scan']),
                                                              quartiles(t['factored']), np.median(t['factored']) / np.median(t['scan']),
                                                              np.max(np.abs(ll_s - ll_e) / np.abs(ll_e))))
        # the planner's share, from device events: everything in front of the matrix-core launch (the host read included), and the launch
        parts = {}
        for what, bits_ in (('planner', 1), ('k_scan_mfma', 2)):
            fac.set_param('sourcewise_scan_timed', bits_)
            fac._dev.profile(True)
            ks = []
            for _ in range(rounds):
                fac.eval_scan(z, r)
                ks.append(fac._dev.profile_read()[1] * 1e-3)
            fac._dev.profile(False)
            parts[what] = ks
        fac.set_param('sourcewise_scan_timed', 3)
        say('%7d points, device events: planner (screen, key, sort, structure, host read, fill) %s   k_scan_mfma %s   planner share %.0f %%'
            % (P, quartiles(parts['planner']), quartiles(parts['k_scan_mfma']),
               100 * np.median(parts['planner']) / (np.median(parts['planner']) + np.median(parts['k_scan_mfma']))))
    say('# not measured: blueice_amd.grid.grid_scan through the likelihood class, every class but <4, 1>, several datasets, other list lengths')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_scan_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    fac.close()


def grid_limit():
    """The 90 % credible upper limit on the signal's multiplier from a gridded likelihood (blueice_amd.grid.grid_scan on the
    source-wise model: bi_grid_reduce_sourcewise), marginalised by the trapezoid rule over the signal's own nuisance parameter and
    two background multipliers with every other parameter at its default, beside the same quantile of a chain over the same four
    parameters (blueice_amd.sampler.sample_posterior with the others fixed)."""
    from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood, grid, sampler
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins))
    lf = SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(nonempty_bins=True))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(3)
    d = lf.base_model.simulate()
    lf.set_data(d[:max(len(d) // 8, 1)])                          # mostly empty bins: the non-empty-bin form's case
    nuisance = own[0][0]                                          # the signal's first own parameter
    keep = [('s0_rate_multiplier', np.linspace(0.0, 1.0, 65))]
    reduce = [(nuisance, np.linspace(-2.0, 2.0, 33)), ('s1_rate_multiplier', np.linspace(0.02, 0.4, 25)),
              ('s2_rate_multiplier', np.linspace(0.02, 0.4, 25))]
    fixed = {n: 0.0 for n in names if n != nuisance}
    fixed['s3_rate_multiplier'] = 0.125
    results = {}
    for route in ('scan', 'points'):
        lf.config['sourcewise_grid_route'] = route
        grid.grid_scan(lf, keep=keep, reduce=reduce, **fixed)    # (warm: allocations)
        t0 = time.perf_counter()
        results[route] = grid.grid_scan(lf, keep=keep, reduce=reduce, **fixed)
        res = results[route]
        print('grid of %d x %d x %d x %d = %d points, route %s on the %s engine: %.3f s (%d chunks, %d launches, %d excluded points)'
              % (len(keep[0][1]), 33, 25, 25, res.counters[1], route, res.engine, time.perf_counter() - t0, res.counters[0], res.counters[3],
                 res.excluded))
    limits = {r: v.credible_upper_limit(0.9) for r, v in results.items()}
    rng = np.random.default_rng(1)
    W, steps, burn = 32, 2000, 500
    best = results['scan']
    k = int(np.argmax(best.profile))
    at = dict([('s0_rate_multiplier', keep[0][1][k])] + [(n, float(best.best[n][k])) for n, _ in reduce])
    order = ['s0_rate_multiplier', 's1_rate_multiplier', 's2_rate_multiplier', nuisance]      # rate multipliers first, then shape parameters
    p0 = np.array([at[n] for n in order])[None, :] + 0.01 * rng.standard_normal((W, 4))
    p0[:, :3] = np.abs(p0[:, :3])
    t0 = time.perf_counter()
    run = sampler.sample_posterior(lf, n_walkers=W, n_steps=steps, seed=4, p0=p0, **fixed)
    assert run.names == order, run.names
    kept = run.flat(discard=burn)
    s0 = kept[:, run.names.index('s0_rate_multiplier')]
    inside = np.mean(s0 <= keep[0][1][-1])
    print('chain over the same %d parameters: %d walkers x %d steps on the %s engine in %.3f s, acceptance %.3f'
          % (len(run.names), W, steps, run.engine, time.perf_counter() - t0, run.acceptance_fraction.mean()))
    print('90 % credible upper limit on s0_rate_multiplier (flat priors on the multipliers, the nuisance parameter\'s Gaussian constraint):')
    print('    gridded likelihood, route scan    %.4f' % limits['scan'])
    print('    gridded likelihood, route points  %.4f' % limits['points'])
    print('    chain (posterior quantile)        %.4f   (%.1f %% of the chain inside the grid\'s range of the multiplier)'
          % (np.quantile(s0, 0.9), 100 * inside))


def unbinned():
    """Eight nuisances of five anchors and four rate multipliers fitted over events, and one profile scan of the signal's multiplier"""
    from blueice_amd import GaussianPrior, SourceWiseUnbinnedLogLikelihood
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins), source_class=NuisanceHistogramSource)
    lf = SourceWiseUnbinnedLogLikelihood(conf)
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    t0 = time.perf_counter()
    lf.prepare()
    rows = sum(5 ** len(o) for o in own)
    print('(1) prepare(): %d shape parameters x 5 anchors, 4 histogram sources responding to %s: %d density histograms on the device, %.2f s'
          % (len(names), ', '.join('/'.join(o) for o in own), rows, time.perf_counter() - t0))
    np.random.seed(3)
    data = lf.base_model.simulate()
    t0 = time.perf_counter()
    lf.set_data(data)
    print('    set_data(): %d events scored on the %s at %d rows: an event store of %.2f MB (the full grid would hold 5^%d x 4 rows: %.1e MB)'
          % (len(data), lf.last_scoring_route, rows, lf.ctx.get_param('sourcewise_events_bytes') / 1e6, len(names),
             5.0 ** len(names) * 4 * len(data) * 8 / 1e6))
    t0 = time.perf_counter()
    best, ll, info = lf.bestfit_batched(return_info=True)
    print('(2) bestfit_batched over events, %d parameters floating: max ll %.4f, converged %s, %d evaluations in %d device calls, %.3f s'
          % (len(best), ll[0], bool(info['converged'][0]), info['evaluations'], info['calls'], time.perf_counter() - t0))
    print('    ' + ', '.join('%s %.3f' % (k.replace('_rate_multiplier', ''), v[0]) for k, v in best.items()))
    grid = np.linspace(0.7, 1.3, args.scan)
    t0 = time.perf_counter()
    scan = lf.likelihood_ratio_scan(('s0_rate_multiplier', grid))
    dt = time.perf_counter() - t0
    inside = grid[2 * scan <= 1.0]
    print('(3) likelihood_ratio_scan over s0_rate_multiplier: %d hypotheses, 11 nuisances profiled at each, %.3f s; minimum at %.3f, '
          '2 dlnL <= 1 on [%.3f, %.3f]' % (args.scan, dt, grid[np.argmin(scan)], inside.min(), inside.max()))
    # the errors of all twelve parameters from both routes: the analytic Hessian over the event store, and differences of the gradient
    errors, seconds = {}, {}
    for route, analytic in (('analytic', True), ('gradient-differences', False)):
        lf.config['analytic_hessian'] = analytic
        t0 = time.perf_counter()
        fit, ll_fit = lf.bestfit_minuit()
        seconds[route] = time.perf_counter() - t0
        assert lf.hessian_method == route
        errors[route] = fit
    print('(4) bestfit_minuit: max ll %.4f; parabolic errors from the analytic Hessian (bi_eval_sourcewise_events_hess, %.3f s with the fit) and '
          'from differences of the gradient (%d displaced points, %.3f s with the fit)' % (ll_fit, seconds['analytic'], 2 * len(best) + 1,
                                                                                           seconds['gradient-differences']))
    print('    %-10s %10s %12s %12s' % ('parameter', 'value', 'analytic', 'differences'))
    for k in best:
        print('    %-10s %10.4f %12.5f %12.5f' % (k.replace('_rate_multiplier', ''), errors['analytic'][k], errors['analytic'][k + '_error'],
                                                  errors['gradient-differences'][k + '_error']))
    lf.ctx.close()


def measure_unbinned_hessian():
    """bi_eval_sourcewise_events_hess against what it replaces -- ONE bi_eval_factored gradient call over the (2 F + 1) P points of
    central differences, as the class takes them -- and against bi_eval_hess on the same model expanded to the 5^4 unbinned grid
    model, at 10^6 and 10^4 events, 64 points and one point per call.  Alternated calls, medians with quartiles, device events for
    the kernels alone.  Written to profiles/sourcewise_events_curv_measure.txt as well."""
    import os
    from blueice_amd.device import DeviceContext
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    F = d + S
    n_a, nb = 5, args.measure_bins
    B = nb ** 3
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05                                         # densities over the unit cube
    rows *= B / rows.sum(axis=-1, keepdims=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fac = SourceWiseContext(0)
    say('# examples/many_nuisances.py --measure-unbinned-hessian --measure-bins %d --rounds %d on %s' % (nb, args.rounds, fac.info()['arch']))
    say('# d = %d, S = %d, one own axis per source (class <4, 1>: 8 basis columns, one launch), %d anchors, density histograms of %d^3 bins, '
        '\'linear\' lookup, F = %d' % (d, S, n_a, nb, F))
    edges = [np.linspace(0., 1., nb + 1)] * 3
    centres = [0.5 * (e[:-1] + e[1:]) for e in edges]
    mus = (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])                   # relative rates (10 in all); the scale is per dataset
    tp = DeviceContext(0)
    tp.begin_model([g] * d, S, B)
    for lin, idx in enumerate(np.ndindex(*(n_a,) * d)):          # the same likelihood on the product grid: source s from ITS anchor
        tp.set_anchor(lin, np.stack([rows[s, idx[s]] for s in range(S)]), np.array([mus[s, idx[s]] for s in range(S)]))
    tp.end_model()
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    for events in (1e6, 1e4):
        N = int(events)
        coords = [np.clip(rng.random(N), c[0], c[-1]) for c in centres]
        full = DeviceContext(0)
        fac.score_events('linear', centres, [coords], 1e-12)
        tp.score_events(full, 'linear', centres, coords, 1e-12)
        for P in (64, 1):
            z = rng.uniform(0.1, 0.9, (P, d)) + rng.integers(-2, 2, (P, d))      # strictly inside cells: the differences stay in them
            r = events / 10.0 * rng.uniform(0.8, 1.2, (P, S))
            zz, rr = np.tile(z, (2 * F + 1, 1)), np.tile(r, (2 * F + 1, 1))
            for j in range(F):
                for k, sign in enumerate((1.0, -1.0)):
                    at = slice((1 + 2 * j + k) * P, (2 + 2 * j + k) * P)
                    if j < d:
                        zz[at, j] += sign * 1e-4
                    else:
                        rr[at, j - d] *= 1.0 + sign * 1e-5
            a, b = fac.eval_events_hess(z, r), full.eval_hess(z, r)
            g1 = fac.eval_grad(z, r)
            same = np.array_equal(a[0], g1[0]) and np.array_equal(a[1], g1[1]) and np.array_equal(a[2], g1[2])
            rel = np.max(np.abs(a[3] - b[3])) / np.max(np.abs(b[3]))
            calls = [('hess', lambda: fac.eval_events_hess(z, r)), ('diff', lambda: fac.eval_grad(zz, rr)), ('grid', lambda: full.eval_hess(z, r)),
                     ('grad', lambda: fac.eval_grad(z, r))]
            times = {name: [] for name, _ in calls}
            for rnd in range(3 + args.rounds):          # three warm-up rounds; the calls alternate inside every round
                for name, call in calls:
                    t0 = time.perf_counter()
                    call()
                    if rnd >= 3:
                        times[name].append(time.perf_counter() - t0)
            say('%.0e events, %2d points per call: bi_eval_sourcewise_events_hess %s   bi_eval_factored + gradient at (2 F + 1) P = %d points %s   '
                'bi_eval_hess on the 5^%d unbinned grid model %s   bi_eval_factored + gradient at the P points %s'
                % (events, P, quartiles(times['hess']), len(zz), quartiles(times['diff']), d, quartiles(times['grid']), quartiles(times['grad'])))
            say('%.0e events, %2d points per call: differences / analytic %.2f, grid model / analytic %.2f, analytic / one gradient call %.2f; ll and '
                'gradient bit for bit bi_eval_factored\'s: %s; max |H - H of the grid model| %.1e of the largest entry'
                % (events, P, np.median(times['diff']) / np.median(times['hess']), np.median(times['grid']) / np.median(times['hess']),
                   np.median(times['hess']) / np.median(times['grad']), same, rel))
            cols = max(512, (N + 511) // 512 * 512)
            for name, ctx, call, n_rows, n_pts in (('k_sourcewise_events_curv + k_finish', fac._dev, calls[0][1], 2 * S, P),
                                                   ('k_sourcewise_events + k_finish, (2 F + 1) P points', fac._dev, calls[1][1], 2 * S, len(zz)),
                                                   ('the grid route\'s kernels', full, calls[2][1], S * 2 ** d, P)):
                ctx.profile(True)
                ks = []
                for _ in range(args.rounds):
                    call()
                    ks.append(ctx.profile_read()[1] * 1e-3)
                ctx.profile(False)
                gb = n_rows * cols * 8 * n_pts / 1e9
                say('%.0e events, %2d points, kernels alone (%s): %s; %d rows x %d columns x 8 bytes x %d points = %.3f GB -> %.2f TB/s'
                    % (events, P, name, quartiles(ks), n_rows, cols, n_pts, gb, gb / np.median(ks) / 1e3))
        full.close()
    say('# cache-assisted: the event store is %.1f MB at 1e4 events (inside an L2) and %.0f MB at 1e6 (inside the 256 MiB Infinity Cache), and the '
        'points of a call read the same rows again; the grid model\'s tensor is %.0f MB and %.0f GB' % (S * n_a * 10240 * 8 / 1e6, S * n_a * 1e6 * 8 / 1e6,
                                                                                                       n_a ** d * S * 1e4 * 8 / 1e6, n_a ** d * S * 1e6 * 8 / 1e9))
    say('# not measured: every class but <4, 1> (more sources, more own axes), the panelled classes <8, 2> and <8, 3>, T > 1 event sets, other shapes')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_events_curv_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    fac.close()
    tp.close()


def measure_unbinned():
    """bi_eval_factored on the event store against the parent's route -- the same model expanded to the 5^4 unbinned grid model in a
    second context, which reads 64 rows per point where this one reads 8 -- at 10^4 and 10^6 events, 64 points and one point per
    call, with and without the gradient; and bi_sourcewise_score_events against bi_score_events on the expanded templates.
    Alternated calls, medians with quartiles, device events for the kernels alone.  Written to
    profiles/sourcewise_events_measure.txt as well."""
    import os
    from blueice_amd.device import DeviceContext
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, nb = 5, args.measure_bins
    B = nb ** 3
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05                                         # densities over the unit cube
    rows *= B / rows.sum(axis=-1, keepdims=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fac = SourceWiseContext(0)
    say('# examples/many_nuisances.py --measure-unbinned --measure-bins %d --rounds %d on %s' % (nb, args.rounds, fac.info()['arch']))
    say('# d = %d, S = %d, one own axis per source (class <4, 1>), %d anchors, density histograms of %d^3 bins, \'linear\' lookup' % (d, S, n_a, nb))
    edges = [np.linspace(0., 1., nb + 1)] * 3
    centres = [0.5 * (e[:-1] + e[1:]) for e in edges]
    mus = (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])                   # relative rates (10 in all); the scale is per dataset
    tp = DeviceContext(0)
    t0 = time.perf_counter()
    tp.begin_model([g] * d, S, B)
    for lin, idx in enumerate(np.ndindex(*(n_a,) * d)):          # the same likelihood on the product grid: source s from ITS anchor
        tp.set_anchor(lin, np.stack([rows[s, idx[s]] for s in range(S)]), np.array([mus[s, idx[s]] for s in range(S)]))
    tp.end_model()
    say('expanded templates resident: %d anchor models, %.1f GB, %.1f s to stream; source-wise: %d rows, %.2f GB'
        % (n_a ** d, n_a ** d * S * B * 8 / 1e9, time.perf_counter() - t0, S * n_a, S * n_a * B * 8 / 1e9))
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    for events in (1e4, 1e6):
        N = int(events)
        coords = [np.clip(rng.random(N), c[0], c[-1]) for c in centres]
        full = DeviceContext(0)
        t_sw, t_full = [], []
        for rnd in range(1 + args.rounds):                        # one warm-up round; the two calls alternate
            t0 = time.perf_counter()
            fac.score_events('linear', centres, [coords], 1e-12)
            t1 = time.perf_counter()
            tp.score_events(full, 'linear', centres, coords, 1e-12)
            t2 = time.perf_counter()
            if rnd:
                t_sw.append(t1 - t0)
                t_full.append(t2 - t1)
        say('%.0e events: bi_sourcewise_score_events (%d rows, store %.1f MB) %s   bi_score_events on the expanded templates (%d rows, %.1f MB) %s   ratio %.1f'
            % (events, S * n_a, fac.get_param('sourcewise_events_bytes') / 1e6, quartiles(t_sw), n_a ** d * S, n_a ** d * S * N * 8 / 1e6,
               quartiles(t_full), np.median(t_full) / np.median(t_sw)))
        for P in (64, 1):
            z, r = rng.uniform(-1.9, 1.9, (P, d)), events / 10.0 * rng.uniform(0.8, 1.2, (P, S))
            a, b = fac.eval_grad(z, r), full.eval_grad(z, r)
            rel = np.max(np.abs(a[0] - b[0]) / np.abs(b[0]))
            calls = [('store, gradient', lambda: fac.eval_grad(z, r)), ('grid, gradient', lambda: full.eval_grad(z, r)),
                     ('store, values', lambda: fac.eval(z, r)), ('grid, values', lambda: full.eval(z, r))]
            times = {name: [] for name, _ in calls}
            for rnd in range(3 + args.rounds):          # three warm-up rounds; the calls alternate inside every round
                for name, call in calls:
                    t0 = time.perf_counter()
                    call()
                    if rnd >= 3:
                        times[name].append(time.perf_counter() - t0)
            for what, base in (('gradient', 'bi_eval_grad'), ('values', 'bi_eval')):
                st, gt = times['store, ' + what], times['grid, ' + what]
                say('%.0e events, %2d points per call, %-8s bi_eval_factored on the event store %s   %s on the 5^%d unbinned grid model %s   ratio %.2f   '
                    '(max |ll difference| / |ll| %.1e)' % (events, P, what, quartiles(st), base, d, quartiles(gt), np.median(gt) / np.median(st), rel))
            if P == 64:
                cols = max(512, (N + 511) // 512 * 512)
                for name, ctx, call, n_rows in (('k_sourcewise_events + k_finish', fac._dev, calls[0][1], 2 * S),
                                                ('the grid route\'s kernels', full, calls[1][1], S * 2 ** d)):
                    ctx.profile(True)
                    ks = []
                    for _ in range(args.rounds):
                        call()
                        ks.append(ctx.profile_read()[1] * 1e-3)
                    ctx.profile(False)
                    med = np.median(ks)
                    say('%.0e events, 64 points, with gradient, kernels alone (%s): %s; %d rows x %d columns x 8 bytes x 64 points = %.3f GB -> %.2f TB/s'
                        % (events, name, quartiles(ks), n_rows, cols, n_rows * cols * 8 * 64 / 1e9, n_rows * cols * 8 * 64 / med / 1e12))
        full.close()
    say('# cache-assisted: every figure at 1e4 events (the event store is %.1f MB, inside an L2; the grid model\'s tensor is %.0f MB, inside the '
        '256 MiB Infinity Cache; the 64 points of a call read the same rows again).  At 1e6 events the store is %.0f MB -- still inside the '
        'Infinity Cache -- and the grid model\'s tensor %.0f GB, which is not' % (S * n_a * 10240 * 8 / 1e6, n_a ** d * S * 1e4 * 8 / 1e6,
                                                                                 S * n_a * 1e6 * 8 / 1e6, n_a ** d * S * 1e6 * 8 / 1e9))
    say('# not measured: every class but <4, 1>, T > 1 event sets, the fit loop\'s wall time, \'piecewise\' scoring, other shapes')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_events_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    fac.close()
    tp.close()


def unbinned_toys():
    """Twelve nuisances of five anchors (5^12 grid anchors: no grid model) and six rate multipliers over events: a small ensemble of
    event-level toys drawn on the device and fitted, and the toy-calibrated critical value of the signal's upper limit beside Wilks'"""
    from scipy import stats
    from blueice_amd import GaussianPrior, SourceWiseUnbinnedLogLikelihood, inference, sourcewise_event_toys, sourcewise_simulated_events
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins), n_params=12, n_sources=6, own_per_source=2, events_per_day=40.,
                                             source_class=NuisanceHistogramSource)
    lf = SourceWiseUnbinnedLogLikelihood(conf)
    for s in range(6):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    t0 = time.perf_counter()
    lf.prepare()
    print('(1) prepare(): %d shape parameters x 5 anchors, 6 histogram sources of two own parameters: %d density histograms, %.2f s'
          % (len(names), sum(5 ** len(o) for o in own), time.perf_counter() - t0))
    n_toys = max(8, args.toys // 5)
    t0 = time.perf_counter()
    counts = sourcewise_event_toys(lf, n_toys, seed=5, np3=0.5)
    dt = time.perf_counter() - t0
    d0 = sourcewise_simulated_events(lf, 0)
    print('(2) sourcewise_event_toys: %d toys of %.0f events on average drawn and scored on the device in %.4f s (store %.2f MB); toy 0 has %d events, '
          '%s per source' % (n_toys, counts.sum(axis=1).mean(), dt, lf.ctx.get_param('sourcewise_events_bytes') / 1e6, len(d0), counts[0].tolist()))
    t0 = time.perf_counter()
    best, ll = inference.bestfit_toys(lf)
    # (s3 is the one source alone at its centre: s0 and s4, s1 and s5 share theirs and are all but degenerate pairs)
    print('    bestfit_toys: %d parameters floating in each of %d fits, %.3f s; s3_rate_multiplier %.3f +- %.3f over the ensemble (truth 1)'
          % (len(best), n_toys, time.perf_counter() - t0, best['s3_rate_multiplier'].mean(), best['s3_rate_multiplier'].std()))
    hyp = np.array([0.8, 1.0, 1.2])
    t0 = time.perf_counter()
    table = inference.neyman_thresholds(lf, 's3_rate_multiplier', hyp, n_toys, kind='upper', seed=6, chunk=2 * n_toys)
    level = 1 - 1.0 / n_toys if n_toys < 10 else 0.9
    crit = table.critical_values(level)
    print('(3) neyman_thresholds: %d hypotheses x %d toys, two fits per toy, %.3f s' % (len(hyp), n_toys, time.perf_counter() - t0))
    print('    critical value of t at the %.0f %% level (kind upper):  ' % (100 * level)
          + ', '.join('s3 = %.1f: %.3f' % (h, c) for h, c in zip(hyp, crit)) + ';   Wilks: %.3f' % stats.norm.ppf(level) ** 2)
    lf.ctx.close()


def measure_unbinned_toys():
    """bi_sourcewise_simulate_event_toys against the two routes that existed: bi_simulate_event_toys on the same model expanded to the
    5^4 unbinned grid model (2500 rows per event where the source-wise store holds 20), and the host route (draw every toy with NumPy
    from the morphed histograms as HistogramPdfSource.simulate does, then score all sets with bi_sourcewise_score_events, as
    base_model.simulate() + set_datasets do).  256 toys of 10^4 expected events and one toy of 10^6, one truth; alternated calls,
    medians with quartiles, and the device time of the call's four parts from the library's own events.  Written to
    profiles/sourcewise_event_toys_measure.txt as well."""
    import os
    from blueice_amd.device import DeviceContext
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a, nb = 5, args.measure_bins
    B = nb ** 3
    rng = np.random.default_rng(11)
    g = np.linspace(-2., 2., n_a)
    rows = rng.random((S, n_a, B)) + 0.05                                         # densities over the unit cube
    rows *= B / rows.sum(axis=-1, keepdims=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fac = SourceWiseContext(0)
    say('# examples/many_nuisances.py --measure-unbinned-toys --measure-bins %d --rounds %d on %s' % (nb, args.rounds, fac.info()['arch']))
    say('# d = %d, S = %d, one own axis per source (class <4, 1>), %d anchors, density histograms of %d^3 bins, \'linear\' lookup, one truth' % (d, S, n_a, nb))
    edges = [np.linspace(0., 1., nb + 1)] * 3
    centres = [0.5 * (e[:-1] + e[1:]) for e in edges]
    mus = (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])                   # relative rates (10 in all); the scale is per call
    tp = DeviceContext(0)
    tp.begin_model([g] * d, S, B)
    for lin, idx in enumerate(np.ndindex(*(n_a,) * d)):          # the same likelihood on the product grid: source s from ITS anchor
        tp.set_anchor(lin, np.stack([rows[s, idx[s]] for s in range(S)]), np.array([mus[s, idx[s]] for s in range(S)]))
    tp.end_model()
    fac.begin_model([g] * d, S, B, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, rows[s, a], mus[s, a])
    fac.end_model()
    z = np.array([0.3, -1.2, 0.7, 1.6])

    def host_route(T, scale, seed):
        """what base_model.simulate() + set_datasets do, T times: Poisson numbers, bins by the running sums of the morphed pmf,
        uniform positions (NumPy), then one device scoring of all sets"""
        gen = np.random.default_rng(seed)
        k = np.clip(np.searchsorted(g, z, side='right') - 1, 0, n_a - 2)
        t = (z - g[k]) / (g[k + 1] - g[k])
        cdf = [np.cumsum((1 - t[s]) * rows[s, k[s]] + t[s] * rows[s, k[s] + 1]) for s in range(S)]
        rate = [((1 - t[s]) * mus[s, k[s]] + t[s] * mus[s, k[s] + 1]) * scale[s] for s in range(S)]
        sets = []
        for _ in range(T):
            bins = np.concatenate([np.searchsorted(cdf[s], gen.random(gen.poisson(rate[s])) * cdf[s][-1], side='right') for s in range(S)])
            idx = np.unravel_index(np.minimum(bins, B - 1), (nb,) * 3)
            sets.append([np.clip(e[i] + gen.random(len(bins)) * (e[i + 1] - e[i]), c[0], c[-1]) for e, i, c in zip(edges, idx, centres)])
        fac.score_events('linear', centres, sets, 1e-12)

    for T, events in ((256, 1e4), (1, 1e6)):
        scale = np.full(S, events / 10.0)
        full = DeviceContext(0)
        calls = [('device', lambda: fac.simulate_event_toys('linear', edges, z[None], scale[None], [T], 7, 1e-12)),
                 ('grid', lambda: tp.simulate_event_toys(full, 'linear', edges, z, scale, T, 7, 1e-12)),
                 ('host', lambda: host_route(T, scale, 7))]
        n_sw, n_grid = calls[0][1](), calls[1][1]()
        same = np.array_equal(n_sw, n_grid) and np.array_equal(fac.download_events()[0], full.download_events()[0])
        times = {name: [] for name, _ in calls}
        for rnd in range(2 + args.rounds):              # two warm-up rounds; the calls alternate inside every round
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                if rnd >= 2:
                    times[name].append(time.perf_counter() - t0)
        say('%3d toys of %.0e expected events (%d drawn): bi_sourcewise_simulate_event_toys (store: 20 rows, %.1f MB) %s   bi_simulate_event_toys on the '
            '5^%d grid model (2500 rows, %.1f MB) %s   host route (NumPy draws + bi_sourcewise_score_events) %s'
            % (T, events, n_sw.sum(), S * n_a * 8 * np.maximum(512, (n_sw.sum(axis=1) + 511) // 512 * 512).sum() / 1e6, quartiles(times['device']), d,
               n_a ** d * S * 8 * n_sw.sum() / 1e6, quartiles(times['grid']), quartiles(times['host'])))
        say('%3d toys of %.0e: grid model / source-wise %.2f, host route / source-wise %.2f; the events of the two device routes are equal bit for bit: %s'
            % (T, events, np.median(times['grid']) / np.median(times['device']), np.median(times['host']) / np.median(times['device']), same))
        fac._dev.profile(True)
        parts = {k: [] for k in ('layout', 'pmf', 'events', 'score')}
        for _ in range(args.rounds):
            calls[0][1]()
            for k in parts:
                parts[k].append(fac.get_param('sim_ns_' + k) * 1e-9)
            fac._dev.profile_read()
        fac._dev.profile(False)
        say('%3d toys of %.0e, device time of the call\'s parts: counts + layout %s   pmf rows + running sums (k_sourcewise_pmf, %d scans) %s   '
            'event kernel %s   scoring (k_score_locate, k_score_rows, k_fill_columns; with the host\'s gaps between them) %s'
            % (T, events, quartiles(parts['layout']), S, quartiles(parts['pmf']), quartiles(parts['events']), quartiles(parts['score'])))
        full.close()
    say('# cache-assisted: the pmf and cdf rows of the truth (2 x %d x %.0f MB) and the %d rows the scoring gathers from (%.0f MB) stay in the 256 MiB '
        'Infinity Cache between the rounds, as does the store of the 256 toys; the grid model gathers from %.0f GB of templates, which do not'
        % (S, B * 8 / 1e6, S * n_a, S * n_a * B * 8 / 1e6, n_a ** d * S * B * 8 / 1e9))
    say('# not measured: every class but <4, 1>, H > 1 truths (sub-batches), \'piecewise\' scoring, the fits on the toys, other shapes')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_event_toys_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    fac.close()
    tp.close()


def unbinned_posterior():
    """The 90 % credible upper limit on the signal's multiplier of the EVENT model from a gridded likelihood
    (blueice_amd.grid.grid_scan on SourceWiseUnbinnedLogLikelihood: bi_grid_reduce_sourcewise_events, one work item per grid point),
    marginalised over the signal's own nuisance parameter and two background multipliers with every other parameter fixed, beside
    the same quantile of a chain over the same four parameters (blueice_amd.sampler.sample_posterior:
    bi_sample_stretch_sourcewise_events, the proposals planned on the device)."""
    from blueice_amd import GaussianPrior, SourceWiseUnbinnedLogLikelihood, grid, sampler
    from blueice_amd.synthetic import NuisanceHistogramSource, many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins), source_class=NuisanceHistogramSource)
    lf = SourceWiseUnbinnedLogLikelihood(conf)
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
    lf.prepare()
    np.random.seed(3)
    d = lf.base_model.simulate()
    lf.set_data(d[:max(len(d) // 8, 1)])
    print('%d events scored on the %s: an event store of %.2f MB' % (lf.n_events_per_dataset[0], lf.last_scoring_route,
                                                                    lf.ctx.get_param('sourcewise_events_bytes') / 1e6))
    nuisance = own[0][0]                                          # the signal's first own parameter
    keep = [('s0_rate_multiplier', np.linspace(0.0, 1.0, 65))]
    reduce = [(nuisance, np.linspace(-2.0, 2.0, 33)), ('s1_rate_multiplier', np.linspace(0.02, 0.4, 25)),
              ('s2_rate_multiplier', np.linspace(0.02, 0.4, 25))]
    fixed = {n: 0.0 for n in names if n != nuisance}
    fixed['s3_rate_multiplier'] = 0.125
    results = {}
    for engine in ('native', 'host'):
        if engine == 'native':
            grid.grid_scan(lf, keep=keep, reduce=reduce, engine=engine, **fixed)     # (warm: allocations)
        t0 = time.perf_counter()
        res = results[engine] = grid.grid_scan(lf, keep=keep, reduce=reduce, engine=engine, **fixed)
        print('grid of %d x %d x %d x %d = %d points on the %s engine: %.3f s (%d chunks, %d launches, %d excluded points)'
              % (len(keep[0][1]), 33, 25, 25, res.counters[1], res.engine, time.perf_counter() - t0, res.counters[0], res.counters[3], res.excluded))
    rng = np.random.default_rng(1)
    W, steps, burn = 32, 2000, 500
    best = results['native']
    k = int(np.argmax(best.profile))
    at = dict([('s0_rate_multiplier', keep[0][1][k])] + [(n, float(best.best[n][k])) for n, _ in reduce])
    order = ['s0_rate_multiplier', 's1_rate_multiplier', 's2_rate_multiplier', nuisance]      # rate multipliers first, then shape parameters
    p0 = np.array([at[n] for n in order])[None, :] + 0.01 * rng.standard_normal((W, 4))
    p0[:, :3] = np.abs(p0[:, :3])
    t0 = time.perf_counter()
    run = sampler.sample_posterior(lf, n_walkers=W, n_steps=steps, seed=4, p0=p0, **fixed)
    assert run.names == order, run.names
    s0 = run.flat(discard=burn)[:, 0]
    print('chain over the same %d parameters: %d walkers x %d steps on the %s engine in %.3f s, acceptance %.3f, %d stream waits in the step loop'
          % (len(run.names), W, steps, run.engine, time.perf_counter() - t0, run.acceptance_fraction.mean(), run.counters[4]))
    print('90 % credible upper limit on s0_rate_multiplier (flat priors on the multipliers, the nuisance parameter\'s Gaussian constraint):')
    print('    gridded likelihood, native engine  %.4f' % results['native'].credible_upper_limit(0.9))
    print('    gridded likelihood, host engine    %.4f' % results['host'].credible_upper_limit(0.9))
    print('    chain (posterior quantile)         %.4f   (%.1f %% of the chain inside the grid\'s range of the multiplier)'
          % (np.quantile(s0, 0.9), 100 * np.mean(s0 <= keep[0][1][-1])))
    lf.ctx.close()


def measured_event_store(rng, N):
    """the measured source-wise shape over N events -- d = 4, S = 4, one own axis per source (class <4, 1>: 8 rows per point), 5
    anchors -- as a one-bin carrier of the geometry and the rates with random pdf values of order one uploaded row by row"""
    from blueice_amd.source_wise import SourceWiseContext
    d = S = 4
    n_a = 5
    g = np.linspace(-2., 2., n_a)
    mus = (1 + np.arange(S))[:, None] * (1 + 0.02 * g[None, :])                   # relative rates (10 in all); the scale is per call
    fac = SourceWiseContext(0)
    fac.begin_model([g] * d, S, 1, [(s,) for s in range(S)])
    for s in range(S):
        for a in range(n_a):
            fac.set_anchor(s, a, np.ones(1), mus[s, a])
    fac.end_model()
    values = rng.random((S, n_a, N)) + 0.05
    fac.set_event_rows([N], lambda s, local: values[s, local], 1e-12)
    return fac, d, S, n_a


def alternated(calls, rounds, warm=2):
    times = {name: [] for name, _ in calls}
    for rnd in range(warm + rounds):
        for name, call in calls:
            t0 = time.perf_counter()
            call()
            if rnd >= warm:
                times[name].append(time.perf_counter() - t0)
    return times


def measure_unbinned_grid():
    """The gridded likelihood on the event store at the measured shape: bi_grid_reduce_sourcewise_events (one work item per grid
    point, nothing read by the host per chunk) against the host engine (blueice_amd.grid._host_engine over a likelihood whose
    eval_points is bi_eval_factored on the same store, reduced by reduce_cells) on the same grid, at 10^4 and 10^6 events.
    Alternated calls, medians with quartiles, host clock around calls that end in a stream synchronisation.  There is no scan
    route over events.  Written to profiles/sourcewise_events_scan_measure.txt as well."""
    import os
    from blueice_amd import grid
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(11)
    first = True
    for events, nodes in ((1e4, [np.linspace(0.5, 1.5, 33), np.linspace(-1.9, 1.9, 65), np.linspace(-1.9, 1.9, 65), np.linspace(0.8, 1.2, 7)]),
                          (1e6, [np.linspace(0.5, 1.5, 33), np.linspace(-1.9, 1.9, 17), np.linspace(-1.9, 1.9, 17), np.linspace(0.8, 1.2, 7)])):
        N = int(events)
        fac, d, S, n_a = measured_event_store(rng, N)
        if first:
            say('# examples/many_nuisances.py --measure-unbinned-grid --rounds %d on %s' % (args.rounds, fac.info()['arch']))
            say('# d = %d, S = %d, one own axis per source (class <4, 1>: 8 rows per point), %d anchors, one event set; every other class: '
                'not measured.  The store (20 rows x N doubles) fits the Infinity Cache at both sizes: every number below is cache-assisted'
                % (d, S, n_a))
            first = False
        scale = events / 10.0
        names = ['r0', 'z0', 'z1', 'r1']
        kind, index = np.array([1, 0, 0, 1], dtype=np.int32), np.array([0, 0, 1, 1], dtype=np.int32)
        z0, scale0, unit = np.zeros((1, d)), np.full((1, S), scale), np.full((1, S), scale)
        G = int(np.prod([len(v) for v in nodes]))
        logw = [np.zeros(len(nodes[0]))] + [np.log(grid.trapezoid_weights(v)) for v in nodes[1:]]

        class HostLikelihood:
            """what _host_engine asks of a likelihood: eval_points over the axes' columns, through bi_eval_factored"""
            def eval_points(self, call, livetime_days=None):
                P = len(call['r0'])
                z, r = np.zeros((P, d)), np.full((P, S), scale)
                z[:, 0], z[:, 1], r[:, 0], r[:, 1] = call['z0'], call['z1'], scale * call['r0'], scale * call['r1']
                return fac.eval(z, r)[0]

        axes = list(zip(names, nodes))
        native = lambda: fac.grid_reduce_events(kind, index, z0, scale0, unit, None, 1, nodes, logw=logw, route=0)
        host = lambda: grid._host_engine(HostLikelihood(), axes, 1, logw[1:], None, None, None, {})
        a, h = native(), host()
        say('%.0e events, grid of %s = %d points, 16 cell tuples: route points %d chunk(s), %d launches; max |log_marginal difference| native - host '
            '%.2e, argmax equal: %s' % (events, ' x '.join(str(len(v)) for v in nodes), G, a[3][0], a[3][3], np.max(np.abs(a[0].ravel() - h[0])),
                                        np.array_equal(a[2].ravel(), h[2])))
        rounds = max(3, args.rounds // 8)
        t = alternated([('native', native), ('host', host)], rounds, warm=1)
        for name, what in (('native', 'bi_grid_reduce_sourcewise_events route points'), ('host', 'host engine, bi_eval_factored per 65 536 points')):
            say('    %-48s %s   %.3f M points/s' % (what, quartiles(t[name]), G / np.median(t[name]) / 1e6))
        say('    ratio host / native %.2f' % (np.median(t['host']) / np.median(t['native'])))
        fac.close()
    say('# not measured: a scan route over events (none exists: route 1 is refused), the 10^6-point grid at 10^6 events (the grid there is '
        '33 x 17 x 17 x 7), blueice_amd.grid.grid_scan through the likelihood class, every class but <4, 1>, several event sets')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_events_scan_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


def measure_unbinned_sampler():
    """The ensemble sampler on the event store at the measured shape: bi_sample_stretch_sourcewise_events (propose, the planner's
    event variant, k_sourcewise_events, finish and accept queued on one stream) against the host engine of blueice_amd.sampler -- the
    same move in NumPy, one bi_eval_factored call per half-step -- at 40 and 1024 walkers for 50 steps, 10^4 and 10^6 events.
    Alternated calls, medians with quartiles.  Written to profiles/sourcewise_events_sampler_measure.txt as well."""
    import os
    from blueice_amd import sampler
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(11)
    steps = 50
    first = True
    for events in (1e4, 1e6):
        fac, d, S, n_a = measured_event_store(rng, int(events))
        if first:
            say('# examples/many_nuisances.py --measure-unbinned-sampler --rounds %d on %s' % (args.rounds, fac.info()['arch']))
            say('# d = %d, S = %d, one own axis per source (class <4, 1>), %d anchors, one event set; every other class: not measured.  The store '
                '(20 rows x N doubles) fits the Infinity Cache at both sizes: every number below is cache-assisted' % (d, S, n_a))
            first = False
        scale = events / 10.0
        kind = np.array([1] * S + [0] * d, dtype=np.int32)
        index = np.array(list(range(S)) + list(range(d)), dtype=np.int32)
        names = ['r%d' % s for s in range(S)] + ['z%d' % i for i in range(d)]
        lo, hi = np.array([0.] * S + [-2.] * d), np.array([np.inf] * S + [2.] * d)
        z0, one, unit = np.zeros(d), np.full(S, scale), np.full(S, scale)

        class HostLikelihood:
            """what _host_engine asks of a likelihood: eval_points over the variables' columns, through bi_eval_factored"""
            def eval_points(self, call, livetime_days=None):
                return fac.eval(np.stack([call[n] for n in names[S:]], axis=1), scale * np.stack([call[n] for n in names[:S]], axis=1))[0]

        for W in (40, 1024):
            x0 = np.concatenate([rng.uniform(0.99, 1.01, (W, S)), rng.uniform(-0.1, 0.1, (W, d))], axis=1)[None]
            native = lambda: fac.sample_stretch_events(W, kind, index, z0, one, unit, None, x0, lo, hi, steps, seed=7)
            host = lambda: sampler._host_engine(HostLikelihood(), names, {}, None, None, x0.copy(), lo, hi, steps, 2.0, 7, 0)
            a, b = native(), host()
            say('%.0e events, W = %4d, %d steps: counters of the device loop %s (half-steps, evaluations, accepted, launches, stream waits in the '
                'loop); accepted on the host %d; %.1f %% of the chain entries equal bit for bit'
                % (events, W, steps, [int(v) for v in a[3]], b[3][2], 100 * np.mean(a[0] == b[0])))
            rounds = args.rounds if events * W < 1e8 else max(3, args.rounds // 8)
            t = alternated([('native', native), ('host', host)], rounds, warm=1)
            for name, what in (('native', 'bi_sample_stretch_sourcewise_events'), ('host', 'host engine, bi_eval_factored per half-step')):
                say('%.0e events, W = %4d, %d steps, %-46s %s per call, %.1f us per half-step'
                    % (events, W, steps, what, quartiles(t[name]), np.median(t[name]) * 1e6 / (2 * steps)))
            say('%.0e events, W = %4d: ratio host / native %.2f' % (events, W, np.median(t['host']) / np.median(t['native'])))
        fac.close()
    say('# not measured: blueice_amd.sampler.sample_posterior through the likelihood class, constraint terms, several ensembles, every class '
        'but <4, 1>')
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sourcewise_events_sampler_measure.txt')
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if args.unbinned_posterior:
    unbinned_posterior()
    raise SystemExit(0)
if args.measure_unbinned_grid:
    measure_unbinned_grid()
    raise SystemExit(0)
if args.measure_unbinned_sampler:
    measure_unbinned_sampler()
    raise SystemExit(0)
if args.unbinned_toys:
    unbinned_toys()
    raise SystemExit(0)
if args.measure_unbinned_toys:
    measure_unbinned_toys()
    raise SystemExit(0)
if args.unbinned:
    unbinned()
    raise SystemExit(0)
if args.measure_unbinned:
    measure_unbinned()
    raise SystemExit(0)
if args.measure_unbinned_hessian:
    measure_unbinned_hessian()
    raise SystemExit(0)
if args.grid:
    grid_limit()
    raise SystemExit(0)
if args.measure_grid:
    measure_grid()
    raise SystemExit(0)
if args.measure_sampler:
    measure_sampler()
    raise SystemExit(0)
if args.measure_nonempty:
    measure_nonempty()
    raise SystemExit(0)
if args.posterior:
    posterior()
    raise SystemExit(0)
if args.measure:
    measure()
    raise SystemExit(0)
if args.measure_asimov:
    measure_asimov()
    raise SystemExit(0)
if args.measure_coarse:
    measure_coarse()
    raise SystemExit(0)
if args.asimov:
    asimov_band()
    raise SystemExit(0)
if args.measure_coarse_jacobian:
    measure_coarse_jacobian()
    raise SystemExit(0)
if args.band:
    band()
    raise SystemExit(0)
if args.measure_toys:
    measure_toys()
    raise SystemExit(0)

from blueice_amd import GaussianPrior, SourceWiseBinnedLogLikelihood  # noqa: E402
from blueice_amd.synthetic import many_nuisances_config  # noqa: E402

conf, names, own = many_nuisances_config(n_bins=(args.bins, args.bins))
lf = SourceWiseBinnedLogLikelihood(conf)
for s in range(4):
    lf.add_rate_parameter('s%d' % s)
for n in names:
    lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.), log_prior=GaussianPrior(0., 1.))
t0 = time.perf_counter()
lf.prepare()
print('(1) prepare(): %d shape parameters x 5 anchors, %d sources responding to %s: %d rows on the device instead of 5^%d x %d, %.2f s'
      % (len(names), 4, ', '.join('/'.join(o) for o in own), sum(5 ** len(o) for o in own), len(names), 4, time.perf_counter() - t0))
np.random.seed(3)
data = lf.base_model.simulate()
lf.set_data(data)
print('    set_data(): %d events binned on the device into %d x %d bins' % (len(data), args.bins, args.bins))

t0 = time.perf_counter()
best, ll, info = lf.bestfit_batched(return_info=True)
print('(2) bestfit_batched, %d parameters floating: max ll %.4f, converged %s, %d evaluations in %d device calls, %.3f s'
      % (len(best), ll[0], bool(info['converged'][0]), info['evaluations'], info['calls'], time.perf_counter() - t0))
print('    ' + ', '.join('%s %.3f' % (k.replace('_rate_multiplier', ''), v[0]) for k, v in best.items()))

grid = np.linspace(0.7, 1.3, args.scan)
t0 = time.perf_counter()
scan = lf.likelihood_ratio_scan(('s0_rate_multiplier', grid))
dt = time.perf_counter() - t0
inside = grid[2 * scan <= 1.0]
print('(3) likelihood_ratio_scan over s0_rate_multiplier: %d hypotheses, 11 nuisances profiled at each, %.3f s; minimum at %.3f, '
      '2 dlnL <= 1 on [%.3f, %.3f]' % (args.scan, dt, grid[np.argmin(scan)], inside.min(), inside.max()))
limit = lf.one_parameter_interval('s0_rate_multiplier', 3.0, confidence_level=0.9, kind='upper')
print('    90 %% upper limit on s0_rate_multiplier (one_parameter_interval): %.4f' % limit)

t0 = time.perf_counter()
fit, ll_fit = lf.bestfit_minuit()
order = [k for k in fit if not k.endswith('_error')]
print('(4) bestfit_minuit: max ll %.4f, errors from the analytic Hessian over all %d parameters, %.3f s' % (ll_fit, len(order), time.perf_counter() - t0))
truth = dict([('s%d_rate_multiplier' % s, 1.0) for s in range(4)] + [(n, 0.0) for n in names])
expected = lf.expected_errors(**truth)
for k in order:
    print('    %-20s %8.4f +- %.4f     expected error at the truth %.4f' % (k, fit[k], fit[k + '_error'], expected[k]))
from blueice_amd.inference import hesse  # noqa: E402
cov_names, cov = hesse(lf, {k: fit[k] for k in order})
sigma = np.sqrt(np.diag(cov))
print('    correlation matrix (%s):' % ', '.join(k.replace('_rate_multiplier', '') for k in cov_names))
for row in cov / np.outer(sigma, sigma):
    print('    ' + ' '.join('%6.2f' % v for v in row))

from blueice_amd import inference  # noqa: E402
t0 = time.perf_counter()
gof = inference.goodness_of_fit(lf, n_toys=args.toys, seed=1)
print('(5) goodness_of_fit: deviance %.2f over %d bins - %d floating = %d degrees of freedom; p = %.3f from %d toys (%d failed fits), '
      'asymptotic p = %.3f, %.3f s' % (gof.observed, args.bins ** 2, len(gof.best), gof.ndof, gof.p_value, len(gof.toys), gof.n_failed,
                                     gof.p_value_chi2, time.perf_counter() - t0))
mu = inference.expected_counts_points(lf, {k: np.array([v]) for k, v in gof.best.items()}, per_source=True)[0]
print('    expected events per source at the fit: ' + ', '.join('%.1f' % v for v in mu.reshape(4, -1).sum(axis=1))
      + '; observed %d' % len(data))

hyp = np.linspace(0.8, 1.6, 5)
n_per = max(args.toys // 5, 10)
t0 = time.perf_counter()
table = lf.neyman_thresholds('s0_rate_multiplier', hyp, n_per, kind='upper', seed=2)
print('(6) neyman_thresholds: %d toys at each of %d hypotheses of s0_rate_multiplier, two fits per toy in lock-step, %.3f s'
      % (n_per, len(hyp), time.perf_counter() - t0))
print('    critical values of the 90 % upper limit: ' + ', '.join('%.2f' % v for v in table.critical_values(0.9))
      + '   (Wilks: 1.64)')
limit_toys = lf.one_parameter_interval('s0_rate_multiplier', 3.0, confidence_level=0.9, kind='upper', t_ppf=table)
print('    90 %% upper limit with the toy-calibrated thresholds: %.4f (Wilks: %.4f)' % (limit_toys, limit))
