"""Posterior sampling: Goodman & Weare's affine-invariant stretch move over a likelihood's floating parameters -- the
sampler behind the reference's `bestfit_emcee` (blueice/inference.py:254-321, emcee's EnsembleSampler with its default
StretchMove), without emcee.

A stretch move updates half of the walkers at once from the positions of the other half: a batch of independent points,
which is what the device evaluates best.  Two engines run the SAME algorithm on the SAME random stream (Philox4x32-10,
documented with `bi_sample_stretch` in include/blueice_hip.h):

    'native'   bi_sample_stretch: propose, evaluate, accept and the chain stay on the device; taken whenever nothing but
               the device call sits between the parameters and the likelihood (`BatchObjective.native()`); Gaussian
               constraints (`priors.GaussianPrior`) are added on the device (bi_sample_stretch_gauss); a source-wise model
               (`SourceWiseBinnedLogLikelihood`) has bi_sample_stretch_sourcewise behind the same `ctx.sample_stretch`; an
               unbinned one (`SourceWiseUnbinnedLogLikelihood`, taken by this function, not as a bound method) has
               bi_sample_stretch_sourcewise_events, `ctx.sample_stretch_events`, through the class's `_native_sample_stretch`
    'host'     the restatement below in NumPy, one `lf.eval_points` call per half-step -- for likelihoods with other
               Python callables as priors, sums, re-parametrisations, efficiencies, unphysical_behaviour='error', and
               models whose batches the device planner refuses

Proposals are bitwise the same in both; accept decisions differ only where the two evaluations of the likelihood do.
"""
import numpy as np

from .exceptions import PlannerRefused
from .profile import BatchObjective

__all__ = ['sample_posterior', 'SamplerResult', 'philox4x32_10', 'stretch_draws', 'STRETCH_TAG']

STRETCH_TAG = 0x53545200
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 blocks for arrays of counters (c0..c3) and keys (k0, k1), all 32-bit values -> four uint64 arrays
    holding the 32-bit output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def stretch_draws(seed, ensembles, W, t, h, a):
    """The draws of half-step (t, h) for the moving walkers of every ensemble in `ensembles` (global numbers [E]):
    -> (k [W/2] moving walkers, j [E, W/2] partners, z [E, W/2] stretch factors, u_a [E, W/2])."""
    half = W // 2
    k = h * half + np.arange(half)
    seed = int(seed) & (2 ** 64 - 1)
    r0, r1, r2, r3 = philox4x32_10(k[None, :], np.asarray(ensembles, dtype=np.uint64)[:, None], int(t) & 0xFFFFFFFF, STRETCH_TAG | h,
                                   seed & 0xFFFFFFFF, seed >> 32)
    u_z = ((r0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (r1 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    j = (1 - h) * half + ((r2 * np.uint64(half)) >> np.uint64(32)).astype(np.int64)
    u_a = (r3.astype(np.float64) + 0.5) * 2.0 ** -32
    g = (a - 1.0) * u_z + 1.0
    z = (g * g) / a
    return k, j, z, u_a


class SamplerResult:
    """names [F]; chain [n_steps, (E,) W, F] -- the walkers after every step; log_prob [n_steps, (E,) W];
    acceptance_fraction [(E,) W]; engine 'native' or 'host'; counters: half-steps, evaluations, accepted moves, launches."""

    def __init__(self, names, chain, log_prob, n_accepted, engine, counters):
        self.names, self.chain, self.log_prob, self.engine = list(names), chain, log_prob, engine
        self.n_accepted = n_accepted
        self.acceptance_fraction = n_accepted / max(1, len(chain))
        self.counters = counters

    def flat(self, discard=0):
        """samples [-1, F] without the first `discard` steps, walker by walker as emcee's `chain[:, discard:, :].reshape(-1, F)`"""
        c = self.chain[discard:]
        return np.moveaxis(c, 0, -2).reshape(-1, c.shape[-1])


def _host_engine(lf, names, fixed, livetime_days, datasets, x, lo, hi, n_steps, a, seed, first_ensemble):
    E, W, F = x.shape
    half = W // 2

    def evaluate(pts, ens):
        """ll of points pts [n, F] that belong to ensembles ens [n]"""
        call = {n: pts[:, v] for v, n in enumerate(names)}
        call.update(fixed)
        more = {} if datasets is None else {'dataset': datasets[ens]}
        return np.asarray(lf.eval_points(call, livetime_days=livetime_days, **more), dtype=float)

    ens_all = np.repeat(np.arange(E), W)
    ll = evaluate(x.reshape(-1, F), ens_all).reshape(E, W).copy()
    if not np.all(np.isfinite(ll)):
        e, k = np.argwhere(~np.isfinite(ll))[0]
        raise ValueError("sample_posterior: the log likelihood of start walker %d of ensemble %d is not finite (%s): every "
                         "walker must start at a point of non-zero likelihood" % (k, e, ll[e, k]))
    chain = np.empty((n_steps, E, W, F))
    log_prob = np.empty((n_steps, E, W))
    n_acc = np.zeros((E, W), dtype=np.int64)
    counters = np.array([0, E * W, 0, 0], dtype=np.int64)
    rows = np.arange(E)[:, None]
    for t in range(n_steps):
        for h in (0, 1):
            k, j, z, u_a = stretch_draws(seed, first_ensemble + np.arange(E), W, t, h, a)
            xk, xj = x[:, k, :], x[rows, j, :]
            y = xj + z[..., None] * (xk - xj)
            inside = np.all((y >= lo) & (y <= hi), axis=-1)
            ll_y = np.full((E, half), -np.inf)
            if inside.any():
                ll_y[inside] = evaluate(y[inside], np.broadcast_to(rows, (E, half))[inside])
            counters[1] += int(inside.sum())
            with np.errstate(invalid='ignore'):
                q = ((F - 1) * np.log(z) + ll_y) - ll[:, k]
                take = inside & np.isfinite(ll_y) & (np.log(u_a) < q)
            x[:, k, :] = np.where(take[..., None], y, xk)
            ll[:, k] = np.where(take, ll_y, ll[:, k])
            n_acc[:, k] += take
            counters[0] += 1
        chain[t], log_prob[t] = x, ll
    counters[2] = n_acc.sum()
    return chain, log_prob, n_acc, counters


def sample_posterior(lf, n_walkers=40, n_steps=200, a=2.0, seed=0, guess=None, p0=None, datasets=None, livetime_days=None,
                     engine=None, first_ensemble=0, **fixed):
    """Sample the likelihood's floating parameters (all those not named in `fixed`; rate multipliers first, then shape
    parameters -- names, guesses and bounds from `make_objective`) with `n_walkers` walkers for `n_steps` steps.

    p0 [W, F] (or [E, W, F]): the start; default the reference's, guess * U(0.95, 1.05) per walker
    (blueice/inference.py:284) from numpy.random.default_rng(seed) -- a guess of 0 leaves that parameter without spread,
    pass p0 or `guess` then.  datasets: one ensemble per dataset the likelihood holds (`simulate_toys`, a stack given to
    `set_binned_data`), all in the same call; ensemble e is ensemble first_ensemble + e of the seed's random stream.
    engine: None (native where possible), 'native', 'host'.  -> SamplerResult."""
    W, n_steps = int(n_walkers), int(n_steps)
    if W < 2 or W % 2:
        raise ValueError("sample_posterior: the stretch move needs an even number of walkers >= 2 (got %d)" % W)
    if not a > 1:
        raise ValueError("sample_posterior: the stretch scale a must be > 1 (got %r)" % (a,))
    if n_steps < 0:
        raise ValueError("sample_posterior: n_steps must be >= 0")
    if engine not in (None, 'native', 'host'):
        raise ValueError("sample_posterior: engine must be None, 'native' or 'host'")
    _, names, guesses, bounds = lf.make_objective(minus=False, guess=guess, **fixed)
    F = len(names)
    lo = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=float)
    hi = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=float)
    if datasets is not None:
        datasets = np.atleast_1d(np.asarray(datasets, dtype=np.int64))
    E = 1 if datasets is None else len(datasets)
    if p0 is None:
        p0 = np.random.default_rng(seed).uniform(0.95, 1.05, size=(W, F)) * np.asarray(guesses, dtype=float)
    p0 = np.asarray(p0, dtype=float)
    if p0.shape not in ((W, F), (E, W, F)):
        raise ValueError("sample_posterior: p0 must have shape [n_walkers, %d]%s" % (F, '' if datasets is None else ' or [%d, n_walkers, %d]' % (E, F)))
    x = np.ascontiguousarray(np.broadcast_to(p0, (E, W, F))).copy()
    outside = ~np.all((x >= lo) & (x <= hi), axis=-1)
    if outside.any():
        e, k = np.argwhere(outside)[0]
        raise ValueError("sample_posterior: start walker %d of ensemble %d lies outside the bounds of the parameters" % (k, e))

    native = None
    if engine != 'host':
        native = BatchObjective(lf, names, {}, fixed, livetime_days, datasets).native()
        if native is None and engine == 'native':
            raise ValueError("sample_posterior: this likelihood has Python between its parameters and the device call (priors "
                             "that are not a GaussianPrior, efficiencies, a sum or re-parametrisation): engine='host'")
    result = None
    if native is not None:
        try:
            priors = None
            if np.any(np.isfinite(native['prior_sigma'])) or np.any(native['prior_const'] != 0):
                priors = (native['prior_mean'], native['prior_sigma'], native['prior_const'])
            stretch = getattr(lf, '_native_sample_stretch', None) or lf.ctx.sample_stretch
            result = stretch(W, native['kind'], native['index'], native['z0'], native['scale0'], native['unit'], datasets, x, lo, hi, n_steps,
                             a=a, seed=seed, first_ensemble=first_ensemble, priors=priors)
            used = 'native'
        except PlannerRefused:
            if engine == 'native':
                raise
    if result is None:
        result = _host_engine(lf, names, fixed, livetime_days, datasets, x, lo, hi, n_steps, float(a), seed, int(first_ensemble))
        used = 'host'
    chain, log_prob, n_acc, counters = result
    if datasets is None:
        chain, log_prob, n_acc = chain[:, 0], log_prob[:, 0], n_acc[0]
    return SamplerResult(names, chain, log_prob, n_acc, used, counters)
