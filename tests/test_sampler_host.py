"""The ensemble sampler without a GPU: the host engine of blueice_amd.sampler (the NumPy restatement of bi_sample_stretch)
against the independent oracle of tests/sampler_oracle.py over the CPU-oracle likelihood, the known posterior, the
refusals, and the drop-ins built on the sampler (bestfit_emcee, plot_likelihood_ratio)."""
import numpy as np
import pytest
from scipy import stats

import sampler_oracle as so
from golden_util import load_case
from oracle_lf import OracleLikelihood


def oracle_lf(name):
    c = load_case(name)
    names = ['z%d' % i for i in range(c['d'])]
    return OracleLikelihood(c['model'], c['counts'], names), c


def start_of(lf, names, W, seed):
    """walkers around multipliers of 1 and the middle of every shape parameter's anchor range"""
    rng = np.random.default_rng(seed)
    cols = []
    for n in names:
        if n in lf.shape_parameters:
            lo, hi = lf.get_bounds(n)
            cols.append(0.5 * (lo + hi) + (hi - lo) * rng.uniform(-0.1, 0.1, W))
        else:
            cols.append(rng.uniform(0.9, 1.1, W))
    return np.stack(cols, axis=1)


def gamma_lf(counts=(50.0, 20.0)):
    """two sources that each fill their own bin, expectation 1 per unit multiplier: mu_s ~ Gamma(n_s + 1, 1)"""
    model = dict(anchor_z=[], ps=np.eye(2), mus=np.ones(2), n_model=None)
    return OracleLikelihood(model, np.array(counts), [])


def test_philox_known_answers():
    from blueice_amd.sampler import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert so.philox(ctr, key) == want
        assert tuple(int(v) for v in philox4x32_10(*ctr, *key)) == want
    rng = np.random.default_rng(1)
    ctrs = rng.integers(0, 2 ** 32, size=(50, 6), dtype=np.uint64)
    got = np.stack(philox4x32_10(*ctrs.T), axis=1)
    for row, g in zip(ctrs, got):
        assert so.philox(tuple(int(v) for v in row[:4]), tuple(int(v) for v in row[4:])) == tuple(int(v) for v in g)


def test_draws_match_the_oracle_bitwise():
    from blueice_amd.sampler import stretch_draws
    for W, h, t, a in ((8, 0, 0, 2.0), (8, 1, 5, 2.0), (64, 1, 123, 1.7)):
        k, j, z, u_a = stretch_draws(77 + (5 << 32), np.array([0, 3]), W, t, h, a)
        for e, ens in enumerate((0, 3)):
            for i, kk in enumerate(k):
                jj, zz, uu = so.draw(77 + (5 << 32), ens, W, t, h, int(kk), a)
                assert (jj, zz, uu) == (j[e, i], z[e, i], u_a[e, i])


@pytest.mark.parametrize('name, F, W', [('d2_nonuniform', 1, 8), ('d2_nonuniform', None, 8), ('c1_like', 2, 8), ('c1_like', None, 64)])
def test_host_engine_replays_exactly(name, F, W):
    """band zero: every proposal, recorded log likelihood and decision of the host engine is the oracle's"""
    from blueice_amd.sampler import sample_posterior
    lf, c = oracle_lf(name)
    all_names = [n + '_rate_multiplier' for n in lf.source_name_list] + list(lf.shape_parameters)
    F = len(all_names) if F is None else F
    names = all_names[:F]
    fixed = {n: (1.0 if n.endswith('_rate_multiplier') else 0.5 * sum(lf.get_bounds(n))) for n in all_names[F:]}
    p0 = start_of(lf, names, W, 3)
    steps = 12 if W == 8 else 4
    res = sample_posterior(lf, n_walkers=W, n_steps=steps, seed=11, p0=p0, **fixed)
    assert res.engine == 'host' and res.names == names and res.chain.shape == (steps, W, F)
    bounds = [lf.get_bounds(n) for n in names]
    lo, hi = np.array([b[0] for b in bounds], dtype=float), np.array([b[1] for b in bounds], dtype=float)

    def ll_of(pts):
        call = {n: pts[:, v] for v, n in enumerate(names)}
        call.update(fixed)
        return lf.eval_points(call)

    n_dec, n_band, n_acc = so.replay(res.chain, res.log_prob, p0, ll_of, lo, hi, seed=11, a=2.0, ll_rtol=0.0, band_abs=0.0, band_log=0.0)
    assert n_dec == steps * W and n_band == 0
    assert n_acc == res.n_accepted.sum() == res.counters[2] and n_acc > 0
    assert np.all((res.chain >= lo) & (res.chain <= hi))


def check_gamma(samples, counts):
    for s, n in enumerate(counts):
        mean, var = samples[:, s].mean(), samples[:, s].var()
        print('source %d: mean %.3f (want %.1f), variance %.3f' % (s, mean, n + 1, var))
        assert abs(mean - (n + 1)) <= 0.15 * np.sqrt(n + 1)
        assert 0.8 * (n + 1) <= var <= 1.2 * (n + 1)


def test_known_posterior_host():
    from blueice_amd.sampler import sample_posterior
    lf = gamma_lf()
    res = sample_posterior(lf, n_walkers=32, n_steps=1200, seed=5, guess={'s0_rate_multiplier': 51.0, 's1_rate_multiplier': 21.0})
    assert res.engine == 'host'
    check_gamma(res.flat(discard=200), (50, 20))
    assert 0.2 < res.acceptance_fraction.mean() < 0.9


def test_seeds_and_refusals():
    from blueice_amd.sampler import sample_posterior
    lf = gamma_lf()
    g = {'s0_rate_multiplier': 51.0, 's1_rate_multiplier': 21.0}
    a = sample_posterior(lf, n_walkers=8, n_steps=20, seed=1, guess=g)
    b = sample_posterior(lf, n_walkers=8, n_steps=20, seed=1, guess=g)
    c = sample_posterior(lf, n_walkers=8, n_steps=20, seed=2, guess=g)
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.log_prob, b.log_prob)
    assert not np.array_equal(a.chain, c.chain)
    with pytest.raises(ValueError, match='even number of walkers'):
        sample_posterior(lf, n_walkers=7, guess=g)
    with pytest.raises(ValueError, match='even number of walkers'):
        sample_posterior(lf, n_walkers=0, guess=g)
    with pytest.raises(ValueError, match='must be > 1'):
        sample_posterior(lf, n_walkers=8, a=1.0, guess=g)
    with pytest.raises(ValueError, match='not finite'):
        sample_posterior(lf, n_walkers=8, p0=np.zeros((8, 2)))                   # inside the box, likelihood zero
    with pytest.raises(ValueError, match='start walker 5 of ensemble 0 lies outside the bounds'):
        sample_posterior(lf, n_walkers=8, p0=np.where(np.arange(8)[:, None] == 5, -1.0, 50.0) * np.ones((8, 2)))
    with pytest.raises(ValueError, match="engine='host'"):
        sample_posterior(lf, n_walkers=8, guess=g, engine='native')


def test_bestfit_emcee_shapes_and_gamma_quantiles():
    from blueice_amd import inference
    lf = gamma_lf()
    g = {'s0_rate_multiplier': 51.0, 's1_rate_multiplier': 21.0}
    kw = dict(quiet=True, n_walkers=32, n_steps=1200, n_burn_in=200, seed=9, guess=g)
    best, ll = inference.bestfit_emcee(lf, **kw)
    assert list(best) == ['s0_rate_multiplier', 's1_rate_multiplier'] and ll == lf(**best)
    best2, ll2, err = inference.bestfit_emcee(lf, return_errors=True, **kw)
    best3, ll3, samples = inference.bestfit_emcee(lf, return_samples=True, **kw)
    assert best2 == best == best3 and ll2 == ll == ll3
    assert list(err) == list(best) and samples.shape == (32 * 1000, 2)
    for s, n in enumerate((50, 20)):
        dist = stats.gamma(n + 1)
        key = 's%d_rate_multiplier' % s
        lo, hi = dist.ppf(stats.norm.cdf([-1, 1]))
        assert abs(best[key] - dist.median()) <= 0.15 * np.sqrt(n + 1)
        assert 0.8 <= (err[key] / ((hi - lo) / 2)) ** 2 <= 1.2
    # one parameter held fixed: it is handed to the likelihood call as well
    best4, ll4 = inference.bestfit_emcee(lf, quiet=True, n_walkers=8, n_steps=30, n_burn_in=10, s1_rate_multiplier=20.0,
                                         guess={'s0_rate_multiplier': 51.0})
    assert list(best4) == ['s0_rate_multiplier'] and ll4 == lf(s1_rate_multiplier=20.0, **best4)
    for key in ('datasets', 'first_ensemble'):
        with pytest.raises(ValueError, match='option of sample_posterior'):
            inference.bestfit_emcee(lf, quiet=True, **{key: [0]})


def test_bestfit_emcee_prints_acceptance(capsys):
    from blueice_amd import inference
    inference.bestfit_emcee(gamma_lf(), n_walkers=8, n_steps=20, n_burn_in=5, guess={'s0_rate_multiplier': 51.0, 's1_rate_multiplier': 21.0})
    assert 'Mean acceptance fraction: 0.' in capsys.readouterr().out


def test_plot_likelihood_ratio_draws_the_scan():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from blueice_amd import inference
    lf = gamma_lf()
    x = np.linspace(30.0, 70.0, 9)
    plt.figure()
    got = inference.plot_likelihood_ratio(lf, ('s0_rate_multiplier', x), s1_rate_multiplier=21.0)
    want = inference.likelihood_ratio_scan(lf, ('s0_rate_multiplier', x), s1_rate_multiplier=21.0)
    assert np.array_equal(got, want)
    ax = plt.gca()
    assert len(ax.lines) == 1 and np.array_equal(ax.lines[0].get_ydata(), want) and ax.get_xlabel() == 's0_rate_multiplier'
    plt.close('all')
    plt.figure()
    y = np.linspace(10.0, 30.0, 5)
    got2 = inference.plot_likelihood_ratio(lf, ('s0_rate_multiplier', x), ('s1_rate_multiplier', y), vmax=10)
    assert got2.shape == (9, 5) and np.array_equal(got2, inference.likelihood_ratio_scan(lf, ('s0_rate_multiplier', x), ('s1_rate_multiplier', y)))
    assert len(plt.gcf().axes[0].collections) == 1
    plt.close('all')
    with pytest.raises(ValueError):
        inference.plot_likelihood_ratio(lf)


def test_names_are_public_and_methods():
    from blueice_amd import inference, likelihood
    for name in ('sample_posterior', 'bestfit_emcee', 'plot_likelihood_ratio'):
        assert name in inference.__all__
        for cls in (likelihood.BinnedLogLikelihood, likelihood.LogLikelihoodSum, likelihood.LogLikelihoodReParam):
            assert callable(getattr(cls, name))
