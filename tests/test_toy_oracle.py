"""The toy oracle checked on the CPU: Philox known answers, the inversion loop against the exact quantile, the law of the
PTRS restatement, the undecided share on every input the GPU replay uses, and mutants of the streams that the comparison
must reject (tests/toy_oracle.py; the device side is tests/test_toy_replay_gpu.py)."""
import numpy as np
import pytest
from scipy import stats

import sampler_oracle
import toy_oracle as orc
import toy_replay_cases as cases

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers_and_the_vectorised_form():
    for counter, key, want in KAT:
        assert sampler_oracle.philox(counter, key) == want
        assert tuple(int(v) for v in orc.philox_v(*counter, *key)) == want
    rng = np.random.default_rng(1)
    words = rng.integers(0, 2 ** 32, size=(6, 200), dtype=np.uint64)
    got = np.stack(orc.philox_v(*words))
    for i in range(words.shape[1]):
        assert tuple(int(v) for v in got[:, i]) == sampler_oracle.philox(words[:4, i], words[4:, i])
    hi, lo = np.array([0xFFFFFFFF, 0, 32], dtype=np.uint64), np.array([0xFFFFFFFF, 63, 64], dtype=np.uint64)
    np.testing.assert_array_equal(orc.u53(hi, lo), [1.0 - 2.0 ** -53, 0.0, 2.0 ** -27 + 2.0 ** -53])


@pytest.fixture(scope='module')
def uniforms():
    c = np.arange(1_000_000, dtype=np.uint64)
    r0, r1, r2, r3 = orc.philox_v(c, 0, 7, 0, 99, 0)
    return orc.u53(r0, r1)


@pytest.mark.parametrize('lam', [0.004, 0.7, 3.3, 9.9, float(np.nextafter(10.0, 0.0)), 2.0 ** -20])
def test_inversion_loop_equals_the_exact_quantile(uniforms, lam):
    """The device loop in plain binary64 against the exact quantile (long double, compensated) on 10^6 uniforms, and the
    quantile against scipy's and against mpmath's CDF at the steps it stopped at."""
    import mpmath as mp
    n, und = orc.poisson_quantile(lam, uniforms)
    assert und.sum() <= orc.CAP * len(uniforms), und.sum()
    loop = orc.poisson_small_f64(lam, uniforms)
    ok = ~und
    np.testing.assert_array_equal(loop[ok], n[ok])
    np.testing.assert_array_equal(n[ok], stats.poisson.ppf(uniforms[ok], lam))
    mp.mp.prec = 200
    for i in range(0, len(uniforms), 50_000):
        k, u = int(n[i]), mp.mpf(float(uniforms[i]))
        cdf = lambda m: mp.exp(-mp.mpf(lam)) * mp.fsum(mp.mpf(lam) ** j / mp.factorial(j) for j in range(m + 1))
        assert u <= cdf(k) and (k == 0 or u > cdf(k - 1))


@pytest.mark.parametrize('lam', [10.0, 10.5, 37.0, 250.0, 1e4])
def test_ptrs_restatement_has_the_poisson_law(lam):
    """Rejection sampling has no closed-form answer per uniform, so here the LAW of the oracle's sampler is shown: 10^7
    Philox draws per mu against the exact pmf, chi-square over cells of expected count >= 50, p > 10^-6.  Seeds are fixed:
    deterministic."""
    n_draws, chunk = 10_000_000, 2_000_000
    parts = [orc.poisson_ptrs(np.full(chunk, lam), 2024, np.arange(i, i + chunk, dtype=np.uint64), 5) for i in range(0, n_draws, chunk)]
    k, und = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    assert und.sum() <= orc.CAP * n_draws, und.sum()
    assert np.all(k >= 0) and np.all(k == np.floor(k))
    lo, hi = int(stats.poisson.ppf(1e-9, lam)), int(stats.poisson.isf(1e-9, lam)) + 1
    ks = np.arange(lo, hi + 1)
    expected = stats.poisson.pmf(ks, lam) * n_draws
    observed = np.bincount(np.clip(k.astype(np.int64), lo, hi) - lo, minlength=len(ks)).astype(float)
    expected[0] += stats.poisson.cdf(lo - 1, lam) * n_draws
    expected[-1] += stats.poisson.sf(hi, lam) * n_draws
    # merge cells inwards from both tails until every cell expects >= 50
    e, o = list(expected), list(observed)
    for side in (0, -1):
        step = 1 if side == 0 else -2
        while e[side] < 50 or e[side + (1 if side == 0 else -1)] < 50:
            i = 0 if side == 0 else len(e) - 2
            e[i:i + 2], o[i:i + 2] = [e[i] + e[i + 1]], [o[i] + o[i + 1]]
    e, o = np.array(e), np.array(o)
    assert e.min() >= 50 and abs(e.sum() - n_draws) < 1e-3 * n_draws
    chi2 = np.sum((o - e) ** 2 / e)
    p = stats.chi2.sf(chi2, len(e) - 1)
    assert p > 1e-6, (lam, chi2, len(e), p)


# ---- the undecided share on the inputs of the GPU replay -----------------------------------------------------------------

def _per_bin_replays():
    for B, shift in cases.PER_BIN_CASES:
        yield 'A B=%d shift=%d' % (B, shift), orc.per_bin_toys(cases.per_bin_mu(B, shift), cases.SEED, np.arange(cases.T_PER_BIN))


def _event_replays(small_only=False):
    for B, M, T, path in cases.EVENT_CASES:
        if small_only and M > 2000:
            continue
        mu = cases.event_mu(B, M)
        yield 'B B=%d M=%g' % (B, M), (orc.event_toys if path else orc.per_bin_toys)(mu, cases.SEED, np.arange(T))


def test_undecided_share_of_the_gpu_inputs_is_within_the_cap():
    """Case by case (the small stream-A cases pooled per bin count: a case of 8 draws cannot show a share of 10^-5)."""
    pooled = {}
    for name, rep in _per_bin_replays():
        key = name.split(' shift')[0]
        d, u = pooled.get(key, (0, 0))
        pooled[key] = (d + rep.draws, u + rep.undecided)
    for name, rep in _event_replays():
        pooled[name] = (rep.draws, rep.undecided)
    for dims, method, mus, _ in cases.SIM_CASES:
        edges, ps, m = cases.sim_model(dims, mus)
        dens, rates = cases.sim_point(ps, m)
        rep = orc.simulate_events(dens, edges, rates, cases.SEED)
        pooled['sim %d %s' % (dims, method)] = (rep.draws, rep.undecided)
    report = ', '.join('%s: %d of %d' % (k, u, d) for k, (d, u) in pooled.items())
    for name, (d, u) in pooled.items():
        assert u <= orc.CAP * d, "undecided share of %s is %g; all: %s" % (name, u / d, report)
    print(report)


# ---- mutants -------------------------------------------------------------------------------------------------------------

def _caught(compare, dev, rep):
    with pytest.raises(AssertionError, match='mismatches'):
        compare(dev, rep)


B3 = [(B, s) for B, s in cases.PER_BIN_CASES if B == 3]


@pytest.mark.parametrize('mutant', ['odd01', 'attempt0', 'shift05', 'us13'])
def test_per_bin_mutants_are_caught_on_the_three_bin_case(mutant):
    """The smallest case with a pair and PTRS bins in it: B = 3, all shifts of the mu row, 8 toys each.  The honest device
    restatement passes; the mutant is rejected in at least one of the calls (each call is compared on its own)."""
    toys = np.arange(cases.T_PER_BIN)
    caught = 0
    for B, shift in B3:
        mu = cases.per_bin_mu(B, shift)
        rep = orc.per_bin_toys(mu, cases.SEED, toys)
        orc.compare_toys(rep.counts, rep)
        bad = orc.per_bin_toys(mu, cases.SEED, toys, mutant=mutant).counts
        try:
            orc.compare_toys(bad, rep)
        except AssertionError as err:
            assert 'mismatches' in str(err)
            caught += 1
    assert caught >= 1, mutant


def test_truncated_dataset_word_is_caught_at_the_offset_seam():
    off, T = cases.OFFSETS[0]
    toys = np.arange(off, off + T, dtype=np.uint64)
    mu = cases.per_bin_mu(3, 3)
    rep = orc.per_bin_toys(mu, cases.SEED, toys)
    _caught(orc.compare_toys, orc.per_bin_toys(mu, cases.SEED, toys, mutant='trunc32').counts, rep)
    mu = cases.event_mu(4096, 2.5)
    rep = orc.event_toys(mu, cases.SEED, toys)
    _caught(orc.compare_toys, orc.event_toys(mu, cases.SEED, toys, mutant='trunc32').counts, rep)


def test_event_path_mutants_are_caught():
    """pad_count on the smallest power-of-two case (B = 4096, M = 2.5); rle_drop on the smallest case in which a run crosses a
    thread's segment (B = 4096, M = 9.999: with 2.5 expected events no run of the six toys does); bisect_lt differs from the
    rule only where u M ties with a running sum exactly, which no 53-bit uniform of any case does (and which would lie inside
    the band): shown on a crafted uniform, u = 0 on the leading plateau, caught by 'no event where mu = 0', the one assertion
    that covers undecided draws as well."""
    toys = np.arange(6)
    mu = cases.event_mu(4096, 2.5)
    rep = orc.event_toys(mu, cases.SEED, toys)
    orc.compare_toys(rep.counts, rep)
    _caught(orc.compare_toys, orc.event_toys(mu, cases.SEED, toys, mutant='pad_count').counts, rep)
    mu = cases.event_mu(4096, 9.999)
    rep = orc.event_toys(mu, cases.SEED, toys)
    _caught(orc.compare_toys, orc.event_toys(mu, cases.SEED, toys, mutant='rle_drop').counts, rep)
    mu = cases.event_mu(4096, 10.0)
    honest = orc.event_toys(mu, cases.SEED, toys, forced_u={0: 0.0})
    assert np.all(honest.counts[:, mu == 0] == 0) and honest.undecided >= 1
    _caught(orc.compare_toys, orc.event_toys(mu, cases.SEED, toys, mutant='bisect_lt', forced_u={0: 0.0}).counts, honest)
    same = orc.event_toys(mu, cases.SEED, toys, mutant='bisect_lt')
    np.testing.assert_array_equal(same.counts, orc.event_toys(mu, cases.SEED, toys).counts)


def test_swapped_axes_are_caught_in_two_dimensions():
    dims, method, mus, _ = cases.SIM_CASES[2]
    edges, ps, m = cases.sim_model(dims, mus)
    dens, rates = cases.sim_point(ps, m)
    rep = orc.simulate_events(dens, edges, rates, cases.SEED)
    assert rep.n[2] > 100 and rep.n[0] == 0
    orc.compare_events(rep.n, rep.coords, rep.source, rep)
    bad = orc.simulate_events(dens, edges, rates, cases.SEED, mutant='axes_swapped')
    with pytest.raises(AssertionError, match='mismatches'):
        orc.compare_events(bad.n, bad.coords, bad.source, rep)
    # no event of the oracle lies where the pmf is zero
    assert np.all(dens[rep.source, rep.bin] > 0)
