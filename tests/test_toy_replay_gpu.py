"""The device toy generators replayed draw for draw against the exact oracle of their streams (tests/toy_oracle.py, written
from the stream definitions in include/blueice_hip.h): bi_generate_toys bin by bin and event by event, bi_simulate_events.
The inputs are those of tests/toy_replay_cases.py; tests/test_toy_oracle.py holds the oracle itself to account on the CPU.
Every comparison prints (draws, undecided) of its case; the oracle's bands and the cap on undecided draws are in toy_oracle."""
import mpmath as mp
import numpy as np
import pytest

import toy_oracle as orc
import toy_replay_cases as cases

pytestmark = pytest.mark.gpu


def make_ctx(mu, rate):
    """d = 0, one source: p = mu / rate (exact: rate is a power of two), expected events `rate`."""
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.upload_model([], (np.asarray(mu) / rate)[None, :], np.array([rate]))
    return ctx


def want_ll(mu, n):
    """sum_b n log mu - mu - lgamma(n + 1), the data-only term by mpmath"""
    live = n > 0
    lg = mp.fsum(mp.loggamma(int(v) + 1) for v in n[live])
    return float(mp.fsum(mp.mpf(float(v)) * mp.log(mp.mpf(float(m))) for v, m in zip(n[live], mu[live])) - mp.fsum(mp.mpf(float(m)) for m in mu) - lg)


def replay_call(ctx, mu, T, seed, offset=0, toys=None, path=0, what='', check_ll=True):
    """One bi_generate_toys call, its toys `toys` (numbers within the call; default all) against the oracle -> their counts."""
    ctx.set_param('toy_offset', offset)
    ctx.generate_toys(None, None, T, seed=seed)
    ctx.set_param('toy_offset', 0)
    assert ctx.get_param('last_toy_method') == path, what
    toys = np.arange(T) if toys is None else np.asarray(toys)
    dev = np.stack([ctx.download_counts(int(t)) for t in toys])
    numbers = (np.uint64(offset) + toys.astype(np.uint64))
    rep = (orc.event_toys if path else orc.per_bin_toys)(mu, seed, numbers)
    draws, undecided, _ = orc.compare_toys(dev, rep, what)
    print('%s: %d draws, %d undecided' % (what, draws, undecided))
    if len(toys) == T and not rep.und_toy.any():
        assert ctx.get_param('nnz_total') == int(np.count_nonzero(rep.counts)), what
    if not check_ll:            # (the row of stream A reaches mu = 2^20: n log mu ~ 10^7 there, whose ulp alone passes 1e-10 |ll|)
        return dev
    ll, st = ctx.eval_datasets(None, None)
    assert st == 0
    for i, t in enumerate(toys):
        if not rep.und_toy[i] and np.all(mu[rep.counts[i] > 0] > 0):
            want = want_ll(mu, rep.counts[i])
            assert abs(ll[t] - want) <= 1e-10 * abs(want), (what, int(t), ll[t], want)
    return dev


@pytest.mark.parametrize('B', sorted({B for B, _ in cases.PER_BIN_CASES}))
def test_per_bin_stream_is_the_oracles(B):
    """Bin counts around the block size of the count / scatter kernels (odd ones end in half a pair), every shift of the mu
    row: both samplers, the switch at mu = 10 to the ulp, mu = 0, 2^-1000 and 2^20, pairs of which one, both or neither take
    PTRS."""
    for _, shift in [c for c in cases.PER_BIN_CASES if c[0] == B]:
        mu = cases.per_bin_mu(B, shift)
        ctx = make_ctx(mu, cases.RATE_A)
        try:
            ctx.set_param('toy_events', 0)
            replay_call(ctx, mu, cases.T_PER_BIN, cases.SEED, what='A B=%d shift=%d' % (B, shift), check_ll=False)
        finally:
            ctx.close()


def test_per_bin_stream_seams_offsets_and_seeds():
    """The launch-chunk seam at 32 768 toys, the same toys through toy_offset, the dataset words at 2^32 and 2^47, and seeds
    around 2^32 and 2^64."""
    s = cases.SEAM_A
    mu = cases.per_bin_mu(s['B'], 0)
    ctx = make_ctx(mu, cases.RATE_A)
    try:
        toys = np.arange(s['first'], s['T'])
        joint = replay_call(ctx, mu, s['T'], cases.SEED, toys=toys, what='A seam', check_ll=False)
        apart = replay_call(ctx, mu, len(toys), cases.SEED, offset=s['first'], what='A seam by toy_offset', check_ll=False)
        np.testing.assert_array_equal(apart, joint)
        for offset, T in cases.OFFSETS:
            replay_call(ctx, mu, T, cases.SEED, offset=offset, what='A toy_offset=%d' % offset, check_ll=False)
        for seed in cases.SEEDS:
            replay_call(ctx, mu, 4, seed, what='A seed=%d' % seed, check_ll=False)
    finally:
        ctx.close()


@pytest.mark.parametrize('B,M,T,path', cases.EVENT_CASES)
def test_event_stream_is_the_oracles(B, M, T, path):
    """Key widths of 12, 13, 16 and 17 bits (odd and even numbers of radix passes), pads that tie with the busy last bin at a
    power-of-two B, zero plateaus at the start and before the busy bin, runs of half the events; N from inversion, at the
    sampler switch, straddling 1024 and 2048 within one launch, the bitonic sort, and the fall-back to one draw per bin."""
    mu = cases.event_mu(B, M)
    ctx = make_ctx(mu, cases.RATE_B)
    try:
        ctx.set_param('sparse', 1)
        replay_call(ctx, mu, T, cases.SEED, path=path, what='B B=%d M=%g' % (B, M))
    finally:
        ctx.close()


def test_event_stream_seams_offsets_and_seeds():
    s = cases.SEAM_B
    mu = cases.event_mu(s['B'], s['M'])
    ctx = make_ctx(mu, cases.RATE_B)
    try:
        ctx.set_param('sparse', 1)
        toys = np.arange(s['first'], s['T'])
        joint = replay_call(ctx, mu, s['T'], cases.SEED, toys=toys, path=1, what='B seam')
        apart = replay_call(ctx, mu, len(toys), cases.SEED, offset=s['first'], path=1, what='B seam by toy_offset')
        np.testing.assert_array_equal(apart, joint)
        for offset, T in cases.OFFSETS:
            replay_call(ctx, mu, T, cases.SEED, offset=offset, path=1, what='B toy_offset=%d' % offset)
        for seed in cases.SEEDS:
            replay_call(ctx, mu, 6, seed, path=1, what='B seed=%d' % seed)
    finally:
        ctx.close()


@pytest.mark.parametrize('path', [0, 1])
def test_morphed_point_of_mini3(path):
    """Several corners and sources: the device's mu differs from the oracle's in the last bits, which is what the bands are for."""
    from blueice_amd.device import DeviceContext
    from blueice_amd.synthetic import SyntheticModel
    from oracle import blueice_oracle as ref
    m = SyntheticModel.named('mini3')
    z, r = m.default_point()
    r = r * (0.02 if path else 1.0)
    dense = m.dense_model()
    ps = ref.interpolate(dense['anchor_z'], dense['ps'], z).reshape(m.S, m.B)
    mu = (ref.rates_at(dense, z, r)[:, None] * ps).sum(axis=0)
    ctx = DeviceContext(0)
    try:
        m.upload(ctx)
        ctx.set_param('sparse', 1)
        ctx.set_param('toy_events', path)
        T = 6
        ctx.generate_toys(z, r, T, seed=cases.SEED)
        assert ctx.get_param('last_toy_method') == path
        dev = np.stack([ctx.download_counts(t) for t in range(T)])
        rep = (orc.event_toys if path else orc.per_bin_toys)(mu, cases.SEED, np.arange(T))
        draws, undecided, _ = orc.compare_toys(dev, rep, 'mini3 path %d' % path)
        print('mini3 path %d: %d draws, %d undecided' % (path, draws, undecided))
    finally:
        ctx.close()


@pytest.mark.parametrize('dims,method,mus,score_sorted', cases.SIM_CASES)
def test_simulated_events_are_the_oracles(dims, method, mus, score_sorted):
    """Every event of bi_simulate_events: its source, its bin and its position on every axis, in drawn order -- with
    score_sorted on and 4096 events or more as well; per-source counts once from inversion, once from PTRS, once 0."""
    from blueice_amd.device import DeviceContext
    edges, ps, anchor_mus = cases.sim_model(dims, mus)
    dens, rates = cases.sim_point(ps, anchor_mus)
    tp, ctx = DeviceContext(0), DeviceContext(0)
    try:
        tp.upload_model([cases.SIM_ANCHORS], ps, anchor_mus)
        ctx.set_param('score_sorted', score_sorted)
        n = tp.simulate_events(ctx, method, edges, [cases.SIM_Z], None, seed=cases.SEED)
        coords, source = ctx.download_events()
        rep = orc.simulate_events(dens, edges, rates, cases.SEED)
        if max(mus) > 4096:
            assert n.sum() >= 4096 and ctx.get_param('events_sorted') == score_sorted
        what = 'sim %d %s' % (dims, method)
        draws, undecided, _ = orc.compare_events(n, coords, source, rep, what)
        print('%s: %d draws, %d undecided' % (what, draws, undecided))
        assert sorted(n > 0) == [False, True, True]
    finally:
        tp.close()
        ctx.close()


def test_event_simulation_refuses_rates_the_count_cannot_hold():
    """N_s travels through the samplers as a 32-bit int: 2^30 expected events per source and more are refused, by name."""
    from blueice_amd.device import DeviceContext
    edges, ps, anchor_mus = cases.sim_model(1, (3.0, 400.0, 0.0))
    tp, ctx = DeviceContext(0), DeviceContext(0)
    try:
        tp.upload_model([cases.SIM_ANCHORS], ps, anchor_mus)
        with pytest.raises(ValueError, match='2\\^30 expected events per source'):
            tp.simulate_events(ctx, 'piecewise', edges, [cases.SIM_Z], [1.0, 2.0 ** 31 / 400.0, 1.0], seed=1)
        n = tp.simulate_events(ctx, 'piecewise', edges, [cases.SIM_Z], [1.0, 1.0, 1.0], seed=1)
        assert n[2] == 0 and n[1] > 200
    finally:
        tp.close()
        ctx.close()
