"""bi_generate_toys_points: T toys at H truth points in one call, held to the exact oracle of the streams (tests/toy_oracle.py)
and to the single-truth calls whose toys they must be bit for bit.  Inputs: tests/toy_truth_cases.py."""
import numpy as np
import pytest

import toy_oracle as orc
import toy_replay_cases as cases
import toy_truth_cases as tc
from test_toy_replay_gpu import make_ctx, want_ll

pytestmark = pytest.mark.gpu


def counts_of(ctx, toys):
    return np.stack([ctx.download_counts(int(t)) for t in toys])


def separate_calls(ctx, scales, n_toys, seed, offset=0):
    """The same ensemble by one generate_toys per truth, toy_offset advanced -> counts [T, B] in toy order"""
    out = []
    for scale, n, first in zip(scales, n_toys, tc.first_toys(n_toys)):
        if n == 0:
            continue
        ctx.set_param('toy_offset', offset + first)
        ctx.generate_toys(None, None if scale is None else [scale], n, seed=seed)
        out.append(counts_of(ctx, range(n)))
    ctx.set_param('toy_offset', 0)
    return np.concatenate(out)


def against_oracle(dev, mu, scales, n_toys, methods, offset, what, toys_of=None):
    """Every truth's toys against the oracle of its method -> the oracle's counts [T, B] (None where a draw is undecided)"""
    want = np.zeros_like(dev)
    decided = True
    for h, (scale, n, first) in enumerate(zip(scales, n_toys, tc.first_toys(n_toys))):
        if n == 0:
            continue
        toys = np.arange(first, first + n) if toys_of is None else toys_of(h, first, n)
        if len(toys) == 0:
            continue
        numbers = np.uint64(offset) + toys.astype(np.uint64)
        rep = (orc.event_toys if methods[h] == 1 else orc.per_bin_toys)(mu * scale, tc.SEED, numbers)
        draws, undecided, _ = orc.compare_toys(dev[toys], rep, '%s truth %d' % (what, h))
        print('%s truth %d: %d draws, %d undecided' % (what, h, draws, undecided))
        want[toys] = rep.counts
        decided = decided and not rep.und_toy.any()
    return want if decided else None


@pytest.mark.parametrize('B', tc.A_BINS)
def test_per_bin_stream_at_mixed_truths(B):
    mu = cases.per_bin_mu(B, 0)
    T = sum(tc.A_N_TOYS)
    ctx = make_ctx(mu, cases.RATE_A)
    try:
        ctx.set_param('toy_events', 0)
        for offset in tc.A_OFFSETS:
            ctx.set_param('toy_offset', offset)
            methods = ctx.generate_toys_points(None, np.array(tc.A_SCALES)[:, None], tc.A_N_TOYS, seed=tc.SEED)
            ctx.set_param('toy_offset', 0)
            np.testing.assert_array_equal(methods, [0, -1, 0, 0])
            assert ctx.T == T and ctx.get_param('last_toy_method') == 0
            dev = counts_of(ctx, range(T))
            against_oracle(dev, mu, tc.A_SCALES, tc.A_N_TOYS, methods, offset, 'A B=%d offset=%d' % (B, offset))
            np.testing.assert_array_equal(dev, separate_calls(ctx, tc.A_SCALES, tc.A_N_TOYS, tc.SEED, offset))
    finally:
        ctx.close()


@pytest.mark.parametrize('B', tc.B_BINS)
def test_event_stream_at_mixed_truths(B):
    mu = cases.event_mu(B, tc.B_M)
    T = sum(tc.B_N_TOYS)
    ctx = make_ctx(mu, cases.RATE_B)
    try:
        ctx.set_param('sparse', 1)
        methods = ctx.generate_toys_points(None, np.array(tc.B_SCALES)[:, None], tc.B_N_TOYS, seed=tc.SEED)
        np.testing.assert_array_equal(methods, [1, 1, 1])
        assert ctx.get_param('last_toy_method') == 1
        dev = counts_of(ctx, range(T))
        want = against_oracle(dev, mu, tc.B_SCALES, tc.B_N_TOYS, methods, 0, 'B B=%d' % B)
        if want is not None:
            assert ctx.get_param('nnz_total') == int(np.count_nonzero(want))
        # the data-only likelihood of every toy at the context's own point (scale 1), as the replay checks it
        ll, st = ctx.eval_datasets(None, None)
        assert st == 0
        if want is not None:
            for t in range(T):
                w = want_ll(mu, want[t])
                assert abs(ll[t] - w) <= 1e-10 * abs(w), (t, ll[t], w)
        np.testing.assert_array_equal(dev, separate_calls(ctx, tc.B_SCALES, tc.B_N_TOYS, tc.SEED))
    finally:
        ctx.close()


def test_both_methods_in_one_call():
    mu = cases.event_mu(tc.MIX_B, tc.MIX_M)
    T = sum(tc.MIX_N_TOYS)
    ctx = make_ctx(mu, cases.RATE_B)
    try:
        ctx.set_param('sparse', 1)
        methods = ctx.generate_toys_points(None, np.array(tc.MIX_SCALES)[:, None], tc.MIX_N_TOYS, seed=tc.SEED)
        np.testing.assert_array_equal(methods, tc.MIX_METHODS)
        assert ctx.get_param('last_toy_method') == 0
        dev = counts_of(ctx, range(T))
        want = against_oracle(dev, mu, tc.MIX_SCALES, tc.MIX_N_TOYS, methods, 0, 'mixed')
        assert want is not None, 'the oracle decides every draw of this case'
        assert ctx.get_param('nnz_total') == int(np.count_nonzero(want))
        ll, st = ctx.eval_datasets(None, None)
        assert st == 0
        for t in range(T):
            w = want_ll(mu, want[t])
            assert abs(ll[t] - w) <= 1e-10 * abs(w), (t, ll[t], w)
        np.testing.assert_array_equal(dev, separate_calls(ctx, tc.MIX_SCALES, tc.MIX_N_TOYS, tc.SEED))
    finally:
        ctx.close()


def test_truth_boundary_next_to_the_launch_chunk_seam():
    mu = cases.per_bin_mu(tc.SEAM_B_BINS, 0)
    T = sum(tc.SEAM_N_TOYS)
    first = cases.SEAM_A['first']
    ctx = make_ctx(mu, cases.RATE_A)
    try:
        methods = ctx.generate_toys_points(None, np.array(tc.SEAM_SCALES)[:, None], tc.SEAM_N_TOYS, seed=tc.SEED)
        np.testing.assert_array_equal(methods, [0, 0])
        assert ctx.T == T
        toys = np.arange(first, T)
        dev = np.zeros((T, tc.SEAM_B_BINS))
        dev[toys] = counts_of(ctx, toys)

        def last(h, first_h, n):
            return toys[(toys >= first_h) & (toys < first_h + n)]
        against_oracle(dev, mu, tc.SEAM_SCALES, tc.SEAM_N_TOYS, methods, 0, 'A seam', toys_of=last)
    finally:
        ctx.close()


@pytest.mark.parametrize('path', [0, 1])
def test_morphed_truths_of_mini3(path):
    """Two truths in different grid cells and one on an anchor: the lists are those of the per-truth calls, exactly."""
    from blueice_amd.device import DeviceContext
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel.named('mini3')
    z0, r = m.default_point()
    r = r * (0.02 if path else 1.0)
    grid = [np.asarray(g, dtype=float) for g in m.anchor_z]
    z_low = np.array([0.75 * g[0] + 0.25 * g[1] for g in grid])
    z_high = np.array([0.25 * g[-2] + 0.75 * g[-1] for g in grid])
    z_anchor = np.array([g[1] for g in grid])
    zs = np.stack([z_low, z_high, z_anchor])
    scales = np.stack([r, 0.5 * r, r])
    n_toys = (2, 2, 2)
    ctx = DeviceContext(0)
    try:
        m.upload(ctx)
        ctx.set_param('sparse', 1)
        ctx.set_param('toy_events', path)
        methods = ctx.generate_toys_points(zs, scales, n_toys, seed=tc.SEED)
        np.testing.assert_array_equal(methods, [path] * 3)
        assert ctx.get_param('last_toy_method') == path
        dev = counts_of(ctx, range(6))
        nnz = ctx.get_param('nnz_total')
        apart, nnz_apart = [], 0
        for h in range(3):
            ctx.set_param('toy_offset', 2 * h)
            ctx.generate_toys(zs[h], scales[h], 2, seed=tc.SEED)
            assert ctx.get_param('last_toy_method') == path
            apart.append(counts_of(ctx, range(2)))
            nnz_apart += ctx.get_param('nnz_total')
        ctx.set_param('toy_offset', 0)
        np.testing.assert_array_equal(dev, np.concatenate(apart))
        assert nnz == nnz_apart
        assert len({dev[2 * h].tobytes() for h in range(3)}) == 3
    finally:
        ctx.close()


def test_refusals_leave_the_resident_toys_usable():
    from blueice_amd.device import DeviceContext
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel.named('mini3')
    z0, r = m.default_point()
    grid = [np.asarray(g, dtype=float) for g in m.anchor_z]
    outside = np.array(z0, dtype=float).copy()
    outside[0] = grid[0][-1] + 1.0
    ctx = DeviceContext(0)
    try:
        m.upload(ctx)
        ctx.generate_toys(z0, r, 3, seed=tc.SEED)
        before, st = ctx.eval_datasets(z0, r)
        with pytest.raises(ValueError, match='truth 1'):
            ctx.generate_toys_points(np.stack([z0, outside, z0]), None, (1, 1, 1), seed=tc.SEED)
        with pytest.raises(ValueError):
            ctx.generate_toys_points(np.stack([z0, z0]), None, (0, 0), seed=tc.SEED)
        with pytest.raises(ValueError):
            ctx.generate_toys_points(np.stack([z0, z0]), None, (2, -1), seed=tc.SEED)
        after, st2 = ctx.eval_datasets(z0, r)
        assert ctx.T == 3
        np.testing.assert_array_equal(after, before)
        np.testing.assert_array_equal(st2, st)
    finally:
        ctx.close()
