"""An independent restatement of the ensemble sampler's random stream and half-step, written from the text of
include/blueice_hip.h (bi_sample_stretch) in plain Python integers and NumPy scalars -- nothing is imported from
blueice_amd/sampler.py -- and the replay check built on it.  Test infrastructure only."""
import math

import numpy as np

MASK = 0xFFFFFFFF
TAG = 0x53545200


def philox(counter, key):
    """Philox4x32-10: counter (c0, c1, c2, c3), key (k0, k1), Python ints -> four 32-bit words."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        a, b = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (b >> 32) ^ c1 ^ k0, b & MASK, (a >> 32) ^ c3 ^ k1, a & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def draw(seed, ensemble, W, t, h, k, a):
    """-> (partner j, stretch factor z, u_a) of moving walker k in half-step (t, h)"""
    r0, r1, r2, r3 = philox((k, ensemble, t, TAG | h), (seed & MASK, (seed >> 32) & MASK))
    u_z = np.float64((r0 >> 5) * 67108864 + (r1 >> 6)) * np.float64(2.0 ** -53)
    j = (1 - h) * (W // 2) + ((r2 * (W // 2)) >> 32)
    u_a = (np.float64(r3) + np.float64(0.5)) * np.float64(2.0 ** -32)
    g = (np.float64(a) - np.float64(1.0)) * u_z + np.float64(1.0)
    z = (g * g) / np.float64(a)
    return j, z, u_a


def proposal(x_k, x_j, z):
    s = x_k - x_j
    p = z * s
    return x_j + p


def replay(chain, log_prob, x0, ll_of, lo, hi, seed, a, ensemble=0, ll_rtol=1e-10, band_abs=2e-10, band_log=1e-12):
    """Replay every half-step of one ensemble from the sampler's OWN previous state.  chain [T, W, F], log_prob [T, W];
    ll_of(points [n, F]) -> the reference log density.  Asserts, per moving walker: the new position is bitwise the old one
    or the proposal; the recorded log density is the reference's at that position within ll_rtol max(1, |ll|); the decision
    is the reference's wherever q = (F - 1) log z + ll(y) - ll(x_k) - log u_a lies outside +-m,
    m = band_abs max(1, |ll(y)|, |ll(x_k)|) + band_log (F - 1) |log z|.  -> (decisions, decisions inside the band, accepted)."""
    T, W, F = chain.shape
    half = W // 2
    state = np.array(x0, dtype=float)
    ll_state = np.asarray(ll_of(state), dtype=float)
    assert np.all(np.isfinite(ll_state))
    n_dec = n_band = n_acc = 0
    for t in range(T):
        for h in (0, 1):
            ks = np.arange(h * half, (h + 1) * half)
            draws = [draw(seed, ensemble, W, t, h, int(k), a) for k in ks]
            ys = np.array([proposal(state[k], state[j], z) for k, (j, z, _) in zip(ks, draws)])
            inside = np.all((ys >= lo) & (ys <= hi), axis=1)
            ll_y = np.full(half, -np.inf)
            if inside.any():
                ll_y[inside] = ll_of(ys[inside])
            for i, k in enumerate(ks):
                j, z, u_a = draws[i]
                assert h * half <= k < (h + 1) * half and (1 - h) * half <= j < (2 - h) * half
                new = chain[t, k]
                moved = np.array_equal(new.view(np.uint64), ys[i].view(np.uint64))
                stayed = np.array_equal(new.view(np.uint64), state[k].view(np.uint64))
                assert moved or stayed, "step %d half %d walker %d: neither the old position nor the proposal" % (t, h, k)
                want_ll = ll_y[i] if (moved and not stayed) else ll_state[k]
                got_ll = log_prob[t, k]
                assert np.isfinite(got_ll) and abs(got_ll - want_ll) <= ll_rtol * max(1.0, abs(want_ll)), (t, h, k, got_ll, want_ll)
                n_dec += 1
                if np.isfinite(ll_y[i]):
                    logz = math.log(z)
                    q = (F - 1) * logz + ll_y[i] - ll_state[k] - math.log(u_a)
                    m = band_abs * max(1.0, abs(ll_y[i]), abs(ll_state[k])) + band_log * (F - 1) * abs(logz)
                    if q > m:
                        assert moved, "step %d half %d walker %d: q = %g > %g but the move was rejected" % (t, h, k, q, m)
                    elif q < -m:
                        assert stayed, "step %d half %d walker %d: q = %g < -%g but the move was accepted" % (t, h, k, q, m)
                    else:
                        n_band += 1
                else:
                    assert stayed, "step %d half %d walker %d: a proposal of zero likelihood was accepted" % (t, h, k)
                if moved and not stayed:
                    n_acc += 1
                    ll_state[k] = ll_y[i]
                state[k] = new
        # (walkers of the other half are untouched within a half-step: the chain row must say so as well)
        assert np.array_equal(state.view(np.uint64), chain[t].view(np.uint64))
    return n_dec, n_band, n_acc
