"""The free-variable map of the native loops (VarMap, bi_varmap.h): the grid, the sampler and the two fit drivers expand a point
from the same six arrays.  One small model where every part of the map can go wrong -- two entries with different z0, scale0 and
unit (none of them 1), datasets in the order [1, 0], three variables whose order interleaves the kinds and permutes the indices
-- and every loop's values against `ctx.eval` at rows expanded in NumPy from the definition:

    row = (z0[e], scale0[e]);  kind 0: z[index[j]] = y_j;  kind 1: rate_scale[index[j]] = y_j * unit[e][index[j]];  dataset[e]

The bound is the one tests/test_grid_gpu.py holds the native grid to against the host engine: 2e-10 max(1, |value|)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, S, B, T, E, F = 2, 3, 40, 2, 2, 3
ANCHORS = [np.array([-1.0, 0.0, 1.5]), np.array([0.0, 0.5, 2.0])]
KIND = np.array([1, 0, 1], dtype=np.int32)                   # rate of source 2, shape axis 1, rate of source 0
INDEX = np.array([2, 1, 0], dtype=np.int32)
Z0 = np.array([[-0.4, 0.3], [0.7, 1.2]])
SCALE0 = np.array([[0.9, 1.1, 1.3], [1.2, 0.8, 0.7]])
UNIT = np.array([[1.5, 0.6, 2.0], [0.5, 1.7, 1.25]])
DATASET = np.array([1, 0], dtype=np.int64)
LO, HI = np.array([0.0, 0.0, 0.0]), np.array([50.0, 2.0, 50.0])
BOUND = 2e-10


@pytest.fixture(scope='module')
def ctx():
    from blueice_amd.device import DeviceContext
    rng = np.random.default_rng(7)
    ps = rng.uniform(0.2, 1.0, (3, 3, S, B))
    ps /= ps.sum(axis=-1, keepdims=True)
    mus = rng.uniform(20.0, 60.0, (3, 3, S))
    counts = rng.poisson(4.0, (T, B)).astype(float)
    c = DeviceContext(0)
    c.upload_model(ANCHORS, ps, mus)
    c.upload_counts(counts)
    c.set_real_counts(counts + rng.uniform(0.1, 0.9, (T, B)))
    yield c
    c.close()


def expand(y, entry):
    """y [n, F] at entries entry [n] -> the rows (z [n, d], rate_scale [n, S], dataset [n]) of the definition"""
    z, rs = Z0[entry].copy(), SCALE0[entry].copy()
    for j in range(F):
        if KIND[j] == 0:
            z[:, INDEX[j]] = y[:, j]
        else:
            rs[:, INDEX[j]] = y[:, j] * UNIT[entry, INDEX[j]]
    return z, rs, DATASET[entry]


def assert_close(got, want):
    assert np.all(np.isfinite(want))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print('max error %.3g of the bound' % (err.max() / BOUND))
    assert np.all(err <= BOUND)


def test_grid(ctx):
    nodes = [np.array([0.5, 1.0, 1.6]), np.array([0.2, 1.4]), np.array([0.8, 1.3])]
    lm, profile, argmax, counters = ctx.grid_reduce(KIND, INDEX, Z0, SCALE0, UNIT, DATASET, F, nodes)
    assert profile.shape == (E, 12) and counters[1] == E * 12
    y = np.stack([m.ravel() for m in np.meshgrid(*nodes, indexing='ij')], axis=1)
    for e in range(E):
        want, st = ctx.eval(*expand(y, np.full(len(y), e)))
        assert not st.any()
        assert_close(profile[e], want)
    assert np.all(argmax == 0)                                 # n_keep = F: one point per cell


def test_sampler(ctx):
    W = 4
    x0 = np.random.default_rng(3).uniform(0.7, 1.3, (E, W, F))
    chain, ll, n_acc, _ = ctx.sample_stretch(W, KIND, INDEX, Z0, SCALE0, UNIT, DATASET, x0, LO, HI, 1, seed=17)
    stayed = n_acc == 0
    assert np.array_equal(chain[0][stayed], x0[stayed])
    entry = np.repeat(np.arange(E), W)
    # every walker's ll is the likelihood at where it stands: the start for those that stayed, the proposal for the others
    for at, which in ((x0, stayed.ravel()), (chain[0], ~stayed.ravel())):
        if which.any():
            want, st = ctx.eval(*expand(at.reshape(-1, F)[which], entry[which]))
            assert not st.any()
            assert_close(ll[0].ravel()[which], want)


@pytest.mark.parametrize('real', [False, True])
def test_fit(ctx, real):
    P = 2 * E
    entry = np.arange(P) % E
    x0 = np.ascontiguousarray(np.random.default_rng(5).uniform(0.8, 1.2, (P, F)))
    x, f = np.empty((P, F)), np.empty(P)
    flags, counters = np.zeros(P, dtype=np.int32), np.zeros(4, dtype=np.int64)
    fit = ctx.fit_batched_real if real else ctx.fit_batched
    fit(P, F, KIND, INDEX, np.ascontiguousarray(Z0[entry]), np.ascontiguousarray(SCALE0[entry]), np.ascontiguousarray(UNIT[entry]),
        np.ascontiguousarray(DATASET[entry]), x0, LO, HI, None, None, 1e-6, 3, x, f, flags, counters)
    assert counters[3] > 0 and not np.array_equal(x, x0)
    z, rs, ds = expand(x, entry)
    if real:
        want, _, _, st = ctx.eval_real(z, rs, ds, gradient=False)
    else:
        ll, st = ctx.eval(z, rs, ds)
        want = -ll
    assert not st.any()
    assert_close(f, want)                                      # wherever the optimiser stopped


@pytest.mark.parametrize('kind, index, j', [(np.array([2, 0, 1], dtype=np.int32), INDEX, 0), (KIND, np.array([2, 5, 0], dtype=np.int32), 1),
                                            (KIND, np.array([2, 1, -1], dtype=np.int32), 2), (KIND, np.array([3, 1, 0], dtype=np.int32), 0)])
def test_refusals(ctx, kind, index, j):
    """every entry point names itself (the *_gauss ones share the checks, and the name, of their plain forms)"""
    why = ': variable %d is neither a shape parameter nor a rate multiplier' % j
    priors = (np.zeros(F), np.full(F, 2.0), None)
    P = E
    x0 = np.ones((P, F))
    x, f, flags, counters = np.empty((P, F)), np.empty(P), np.zeros(P, dtype=np.int32), np.zeros(4, dtype=np.int64)
    fit_args = (P, F, kind, index, Z0, SCALE0, UNIT, DATASET, x0, LO, HI, None, None, 1e-6, 3, x, f, flags, counters)
    for who, call in (('bi_fit_batched', lambda: ctx.fit_batched(*fit_args)),
                      ('bi_fit_batched', lambda: ctx.fit_batched(*fit_args, priors=priors)),
                      ('bi_fit_batched_real', lambda: ctx.fit_batched_real(*fit_args)),
                      ('bi_sample_stretch', lambda: ctx.sample_stretch(4, kind, index, Z0, SCALE0, UNIT, DATASET, np.ones((E, 4, F)), LO, HI, 1)),
                      ('bi_sample_stretch', lambda: ctx.sample_stretch(4, kind, index, Z0, SCALE0, UNIT, DATASET, np.ones((E, 4, F)), LO, HI, 1,
                                                                       priors=priors)),
                      ('bi_grid_reduce', lambda: ctx.grid_reduce(kind, index, Z0, SCALE0, UNIT, DATASET, F, [np.ones(2)] * F))):
        with pytest.raises(ValueError, match='^' + who + why):
            call()
