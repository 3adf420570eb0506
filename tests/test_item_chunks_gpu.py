"""The one-work-item-per-point paths across the 65 535-item launch chunk: bi_eval_gof, bi_eval_real (values only and with
the gradient) and the host route of bi_eval_grad (dense rows and compacted non-empty bins) at P = 65 538 with two dead
points, so that live index and point index differ on both sides of the seam.

The model has B = 96 bins: every item is one tile, run_item_chunks gives every item one block whatever the batch, and a
point's sums are taken in the same order in every batch.  The points around the dead ones and around the seam are therefore
held, bit for bit, to the same points evaluated in a batch of their own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 65538
OUTSIDE, UNPHYSICAL = 3, 65534                     # the dead points: z outside the anchor box, a negative rate scale
PROBES = np.array([0, 2, 4, 65533, 65535, 65536, 65537])
ST_OUT_OF_BOUNDS, ST_UNPHYSICAL = 1, 2
D, S, B, T, T_REAL = 1, 2, 96, 3, 2


@pytest.fixture(scope='module')
def case():
    rng = np.random.default_rng(65538)
    anchor_z = [np.array([-1.0, 0.0, 1.0])]
    ps = rng.uniform(0.2, 1.0, size=(3, S, B))
    ps /= ps.sum(axis=-1, keepdims=True)
    mus = rng.uniform(20.0, 60.0, size=(3, S))
    # mostly empty datasets (at most 20 of 96 bins filled): `sparse = 1` then takes the compacted non-empty bins
    counts = np.zeros((T, B))
    for t in range(T):
        filled = rng.choice(B, size=20, replace=False)
        counts[t, filled] = rng.poisson(3.0, size=20)
    real = rng.uniform(0.0, 2.5, size=(T_REAL, B))
    z = rng.uniform(-1.0, 1.0, size=(P, D))
    rs = rng.uniform(0.5, 1.5, size=(P, S))
    z[OUTSIDE, 0] = 1.5
    rs[UNPHYSICAL, 0] = -1.0
    return dict(anchor_z=anchor_z, ps=ps, mus=mus, counts=counts, real=real, z=z, rs=rs, ds=rng.integers(0, T, size=P),
                ds_real=rng.integers(0, T_REAL, size=P))


def context_of(case, sparse):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', sparse)                 # (before the counts: the non-empty-bin forms are made at upload)
    ctx.upload_model(case['anchor_z'], case['ps'], case['mus'])
    ctx.upload_counts(case['counts'])
    ctx.set_real_counts(case['real'])
    assert ctx.get_param('compact_ready') == (1 if sparse else 0)
    return ctx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(what, evaluate, case, ds, dead_value):
    """evaluate(z, rs, ds) -> (list of float arrays [P, ...], status [P]): the whole batch against the probes alone, the dead
    points' defaults (dead_value in the first array, nan in the others) and every status word"""
    full, st = evaluate(case['z'], case['rs'], ds)
    alone, st_alone = evaluate(case['z'][PROBES], case['rs'][PROBES], ds[PROBES])
    assert not st_alone.any()
    for k, (a, b) in enumerate(zip(full, alone)):
        np.testing.assert_array_equal(bits(a[PROBES]), bits(b), err_msg='%s, output %d at the probes' % (what, k))
        assert np.all(np.isfinite(b)), '%s, output %d: the probes are live points' % (what, k)
    want_st = np.zeros(P, dtype=np.int32)
    want_st[OUTSIDE], want_st[UNPHYSICAL] = ST_OUT_OF_BOUNDS, ST_UNPHYSICAL
    np.testing.assert_array_equal(st, want_st, err_msg=what + ': status')
    for p in (OUTSIDE, UNPHYSICAL):
        assert np.all(full[0][p] == dead_value), '%s: point %d has %r' % (what, p, full[0][p])
        for a in full[1:]:
            assert np.all(np.isnan(a[p])), '%s: point %d has %r' % (what, p, a[p])


def test_gof_and_real_counts_across_the_launch_chunk(case):
    ctx = context_of(case, 0)
    try:
        def gof(z, rs, ds):
            half, pearson, st = ctx.eval_gof(z, rs, ds)
            return [np.stack([half, pearson], axis=1)], st            # (both statistics are +inf at a dead point)

        def real(z, rs, ds):
            half, gz, gs, st = ctx.eval_real(z, rs, ds)
            return [half, gz, gs], st

        def real_values(z, rs, ds):
            half, _, _, st = ctx.eval_real(z, rs, ds, gradient=False)
            return [half], st

        check('eval_gof', gof, case, case['ds'], np.inf)
        check('eval_real', real, case, case['ds_real'], np.inf)
        check('eval_real, values only', real_values, case, case['ds_real'], np.inf)
    finally:
        ctx.close()


@pytest.mark.parametrize('sparse', [0, 1])
def test_host_gradient_route_across_the_launch_chunk(case, sparse):
    ctx = context_of(case, sparse)
    plan_min = ctx.get_param('device_plan_min')
    try:
        ctx.set_param('device_plan_min', 0)            # the descriptors of every batch are made on the host

        def grad(z, rs, ds):
            ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
            return [ll, gz, gs], st

        check('eval_grad, sparse %d' % sparse, grad, case, case['ds'], -np.inf)
        assert ctx.get_param('last_morph_nbx') == 1 and ctx.get_param('last_morph_items') == len(PROBES)
    finally:
        ctx.set_param('device_plan_min', plan_min)
        ctx.close()
