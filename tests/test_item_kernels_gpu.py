"""The chunked tile walk of the per-point item kernels (csrc/bi_k_item.h: ItemTiles) in the kernels whose own test files
never reach it: k_morph_real (bi_eval_real), k_morph_gof (bi_eval_gof) and k_morph_bbgrad (bi_eval_grad with a
Beeston-Barlow source).  k_morph_hess and k_morph_fisher have theirs (test_derivatives_exact_gpu.py, test_fisher_gpu.py),
k_morph_sets never chunks.

One long row of B = 193 * 512 - 100 bins = 193 tiles with tile_chunks 3: 193 >= 64 * 3, so the walk runs in 3 regions of 65
tiles, the last one two tiles short (steps that are past the end) and the last tile 100 bins short; S = 2 sources on one axis
of two anchors, two points per call (a point inside the cell and one on the upper anchor), tile_chunks 1 and 3, nontemporal
loads off and on.  Every result is held to the oracle and the per-entry bound of the kernel's own test file, imported from
there; model, data and the slower oracles are computed once and shared by the four geometries."""
import numpy as np
import pytest

import derivative_oracle as do
import real_counts_oracle as rco
import test_gof_gpu as gof
import test_real_counts_gpu as real
from fisher_fixtures import synthetic_model
from test_derivatives_exact_gpu import ctx_of, synth

pytestmark = pytest.mark.gpu

B = 193 * 512 - 100
GEOMETRIES = [(chunks, nt) for chunks in (1, 3) for nt in (0, 1)]
ZS = np.array([[0.3], [1.0]])


@pytest.fixture(scope='module')
def dense_case():
    """the model (about 1.6 events expected per bin), two points, Poisson counts and real-valued counts, a dataset per point"""
    rng = np.random.default_rng(193)
    model = synthetic_model(rng, 1, 2, B, anchors=(-1.0, 1.0), holes=False)
    model = dict(model, mus=model['mus'] * 2000.0)
    rs = rng.uniform(0.4, 1.6, size=(2, 2))
    mu = rco.expectation(model, [0.2], np.full(2, 1.1))
    counts = rng.poisson(np.stack([mu, 0.3 * mu])).astype(float)
    real_counts = np.stack([mu, 0.3 * rco.expectation(model, [0.0], np.ones(2))])
    assert (B + 511) // 512 == 193 and np.count_nonzero(counts[0]) > B // 2
    return model, rs, counts, real_counts, np.arange(2)


def test_real_counts_on_a_chunked_walk(dense_case):
    model, rs, _, counts, ds = dense_case
    wants = [rco.point(model, counts[ds[p]], ZS[p], rs[p]) for p in range(2)]
    assert all(w['status'] == 0 and np.isfinite(w['half_deviance']) and w['half_deviance'] > 0 for w in wants)
    ctx = real.context_of(model)
    try:
        ctx.set_real_counts(counts)
        for chunks, nt in GEOMETRIES:
            ctx.set_param('tile_chunks', chunks)
            ctx.set_param('nt_loads', nt)
            what = 'k_morph_real, tile_chunks %d, nt_loads %d' % (chunks, nt)
            real.check_against_oracle(ctx.eval_real(ZS, rs, ds), wants, what)
            real.check_against_oracle(ctx.eval_real(ZS, rs, ds, gradient=False), wants, what + ', value only', gradient=False)
    finally:
        ctx.close()


def test_goodness_of_fit_on_a_chunked_walk(dense_case):
    model, rs, counts, _, ds = dense_case
    ctx = gof.context_of(model, counts, 0)
    try:
        for chunks, nt in GEOMETRIES:
            ctx.set_param('tile_chunks', chunks)
            ctx.set_param('nt_loads', nt)
            got = ctx.eval_gof(ZS, rs, ds)
            assert not got[2].any() and np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
            gof.check_against_oracle(got, model, counts, ZS, rs, ds, what='k_morph_gof, tile_chunks %d, nt_loads %d' % (chunks, nt))
    finally:
        ctx.close()


def test_beeston_barlow_gradient_on_a_chunked_walk():
    m = synth(2, (2,), (B,), bb_source=0)
    counts = m.counts(dense=True)
    zs, rs = m.random_points(1, seed=2)
    zs = np.concatenate([zs, [[m.anchor_z[0][-1]]]])
    rs = np.concatenate([rs, [[0.9, 1.2]]])
    model = m.dense_model()
    wants = [do.bb_gradient(model, zs[p], rs[p], counts, 0) for p in range(2)]
    for chunks, nt in GEOMETRIES:
        ctx = ctx_of(m, counts, tile_chunks=chunks, nt_loads=nt)
        try:
            ll, gz, gs, st = ctx.eval_grad(zs, rs)
            g = np.concatenate([gz, gs], axis=1)
            for p, o in enumerate(wants):
                what = 'k_morph_bbgrad, tile_chunks %d, nt_loads %d, point %d' % (chunks, nt, p)
                assert st[p] & ~4 == 0 and np.isfinite(ll[p]), what           # (4: the first-root flag, as check_grad masks it)
                worst = max(do.check_entries(ll[p], o['ll'], o['ll_cond'], what=what + ' ll'),
                            do.check_entries(g[p], o['grad'], o['grad_cond'], what=what + ' grad'))
                print('%s: worst |err| / (2^-52 cond) = %.3g (C = %d)' % (what, worst, do.C_POISSON))
        finally:
            ctx.close()
