"""The source-wise kernels at every launch geometry they can take, against the exact oracles: k_morph_factored, k_factored_curv
(observed and Fisher form, every Gram panel), k_sourcewise_gof and k_sourcewise_real under the chunked tile walk of ItemTiles
(193 tiles in three regions, the last two tiles short), with blocks that take a second tile (1025 tiles on fewer blocks, k_finish
adding every block's partial), with tiles behind a step past the end of a ragged last chunk (2177 tiles in 34 regions), and with
plain and nontemporal loads in every (source slots, own axes) class; k_sourcewise_expect with both load forms.  The models,
points and data are tests/sourcewise_walk_cases.py's (held to their claims on the CPU by tests/test_sourcewise_walk_cases.py).

This file defines no tolerance: every bound and checker is the entry point's own --
    eval, eval_grad          test_factored_gpu.check_points with factored_oracle.factored_derivatives
    eval_hess, eval_fisher   test_factored_curvature_gpu.check_curvature(..., expanded=False)
    eval_gof                 test_sourcewise_toys_gpu._gof_want on the expansion and its TOL
    expected_counts          derivative_oracle.check_entries against sourcewise_toy_cases.exact_expectation, cond = mu_b
    eval_real                sourcewise_real_oracle.want_point on the expansion, test_sourcewise_real_gpu.check_against_oracle
-- and every oracle is computed once and shared between the geometries.  Per geometry and entry point: every status word 0,
every entry within its bound, a values-only call gives the bits of the call with the gradient, eval_hess returns eval_grad's bits,
a repeated call gives the same bits, a point alone gives the bits it had in the batch of two, and nt_loads 0 and 1 give the same
bits of every output.  Different tile_chunks need not agree bit for bit (which block holds which tile changes the order in which
k_finish adds the partials): there the oracle alone decides.  The counters last_morph_nbx / last_morph_items say which grid a
launch of FacBatch::run took.  Run with -s for the worst |err| / bound per family and entry point."""
import numpy as np
import pytest

import factored_curvature_oracle as fc
import factored_oracle as fo
import sourcewise_real_oracle as sro
import sourcewise_toy_cases as toy_cases
import sourcewise_walk_cases as wc
import test_factored_curvature_gpu as curv
import test_factored_gpu as fac
import test_sourcewise_real_gpu as real
import test_sourcewise_toys_gpu as toys
from derivative_oracle import C_POISSON, check_entries

pytestmark = pytest.mark.gpu

WORST = {}
NBX = {}
_CASES, _WANT, _FULL = {}, {}, {}


def case_of(key):
    if key not in _CASES:
        _CASES[key] = wc.make_case(*key)
    return _CASES[key]


def full_of(key):
    """the expansion of one case at a time (up to about 100 MB)"""
    if key not in _FULL:
        _FULL.clear()
        _FULL[key] = fo.expand(case_of(key).model)
    return _FULL[key]


def want(key, kind, p):
    """the oracle of point p of a case, computed once"""
    if (key, kind, p) not in _WANT:
        c = case_of(key)
        z, rs = c.z[p], c.rs[p]
        if kind == 'grad':
            w = fo.factored_derivatives(c.model, z, rs, c.counts[c.ds[p]])
        elif kind == 'gof':
            w = toys._gof_want(full_of(key), c.counts[c.ds[p]], z, rs)
        elif kind == 'expect':
            w = toy_cases.exact_expectation(c.model, z, rs)
        else:
            assert kind == 'real'
            w = sro.want_point(c.model, full_of(key), c.real[c.ds[p]], z, rs)
        _WANT[(key, kind, p)] = w
    return _WANT[(key, kind, p)]


@pytest.fixture(scope='module', autouse=True)
def shared():
    """check_curvature computes its oracles itself: the factored specification answers a point it has seen from a table.  At the
    end: the figures of the run, and the cases released."""
    table = {}

    def once(f):
        def g(model, z, rs, *counts):
            # the models stay alive in _CASES, so id(model) names one; a point has one dataset, and the table says so if not
            k = (f.__name__, id(model), np.asarray(z).tobytes(), np.asarray(rs).tobytes())
            if k not in table:
                table[k] = (f(model, z, rs, *counts), model, [np.array(n, dtype=float) for n in counts])
            result, seen_model, seen_counts = table[k]
            assert seen_model is model and len(seen_counts) == len(counts)
            assert all(np.array_equal(a, b) for a, b in zip(seen_counts, counts)), 'the same point with other counts'
            return result
        return g

    mp = pytest.MonkeyPatch()
    mp.setattr(fc, 'curvature', once(fc.curvature))
    mp.setattr(fc, 'information', once(fc.information))
    yield
    mp.undo()
    print('\nworst |err| / bound per family and entry point:')
    for k in sorted(WORST):
        print('  %-12s %-28s %.3g' % (k + (WORST[k],)))
    for k in sorted(NBX):
        print('  %-12s %4d tiles: last_morph_nbx %s' % (k, wc.n_tiles(wc.bins_of(k)), sorted(NBX[k])))
    for d in (_CASES, _WANT, _FULL):
        d.clear()


def note(family, entry, ratio):
    WORST[(family, entry)] = max(WORST.get((family, entry), 0.0), float(ratio))


def upload(c):
    ctx = toy_cases.upload(c.model, c.counts)
    ctx.set_real_counts(c.real)
    return ctx


def settings(ctx, chunks, nt):
    ctx.set_param('tile_chunks', chunks)
    ctx.set_param('nt_loads', nt)


def grid_check(ctx, c, items):
    """the grid of the launch FacBatch::run made last: one block per tile on the 193-tile rows, fewer blocks than tiles (a block
    takes a second tile) on the 1025-tile rows -- read from the counters, no constant of the host restated"""
    nbx, n, fused = (ctx.get_param('last_morph_' + k) for k in ('nbx', 'items', 'fused'))
    NBX.setdefault(c.family, set()).add(nbx)
    assert n == items and fused == 0, (c.family, c.name, nbx, n, fused)
    if c.family == 'chunked':
        assert nbx == c.tiles == wc.CHUNKED_TILES, (c.name, nbx)
    elif c.family in ('striding', 'past_the_end'):
        assert 1 <= nbx < c.tiles and c.tiles in (wc.STRIDING_TILES, wc.PAST_TILES), (c.name, nbx)
    else:
        assert 1 <= nbx <= c.tiles, (c.name, nbx)


def same(a, b, what):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None, what
        else:
            np.testing.assert_array_equal(x, y, err_msg=what)


def stable(c, call, what, ctx=None):
    """call(sel) -> the outputs for the points `sel`.  A repeated call gives the same bits and every point alone the bits it has in
    the batch of two (the blocks of an item depend on the row length alone) -> the batch's outputs.  ctx: the call goes through
    FacBatch::run, whose grid is checked behind the batch and behind a single point."""
    first = call(slice(None))
    if ctx is not None:
        grid_check(ctx, c, 2)
    same(call(slice(None)), first, what + ', repeated')
    for p in range(2):
        alone = call(slice(p, p + 1))
        if ctx is not None:
            grid_check(ctx, c, 1)
        same([None if a is None else a[0] for a in alone], [None if b is None else b[p] for b in first], what + ', point %d alone' % p)
    return first


def across_loads(c, ctx, body):
    """body(what) -> outputs, at every (tile_chunks, nt_loads) of the family: nt_loads 0 and 1 of one tile_chunks give the same
    bits (only the cache policy differs); with the default nt_loads = 2 a single point takes the nontemporal form, a batch the
    plain one"""
    ref = {}
    for chunks, nt in wc.GEOMETRIES[c.family]:
        settings(ctx, chunks, nt)
        what = '%s %s, tile_chunks %d, nt_loads %d' % (c.family, c.name, chunks, nt)
        got = body(what)
        if chunks in ref:
            same(got, ref[chunks], what + ' against the other load form')
        else:
            ref[chunks] = got
    assert all(sorted(nt for ch, nt in wc.GEOMETRIES[c.family] if ch == chunks) == [0, 1] for chunks in ref)
    return ref


KEY_IDS = '-'.join


@pytest.mark.parametrize('key', wc.KEYS, ids=KEY_IDS)
def test_value_and_gradient(key):
    """k_morph_factored<SC, EM, GRAD, NT>, the four forms of the case's class: value and gradient of both points"""
    c = case_of(key)
    oracle = lambda z, rs, n: want(key, 'grad', 0 if np.array_equal(z, c.z[0]) else 1)         # noqa: E731
    ctx = upload(c)
    try:
        def body(what):
            note(c.family, 'eval, eval_grad', fac.check_points(ctx, c.model, c.z, c.rs, c.counts, oracle, what, dataset=c.ds) / C_POISSON)
            grad = stable(c, lambda s: ctx.eval_grad(c.z[s], c.rs[s], c.ds[s]), what + ', eval_grad', ctx)
            value = stable(c, lambda s: ctx.eval(c.z[s], c.rs[s], c.ds[s]), what + ', eval', ctx)
            assert not grad[3].any() and not value[1].any(), what
            np.testing.assert_array_equal(value[0], grad[0], err_msg=what + ': values only against the gradient call')
            return grad
        ref = across_loads(c, ctx, body)
        if c.family == 'load_forms':
            chunks = wc.GEOMETRIES[c.family][0][0]
            settings(ctx, chunks, 2)                        # the default: a single point takes the nontemporal form
            for p in range(2):
                s = slice(p, p + 1)
                alone = ctx.eval_grad(c.z[s], c.rs[s], c.ds[s])
                same([a[0] for a in alone], [b[p] for b in ref[chunks]], 'nt_loads 2, eval_grad, point %d' % p)
                assert ctx.eval(c.z[s], c.rs[s], c.ds[s])[0][0] == ref[chunks][0][p]
    finally:
        ctx.close()


@pytest.mark.parametrize('key', wc.FULL_KEYS, ids=KEY_IDS)
def test_goodness_of_fit(key):
    """k_sourcewise_gof<SC, EM, NT>: half-deviance and Pearson chi2 against the long-double statistics of the expansion"""
    c = case_of(key)
    ctx = upload(c)
    try:
        def body(what):
            half, pearson, st = got = stable(c, lambda s: ctx.eval_gof(c.z[s], c.rs[s], c.ds[s]), what + ', eval_gof', ctx)
            assert not st.any(), what
            for p in range(2):
                for g, w, name in zip((half[p], pearson[p]), want(key, 'gof', p), ('half-deviance', 'pearson')):
                    bound = toys.TOL * max(1.0, abs(w))
                    print('%s point %d %s: %r, want %r (%.3g of the bound)' % (what, p, name, g, w, abs(g - w) / bound))
                    assert abs(g - w) <= bound, '%s point %d %s: %r, want %r' % (what, p, name, g, w)
                    note(c.family, 'eval_gof', abs(g - w) / bound)
            return got
        ref = across_loads(c, ctx, body)
        if c.family == 'load_forms':
            chunks = wc.GEOMETRIES[c.family][0][0]
            settings(ctx, chunks, 2)
            for p in range(2):
                s = slice(p, p + 1)
                alone = ctx.eval_gof(c.z[s], c.rs[s], c.ds[s])
                same([a[0] for a in alone], [b[p] for b in ref[chunks]], 'nt_loads 2, eval_gof, point %d' % p)
    finally:
        ctx.close()


@pytest.mark.parametrize('key', wc.FULL_KEYS, ids=KEY_IDS)
def test_real_valued_counts(key):
    """k_sourcewise_real<SC, EM, GRAD, NT>: half-deviance of the real-valued sets and its gradient, gradient on and off"""
    c = case_of(key)
    wants = [want(key, 'real', p) for p in range(2)]
    assert all(w['status'] == 0 and np.isfinite(w['half_deviance']) and w['half_deviance'] > 0 for w in wants)
    ctx = upload(c)
    try:
        def body(what):
            got = stable(c, lambda s: ctx.eval_real(c.z[s], c.rs[s], c.ds[s]), what + ', eval_real', ctx)
            value = stable(c, lambda s: ctx.eval_real(c.z[s], c.rs[s], c.ds[s], gradient=False), what + ', eval_real, value only', ctx)
            real.check_against_oracle(got, wants, what)
            real.check_against_oracle(value, wants, what + ', value only', gradient=False)
            np.testing.assert_array_equal(value[0], got[0], err_msg=what + ': values only against the gradient call')
            np.testing.assert_array_equal(value[3], got[3])
            for p, w in enumerate(wants):                   # (the figures check_against_oracle held to its bounds)
                note(c.family, 'eval_real', abs(got[0][p] - w['half_deviance']) / (real.TOL * max(1.0, abs(w['half_deviance']))))
                g = np.concatenate([got[1][p], got[2][p]])
                note(c.family, 'eval_real, gradient', np.max(np.abs(g - w['grad']) / (real.TOL * np.maximum(1.0, w['grad_cond']))))
            return got
        ref = across_loads(c, ctx, body)
        if c.family == 'load_forms':
            chunks = wc.GEOMETRIES[c.family][0][0]
            settings(ctx, chunks, 2)
            for p in range(2):
                s = slice(p, p + 1)
                alone = ctx.eval_real(c.z[s], c.rs[s], c.ds[s])
                same([a[0] for a in alone], [b[p] for b in ref[chunks]], 'nt_loads 2, eval_real, point %d' % p)
                assert ctx.eval_real(c.z[s], c.rs[s], c.ds[s], gradient=False)[0][0] == ref[chunks][0][p]
    finally:
        ctx.close()


@pytest.mark.parametrize('key', wc.EXPECT_KEYS, ids=KEY_IDS)
def test_expected_counts(key):
    """k_sourcewise_expect<SC, EM, PS, NT>: every bin of the expectation, in total and per source, against the long-double sum"""
    c = case_of(key)
    S, B = len(c.model['own']), fo.n_bins(c.model)
    ctx = upload(c)
    try:
        def body(what):
            mu, = stable(c, lambda s: (ctx.expected_counts(c.z[s], c.rs[s]),), what + ', expected_counts')
            per, = stable(c, lambda s: (ctx.expected_counts(c.z[s], c.rs[s], per_source=True),), what + ', expected_counts per source')
            assert mu.shape == (2, B) and per.shape == (2, S, B)
            for p in range(2):
                want_mu, want_per = want(key, 'expect', p)
                note(c.family, 'expected_counts', check_entries(mu[p], want_mu, want_mu, what='%s mu[%d]' % (what, p)) / C_POISSON)
                note(c.family, 'expected_counts',
                     check_entries(per[p], want_per, want_per, what='%s per source[%d]' % (what, p)) / C_POISSON)
                np.testing.assert_allclose(per[p].sum(axis=0), mu[p], rtol=1e-13, atol=0)
            return mu, per
        ref = across_loads(c, ctx, body)
        if c.family == 'load_forms':
            chunks = wc.GEOMETRIES[c.family][0][0]
            settings(ctx, chunks, 2)
            for p in range(2):
                s = slice(p, p + 1)
                np.testing.assert_array_equal(ctx.expected_counts(c.z[s], c.rs[s])[0], ref[chunks][0][p])
                np.testing.assert_array_equal(ctx.expected_counts(c.z[s], c.rs[s], per_source=True)[0], ref[chunks][1][p])
    finally:
        ctx.close()


@pytest.mark.parametrize('key', wc.CURVATURE_KEYS, ids=KEY_IDS)
def test_hessian_and_information(key):
    """k_factored_curv<SC, EM, FISHER, PS, PANEL> (no nontemporal form): once per tile_chunks, every Gram panel a launch of its own
    over the same walk"""
    c = case_of(key)
    ctx = upload(c)
    try:
        for chunks in sorted({ch for ch, _ in wc.GEOMETRIES[c.family]}):
            settings(ctx, chunks, 0)
            what = '%s %s, tile_chunks %d' % (c.family, c.name, chunks)
            worst_h, worst_i = curv.check_curvature(ctx, c.model, c.z, c.rs, c.counts, what, dataset=c.ds, expanded=False)
            grid_check(ctx, c, 2)
            note(c.family, 'eval_hess', worst_h / C_POISSON)
            note(c.family, 'eval_fisher', worst_i / curv.TOL)
            hess = stable(c, lambda s: ctx.eval_hess(c.z[s], c.rs[s], c.ds[s]), what + ', eval_hess', ctx)
            same(hess[:3] + hess[4:], ctx.eval_grad(c.z, c.rs, c.ds), what + ': eval_hess against eval_grad')
            fisher = stable(c, lambda s: ctx.eval_fisher(c.z[s], c.rs[s]), what + ', eval_fisher', ctx)
            assert not hess[4].any() and not fisher[3].any(), what
    finally:
        ctx.close()
