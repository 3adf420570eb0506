"""Every host sub-batch seam of the per-point entry points, crossed on the device: the cases of tests/batch_seam_cases.py (whose
arithmetic tests/test_batch_seam_cases.py checks on the CPU).

At every seam the host re-points the descriptor arrays, re-uses device buffers and maps piece-local item numbers back to point
indices; a mistake there gives plausible numbers for the wrong point, and only a call that crosses the seam can see it.  Per case:

    seam crossed    the read-only parameter last_point_pieces equals the case's figure after the large call (and the number of
                    launch passes after the call of the probes alone)
    bit for bit     every probe -- two live items on either side of every seam, the first and last point, the dead points'
                    neighbours -- equals the same point in a call of the probes alone: an item's blocks depend on the rows' length
                    alone (FacBatch), the coarse geometry never on the number of points, the expectation kernels sum per bin
    oracle          the probes against the oracle and the bound of the entry point's own test file, imported from there:
                    check_entries with C_POISSON (bi_eval_factored, the Hessian, both expected-counts calls), fisher_oracle.check,
                    and the 1e-10 bars of goodness of fit, real-valued data and coarse views
    dead points     their documented defaults, every status word of the P points, no nan or inf at a live point

The Asimov and generator cases hold rows / toys on both sides of the truth seam to bi_*_expected_counts bit for bit and to a call
with that truth alone (same seed, toy_offset = the toy's number): test_sourcewise_real_gpu.py's identity taken at the seam."""
import time

import numpy as np
import pytest

import batch_seam_cases as bsc
import factored_oracle as fo
import fisher_oracle
import gof_oracle
import sourcewise_real_oracle as sro
import sourcewise_toy_cases as toy_cases
import toy_oracle
from derivative_oracle import C_POISSON, check_entries, derivatives
from test_coarse_jacobian_gpu import check as jacobian_check, derivatives as coarse_derivatives
from test_factored_curvature_gpu import TOL as FISHER_TOL
from test_gof_gpu import TOL
from test_sourcewise_coarse_gpu import cell_map, reduce_wide, within_bar
from test_sourcewise_real_gpu import check_against_oracle as check_real

pytestmark = pytest.mark.gpu

N_SETS = 3                       # datasets (counts, real-valued sets) of every model; point p reads set p % N_SETS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def names(family, entry=None):
    return [c.name for c in bsc.CASES if c.family == family and (entry is None or c.entry in entry)]


# ---- models, data and oracles: built once per module and left unchanged -----------------------------------------------------------

class World:
    def __init__(self):
        self._made = {}

    def of(self, key):
        """-> dict(model, full (the expansion; the model itself for the grid family), truths zt, rst [3, ..], counts [3, B],
        real [3, B])"""
        if key in self._made:
            return self._made[key]
        model = bsc.model_of(key)
        rng = np.random.default_rng(bsc.SEED + 17 + sum(key.encode()))
        if 'own' in model:
            full = fo.expand(model)
            zt, rst = toy_cases.box_points(model, rng, N_SETS)
            counts = np.stack([rng.poisson(fo.expectation(model, zt[t], rst[t])).astype(float) for t in range(N_SETS)])
            real = sro.real_datasets('seam_' + key, model, zt, rst)
        else:
            full = model
            S = model['mus'].shape[-1]
            zt, rst = rng.uniform(-0.9, 0.9, (N_SETS, len(model['anchor_z']))), rng.uniform(0.6, 1.5, (N_SETS, S))
            mu = [gof_oracle.statistics(model, np.zeros(bsc.MODEL_BINS[key]), zt[t], rst[t])['mu'] for t in range(N_SETS)]
            counts = np.stack([rng.poisson(m).astype(float) for m in mu])
            real = None
        self._made[key] = dict(model=model, full=full, zt=zt, rst=rst, counts=counts, real=real)
        return self._made[key]


@pytest.fixture(scope='module')
def world():
    return World()


def sourcewise_context(w, counts=True, real=False):
    ctx = toy_cases.upload(w['model'], w['counts'] if counts else None)
    if real:
        ctx.set_real_counts(w['real'])
    return ctx


def grid_context(w, counts=False, sparse=0):
    from blueice_amd.device import DeviceContext
    ctx = DeviceContext(0)
    ctx.set_param('sparse', sparse)
    ctx.upload_model(w['model']['anchor_z'], w['model']['ps'], w['model']['mus'])
    if counts:
        ctx.upload_counts(w['counts'])
    return ctx


# ---- what every case with points shares ---------------------------------------------------------------------------------------------

def cross(case, ctx, evaluate, dead_values, alone_pieces=1):
    """evaluate(z, rs, ds) -> (float arrays [n, ...], status [n] or None).  The whole batch and the probes alone: the counter, the
    probes bit for bit, the dead points' defaults (dead_values, one per array: the value every entry has, nan for nan), every
    status word, no nan or inf at a live point -> (z, rs, ds, the batch's arrays, seconds of the large call)"""
    z, rs = case.points()
    ds = np.arange(case.P, dtype=np.int64) % N_SETS
    t0 = time.perf_counter()
    full, st = evaluate(z, rs, ds)
    seconds = time.perf_counter() - t0
    pieces = ctx.get_param('last_point_pieces')
    print('%s (%s): P = %d, %d live, seams %s: last_point_pieces = %d (want %d), %.3f s' % (
        case.name, case.entry, case.P, case.n_live, case.levels, pieces, case.pieces, seconds))
    assert pieces == case.pieces, '%s: the call cut its live items into %d pieces, the case crosses its seams with %d' % (case.name, pieces, case.pieces)
    pr = case.probes
    alone, st_alone = evaluate(z[pr], rs[pr], ds[pr])
    assert ctx.get_param('last_point_pieces') == alone_pieces
    assert st_alone is None or not st_alone.any()
    live = bsc.live_of(case.P, case.dead)
    number = np.searchsorted(live, pr)                          # the probes' live numbers
    last_piece = number >= case.seams[-1]
    for k, (a, b) in enumerate(zip(full, alone)):
        assert np.all(np.isfinite(b)), '%s, output %d: the probes are live points' % (case.name, k)
        same = np.array([np.array_equal(bits(a[p]), bits(b[i])) for i, p in enumerate(pr)])
        assert same.all(), ('%s, output %d: the probes %s (live numbers %s; in the last piece: %s) differ from the same points evaluated alone'
                            % (case.name, k, pr[~same], number[~same], last_piece[~same]))
        assert np.all(np.isfinite(a[live])), '%s, output %d: a live point is nan or inf' % (case.name, k)
        for p in case.dead:
            v = dead_values[k]
            assert np.all(np.isnan(a[p])) if np.isnan(v) else np.all(a[p] == v), '%s, output %d: dead point %d has %r' % (case.name, k, p, a[p])
    if st is not None:
        np.testing.assert_array_equal(st, case.status(), err_msg=case.name + ': status')
    return z, rs, ds, full, seconds


# ---- FacBatch::run: value, gradient, goodness of fit, real-valued data, Hessian, information ---------------------------------------

def check_value_grad(w, z, rs, ds, out, pr, what, grad):
    worst = 0.0
    for p in pr:
        want = derivatives(w['full'], z[p], rs[p], w['counts'][ds[p]], hessian=False)
        worst = max(worst, check_entries(out[0][p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (what, p)))
        if grad:
            worst = max(worst, check_entries(np.concatenate([out[1][p], out[2][p]]), want['grad'], want['grad_cond'], what='%s grad[%d]' % (what, p)))
    return worst


@pytest.mark.parametrize('name', names('sourcewise', ['bi_eval_factored']))
def test_bi_eval_factored_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    grad = case.extra['call'] == 'grad'
    ctx = sourcewise_context(w)
    try:
        def evaluate(z, rs, ds):
            if grad:
                ll, gz, gs, st = ctx.eval_grad(z, rs, ds)
                return [ll, gz, gs], st
            ll, st = ctx.eval(z, rs, ds)
            return [ll], st

        z, rs, ds, out, _ = cross(case, ctx, evaluate, [-np.inf, np.nan, np.nan])
        worst = check_value_grad(w, z, rs, ds, out, case.probes, name, grad)
        print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (name, worst, C_POISSON))
    finally:
        ctx.close()


@pytest.mark.parametrize('name', names('sourcewise', ['bi_eval_sourcewise_gof']))
def test_bi_eval_sourcewise_gof_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    ctx = sourcewise_context(w)
    try:
        def evaluate(z, rs, ds):
            half, pearson, st = ctx.eval_gof(z, rs, ds)
            return [half, pearson], st

        z, rs, ds, (half, pearson), _ = cross(case, ctx, evaluate, [np.inf, np.inf])
        for p in case.probes:
            s = gof_oracle.statistics(w['full'], w['counts'][ds[p]], z[p], rs[p], dtype=np.longdouble)
            for got, want, what in ((half[p], float(s['half_deviance']), 'half-deviance'), (pearson[p], float(s['pearson']), 'pearson')):
                assert abs(got - want) <= TOL * max(1.0, abs(want)), '%s point %d %s: %r, want %r' % (name, p, what, got, want)
    finally:
        ctx.close()


@pytest.mark.parametrize('name', names('sourcewise', ['bi_eval_sourcewise_real']))
def test_bi_eval_sourcewise_real_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    grad = case.extra['call'] == 'grad'
    ctx = sourcewise_context(w, counts=False, real=True)
    try:
        def evaluate(z, rs, ds):
            half, gz, gs, st = ctx.eval_real(z, rs, ds, gradient=grad)
            return ([half, gz, gs] if grad else [half]), st

        z, rs, ds, out, _ = cross(case, ctx, evaluate, [np.inf, np.nan, np.nan])
        pr = case.probes
        wants = [sro.want_point(w['model'], w['full'], w['real'][ds[p]], z[p], rs[p]) for p in pr]
        got = (out[0][pr], out[1][pr] if grad else None, out[2][pr] if grad else None, np.zeros(len(pr), dtype=np.int32))
        check_real(got, wants, name, gradient=grad)
    finally:
        ctx.close()


@pytest.mark.parametrize('name', names('sourcewise', ['bi_eval_sourcewise_hess']))
def test_bi_eval_sourcewise_hess_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    ctx = sourcewise_context(w)
    try:
        def evaluate(z, rs, ds):
            ll, gz, gs, H, st = ctx.eval_hess(z, rs, ds)
            return [ll, gz, gs, H], st

        z, rs, ds, out, _ = cross(case, ctx, evaluate, [-np.inf, np.nan, np.nan, np.nan], alone_pieces=len(case.extra['passes']))
        worst = 0.0
        for p in case.probes:
            want = derivatives(w['full'], z[p], rs[p], w['counts'][ds[p]], hessian=True)
            worst = max(worst, check_entries(out[0][p], want['ll'], want['ll_cond'], what='%s ll[%d]' % (name, p)),
                        check_entries(np.concatenate([out[1][p], out[2][p]]), want['grad'], want['grad_cond'], what='%s grad[%d]' % (name, p)),
                        check_entries(out[3][p], want['hess'], want['hess_cond'], what='%s hess[%d]' % (name, p)))
            assert np.array_equal(out[3][p], out[3][p].T)
        print('%s: worst |err| / (2^-52 cond) = %.3g of C = %d' % (name, worst, C_POISSON))
    finally:
        ctx.close()


@pytest.mark.parametrize('name', names('sourcewise', ['bi_eval_sourcewise_fisher']))
def test_bi_eval_sourcewise_fisher_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    ctx = sourcewise_context(w, counts=False)                   # the expected information reads no data
    try:
        unbounded = {}

        def evaluate(z, rs, ds):
            info, total, unb, st = ctx.eval_fisher(z, rs)
            unbounded[len(z)] = unb
            return [info, total], st

        z, rs, ds, (info, total), _ = cross(case, ctx, evaluate, [np.nan, np.nan], alone_pieces=len(case.extra['passes']))
        unb = unbounded[case.P]
        np.testing.assert_array_equal(unb[case.probes], unbounded[len(case.probes)])
        assert not unb[list(case.dead)].any()
        worst = 0.0
        for p in case.probes:
            wi = fisher_oracle.information(w['full'], z[p], rs[p])
            worst = max(worst, fisher_oracle.check(info[p], wi, what='%s info[%d]' % (name, p), tol=FISHER_TOL))
            np.testing.assert_array_equal(unb[p], wi['unbounded'])
            assert abs(total[p] - wi['total']) <= FISHER_TOL * max(1.0, wi['total'])
        print('%s: information worst |err| / max(1, cond) = %.3g of %g' % (name, worst, FISHER_TOL))
    finally:
        ctx.close()


# ---- the calls that write bins or cells, source-wise ---------------------------------------------------------------------------------

def test_bi_sourcewise_expected_counts_across_the_memory_cap(world):
    case = bsc.BY_NAME['sw_expect_mem']
    w = world.of(case.model_key)
    ctx = sourcewise_context(w, counts=False)
    try:
        z, rs, _, (mu,), _ = cross(case, ctx, lambda z, rs, ds: ([ctx.expected_counts(z, rs)], None), [np.nan])
        worst = 0.0
        for p in case.probes:
            want = toy_cases.exact_expectation(w['model'], z[p], rs[p])[0]
            worst = max(worst, check_entries(mu[p], want, want, what='%s mu[%d]' % (case.name, p)))
        print('%s: worst |err| / (2^-52 mu) = %.3g of C = %d' % (case.name, worst, C_POISSON))
    finally:
        ctx.close()


def test_bi_sourcewise_expected_coarse_across_the_launch_limit(world):
    case = bsc.BY_NAME['sw_coarse_launch']
    w = world.of(case.model_key)
    shape, groups = case.extra['shape'], [np.asarray(g, dtype=np.int32) for g in case.extra['groups']]
    m, cells = cell_map(shape, groups)
    ctx = sourcewise_context(w, counts=False)
    try:
        assert ctx.set_coarse_binning(shape, groups) == cells

        def evaluate(z, rs, ds):
            mu, st = ctx.expected_coarse(cells, z, rs)
            return [mu], st

        z, rs, _, (mu,), _ = cross(case, ctx, evaluate, [np.nan])
        for p in case.probes:
            want = reduce_wide(m, cells, toy_cases.exact_expectation(w['model'], z[p], rs[p])[0])
            within_bar(mu[p], want, '%s, point %d' % (case.name, p))
    finally:
        ctx.close()


def test_bi_sourcewise_coarse_counts_across_the_launch_limit(world):
    """the store's toys, drawn on the device, addressed through a dataset list longer than one launch: every row is exactly
    np.bincount of the toy's downloaded counts"""
    case = bsc.BY_NAME['sw_coarse_counts_launch']
    w = world.of(case.model_key)
    shape, groups = case.extra['shape'], [np.asarray(g, dtype=np.int32) for g in case.extra['groups']]
    m, cells = cell_map(shape, groups)
    T = case.extra['T']
    ctx = sourcewise_context(w, counts=False)
    try:
        ctx.generate_toys_points(w['zt'], w['rst'], [T // 3] * 3, bsc.TOY_SEED)
        assert ctx.T == T and ctx.set_coarse_binning(shape, groups) == cells
        down = np.stack([ctx.download_counts(t) for t in range(T)])
        want = np.stack([np.bincount(m[m >= 0], weights=row[m >= 0], minlength=cells) for row in down])
        assert want.sum() > 0
        ds = (np.arange(case.P, dtype=np.int64) * 5 + 1) % T
        t0 = time.perf_counter()
        got = ctx.coarse_counts(cells, ds)
        seconds = time.perf_counter() - t0
        pieces = ctx.get_param('last_point_pieces')
        print('%s: n = %d, seams %s: last_point_pieces = %d (want %d), %.3f s' % (case.name, case.P, case.levels, pieces, case.pieces, seconds))
        assert pieces == case.pieces
        assert np.array_equal(got, want[ds])
        alone = ctx.coarse_counts(cells, ds[case.probes])
        assert ctx.get_param('last_point_pieces') == 1 and np.array_equal(bits(alone), bits(got[case.probes]))
    finally:
        ctx.close()


def test_bi_sourcewise_set_asimov_counts_across_the_truth_launches(world):
    case = bsc.BY_NAME['sw_asimov_launch']
    w = world.of(case.model_key)
    z, rs = case.points()
    pr = case.probes
    ctx = sourcewise_context(w, counts=False)
    try:
        t0 = time.perf_counter()
        assert ctx.set_asimov_counts(z, rs) == case.P
        seconds = time.perf_counter() - t0
        pieces = ctx.get_param('last_point_pieces')
        print('%s: H = %d, seams %s: last_point_pieces = %d (want %d), %.3f s' % (case.name, case.P, case.levels, pieces, case.pieces, seconds))
        assert pieces == case.pieces and ctx.real_count_sets == case.P
        rows = np.stack([ctx.download_real_counts(int(h)) for h in pr])
        half, _, _, st = ctx.eval_real(z[pr], rs[pr], pr)                       # set h at its own truth: exactly 0
        assert not st.any() and np.all(half == 0.0)
        assert np.array_equal(bits(rows), bits(ctx.expected_counts(z[pr], rs[pr])))
        for i, h in enumerate(pr):
            want = toy_cases.exact_expectation(w['model'], z[h], rs[h])[0].astype(float)
            assert np.all(np.abs(rows[i] - want) <= TOL * np.maximum(1.0, want)), h
            assert ctx.set_asimov_counts(z[h:h + 1], rs[h:h + 1]) == 1 and ctx.get_param('last_point_pieces') == 1
            assert np.array_equal(bits(ctx.download_real_counts(0)), bits(rows[i])), h
    finally:
        ctx.close()


def test_bi_sourcewise_generate_toys_across_the_truth_launches(world):
    """H truths, one toy each at the probes and none elsewhere: toy t is drawn from the expectation row of its truth, which the
    second launch over the truths wrote for the probes behind the seam"""
    case = bsc.BY_NAME['sw_toys_launch']
    w = world.of(case.model_key)
    z, rs = case.points()
    pr = case.probes
    n_toys = np.zeros(case.P, dtype=np.int64)
    n_toys[pr] = 1
    ctx = sourcewise_context(w, counts=False)
    try:
        t0 = time.perf_counter()
        ctx.generate_toys_points(z, rs, n_toys, bsc.TOY_SEED)
        seconds = time.perf_counter() - t0
        pieces = ctx.get_param('last_point_pieces')
        print('%s: H = %d, seams %s: last_point_pieces = %d (want %d), %.3f s' % (case.name, case.P, case.levels, pieces, case.pieces, seconds))
        assert pieces == case.pieces and ctx.T == len(pr)
        toys = np.stack([ctx.download_counts(t) for t in range(len(pr))])
        for t, h in enumerate(pr):
            mu = fo.expectation(w['model'], z[h], rs[h])
            rep = toy_oracle.per_bin_toys(mu, bsc.TOY_SEED, np.array([t], dtype=np.uint64))
            toy_oracle.compare_toys(toys[t:t + 1], rep, what='%s truth %d' % (case.name, h))
            ctx.set_param('toy_offset', t)                      # the truth alone, its toy's number in the seed's ensemble
            ctx.generate_toys_points(z[h:h + 1], rs[h:h + 1], [1], bsc.TOY_SEED)
            assert ctx.get_param('last_point_pieces') == 1
            assert np.array_equal(bits(ctx.download_counts(0)), bits(toys[t])), h
        ctx.set_param('toy_offset', 0)
    finally:
        ctx.close()


# ---- the grid model -----------------------------------------------------------------------------------------------------------------

def grid_exact(model, z, rs, B):
    """the long-double expectation per source [S, B] of gof_oracle"""
    return gof_oracle.statistics(model, np.zeros(B), z, rs, dtype=np.longdouble)['mu_sources']


@pytest.mark.parametrize('name', names('grid', ['bi_expected_counts']))
def test_bi_expected_counts_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    per_source = case.extra['R'] > 1
    B = bsc.MODEL_BINS[case.model_key]
    ctx = grid_context(w)
    try:
        z, rs, _, (mu,), _ = cross(case, ctx, lambda z, rs, ds: ([ctx.expected_counts(z, rs, per_source=per_source)], None), [np.nan])
        worst = 0.0
        for p in case.probes:
            want = grid_exact(w['model'], z[p], rs[p], B)
            want = want if per_source else want.sum(axis=0)
            worst = max(worst, check_entries(mu[p], want, want, what='%s mu[%d]' % (name, p)))
        print('%s: worst |err| / (2^-52 mu) = %.3g of C = %d' % (name, worst, C_POISSON))
    finally:
        ctx.close()


@pytest.mark.parametrize('name', names('grid', ['bi_expected_coarse']))
def test_bi_expected_coarse_across_its_seams(world, name):
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    shape, groups = case.extra['shape'], [np.asarray(g, dtype=np.int32) for g in case.extra['groups']]
    m, cells = cell_map(shape, groups)
    ctx = grid_context(w)
    try:
        assert ctx.set_coarse_binning(shape, groups) == cells

        def evaluate(z, rs, ds):
            mu, st = ctx.expected_coarse(cells, z, rs)
            return [mu], st

        z, rs, _, (mu,), _ = cross(case, ctx, evaluate, [np.nan])
        for p in case.probes:
            want = reduce_wide(m, cells, grid_exact(w['model'], z[p], rs[p], int(np.prod(shape))).sum(axis=0))
            within_bar(mu[p], want, '%s, point %d' % (name, p))
    finally:
        ctx.close()


def test_bi_expected_coarse_jacobian_across_the_launch_limit(world):
    case = bsc.BY_NAME['grid_jacobian_launch']
    w = world.of(case.model_key)
    shape, groups = case.extra['shape'], [np.asarray(g, dtype=np.int32) for g in case.extra['groups']]
    m, cells = cell_map(shape, groups)
    ctx = grid_context(w)
    try:
        assert ctx.set_coarse_binning(shape, groups) == cells

        def evaluate(z, rs, ds):
            mu, jac, st = ctx.expected_coarse_jacobian(cells, z, rs)
            return [mu, jac], st

        z, rs, _, (mu, jac), _ = cross(case, ctx, evaluate, [np.nan, np.nan])
        total, _ = ctx.expected_coarse(cells, z[case.probes], rs[case.probes])
        assert np.array_equal(bits(mu[case.probes]), bits(total))           # mu has the bits of bi_expected_coarse
        worst = 0.0
        for p in case.probes:
            mu_b, dmu_b, cond_b = coarse_derivatives(w['model'], z[p], rs[p])
            cond = np.asarray(reduce_wide(m, cells, cond_b), dtype=float)
            worst = max(worst, jacobian_check(mu[p], reduce_wide(m, cells, mu_b), cond[0], '%s, mu of point %d' % (case.name, p)),
                        jacobian_check(jac[p], reduce_wide(m, cells, dmu_b), cond[1:], '%s, jac of point %d' % (case.name, p)))
        print('%s: the worst entry is at %.3g of TOL max(1, cond)' % (case.name, worst))
    finally:
        ctx.close()


@pytest.mark.parametrize('name', names('grid', ['bi_coarse_counts']))
def test_bi_coarse_counts_across_its_seams(world, name):
    """dense rows (uploaded counts) across the launch limit, and the non-empty-bin lists of device-generated toys across the
    memory cap with an identity binning: every row is exactly np.bincount of the dataset's downloaded counts"""
    case = bsc.BY_NAME[name]
    w = world.of(case.model_key)
    shape, groups = case.extra['shape'], [np.asarray(g, dtype=np.int32) for g in case.extra['groups']]
    m, cells = cell_map(shape, groups)
    T, lists = case.extra['T'], case.extra['form'] == 'lists'
    ctx = grid_context(w, counts=not lists, sparse=1 if lists else 0)
    try:
        if lists:
            ctx.generate_toys(w['zt'][0], w['rst'][0], T, bsc.TOY_SEED)
        assert ctx.T == T and ctx.get_param('dense_counts') == (0 if lists else 1)
        assert ctx.set_coarse_binning(shape, groups) == cells
        down = np.stack([ctx.download_counts(t) for t in range(T)])
        want = np.stack([np.bincount(m[m >= 0], weights=row[m >= 0], minlength=cells) for row in down])
        assert want.sum() > 0
        ds = (np.arange(case.P, dtype=np.int64) * 5 + 1) % T
        t0 = time.perf_counter()
        got = ctx.coarse_counts(cells, ds)
        seconds = time.perf_counter() - t0
        pieces = ctx.get_param('last_point_pieces')
        print('%s: n = %d, seams %s: last_point_pieces = %d (want %d), %.3f s' % (name, case.P, case.levels, pieces, case.pieces, seconds))
        assert pieces == case.pieces
        assert np.array_equal(got, want[ds])
        alone = ctx.coarse_counts(cells, ds[case.probes])
        assert ctx.get_param('last_point_pieces') == 1 and np.array_equal(bits(alone), bits(got[case.probes]))
    finally:
        ctx.close()


def test_bi_set_asimov_counts_across_the_truth_launches(world):
    case = bsc.BY_NAME['grid_asimov_launch']
    w = world.of(case.model_key)
    z, rs = case.points()
    pr = case.probes
    B = bsc.MODEL_BINS[case.model_key]
    ctx = grid_context(w)
    try:
        t0 = time.perf_counter()
        assert ctx.set_asimov_counts(z, rs) == case.P
        seconds = time.perf_counter() - t0
        pieces = ctx.get_param('last_point_pieces')
        print('%s: H = %d, seams %s: last_point_pieces = %d (want %d), %.3f s' % (case.name, case.P, case.levels, pieces, case.pieces, seconds))
        assert pieces == case.pieces and ctx.real_count_sets == case.P
        rows = np.stack([ctx.download_real_counts(int(h)) for h in pr])
        half, _, _, st = ctx.eval_real(z[pr], rs[pr], pr)                       # set h at its own truth: exactly 0
        assert not st.any() and np.all(half == 0.0)
        assert np.array_equal(bits(rows), bits(ctx.expected_counts(z[pr], rs[pr])))
        for i, h in enumerate(pr):
            want = grid_exact(w['model'], z[h], rs[h], B).sum(axis=0)
            check_entries(rows[i], want, want, what='%s row %d' % (case.name, h))
            assert ctx.set_asimov_counts(z[h:h + 1], rs[h:h + 1]) == 1 and ctx.get_param('last_point_pieces') == 1
            assert np.array_equal(bits(ctx.download_real_counts(0)), bits(rows[i])), h
    finally:
        ctx.close()


def test_a_call_without_a_live_item_counts_no_piece(world):
    w = world.of('tile')
    ctx = sourcewise_context(w)
    try:
        z, rs = toy_cases.box_points(w['model'], np.random.default_rng(1), 4)
        ctx.eval_grad(z, rs)
        assert ctx.get_param('last_point_pieces') == 1
        z[:, 0] = w['model']['anchor_z'][0][-1] + 1.0            # every point outside the box
        ll, st = ctx.eval(z, rs)
        assert np.all(st == bsc.ST_OUT_OF_BOUNDS) and np.all(ll == -np.inf) and ctx.get_param('last_point_pieces') == 0
        ctx.eval_grad(z[:1] * 0.0 + [a[0] for a in w['model']['anchor_z']], rs[:1])
        assert ctx.get_param('last_point_pieces') == 1
        assert np.isnan(ctx.expected_counts(z[:1], rs[:1])).all() and ctx.get_param('last_point_pieces') == 0
        with pytest.raises(ValueError):
            ctx.set_param('last_point_pieces', 3)                # read-only
    finally:
        ctx.close()
