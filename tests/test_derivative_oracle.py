"""The exact derivative oracle (tests/derivative_oracle.py) against the likelihood evaluated in mpmath at 40 digits and
differentiated by mpmath, and its per-entry bound against deliberate bugs: each mutation must break the bound at a typical
point.  CPU only."""
import itertools

import numpy as np
import pytest

import derivative_oracle as do
from golden_util import case_names, load_case
from oracle import blueice_oracle as orc

mpmath = pytest.importorskip('mpmath')
mp = mpmath.mp

BINNED = [n for n in case_names() if load_case(n)['bb_source'] < 0 and not n.startswith('unb_')]
BB = ['bb_d2', 'bb_two_shape', 'ref_bb_second_source', 'mini4bb_zero_u']
UNBINNED = ['unb_shape_2src', 'unb_d0_three_sources', 'unb_nan_pdf', 'unb_mc_hist', 'unb_ref_value', 'unb_shape_2src_clamped']
ORACLE_C = 4            # the oracle itself: a few roundings of cond at most


def mini4bb_zero_u():
    """A mini4bb-like model (4 shape axes, one with a single anchor, 3 sources, Beeston-Barlow source 0) in which the other
    sources expect exactly nothing in a block of bins (U_b == 0)."""
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel(3, (2, 3, 2, 1), (7, 5, 3), bb_source=0)
    model = m.dense_model()
    ps = model['ps'].reshape(model['ps'].shape[:m.d + 1] + (m.B,)).copy()
    ps[..., 1:, 40:55] = 0.0
    model['ps'] = ps.reshape(model['ps'].shape)
    return dict(model=model, counts=m.counts(dense=True).reshape(m.bins), d=m.d, S=m.S, bb_source=0)


def case(name):
    if name == 'mini4bb_zero_u':
        return mini4bb_zero_u()
    if name == 'unb_shape_2src_clamped':      # events 0 and 3 have density 0 at every anchor: on the outlier clamp
        c = load_case('unb_shape_2src')
        ps = np.array(c['model']['ps'], dtype=float)
        ps[..., 0] = 0.0
        ps[..., 3] = 0.0
        return dict(c, model=dict(c['model'], ps=ps))
    return load_case(name)


def points(c, seed):
    """An interior point, and one on anchors: interior anchors where an axis has them, else the top corner."""
    rng = np.random.default_rng(seed)
    grids = [np.asarray(g, dtype=float) for g in c['model']['anchor_z']]
    z_in = np.array([rng.uniform(g[0] + 0.1 * (g[1] - g[0]), g[-1] - 0.1 * (g[-1] - g[-2])) if len(g) > 1 else g[0]
                     for g in grids])
    z_an = np.array([g[len(g) // 2] if len(g) > 2 else g[-1] for g in grids])
    return [(z_in, rng.uniform(0.6, 1.4, c['S'])), (z_an, rng.uniform(0.6, 1.4, c['S']))]


# ---- the likelihood in mpmath -------------------------------------------------------------------------------------

class MpModel:
    """The likelihood at high precision on the float64 tensors; `value(theta, cells)` with the grid cell of every axis fixed
    (the cell's multilinear polynomial), or re-found per point when `cells` is None."""

    def __init__(self, c, kind):
        self.kind = kind
        self.model = c['model']
        self.grids = [np.asarray(g, dtype=float) for g in self.model['anchor_z']]
        self.d, self.S = len(self.grids), int(c['S'])
        self.bb = c.get('bb_source', -1)
        self.outlier = c.get('outlier', 0.0)
        self.last_clamped = set()
        self.counts = None if kind == 'unbinned' else [mp.mpf(float(x)) for x in np.asarray(c['counts'], float).ravel()]

    def cells(self, z):
        return [orc.find_cell(g, float(zi))[0] if len(g) > 1 else 0 for g, zi in zip(self.grids, z)]

    def _interp(self, key, cells, z):
        """-> per source lists of interpolated values over the bins (mp), and the interpolated rates."""
        d, S = self.d, self.S
        axes = []
        for g, k, zi in zip(self.grids, cells, z):
            if len(g) == 1:
                axes.append([(0, mp.mpf(1))])
                continue
            t = (zi - mp.mpf(g[k])) / (mp.mpf(g[k + 1]) - mp.mpf(g[k]))
            axes.append([(k, 1 - t), (k + 1, t)])
        tab = None
        for combo in itertools.product(*axes):
            idx = tuple(a for a, _ in combo)
            w = mp.mpf(1)
            for _, wi in combo:
                w *= wi
            rows = np.asarray(self.model[key][idx], dtype=float).reshape(S, -1) if key != 'mus' else \
                np.asarray(self.model[key][idx], dtype=float).reshape(S, 1)
            if tab is None:
                tab = [[mp.mpf(0)] * rows.shape[1] for _ in range(S)]
            for s in range(S):
                for b in range(rows.shape[1]):
                    x = rows[s, b]
                    tab[s][b] = tab[s][b] + (w * mp.mpf(x) if not np.isnan(x) else mp.nan)
        return tab

    def value(self, theta, cells=None, clamped=None):
        theta = [mp.mpf(x) if not isinstance(x, mp.mpf) else x for x in theta]
        z, rs = theta[:self.d], theta[self.d:]
        cells = cells if cells is not None else self.cells([float(x) for x in z])
        u = self._interp('mus', cells, z)
        r = [u[s][0] * rs[s] for s in range(self.S)]
        P = self._interp('ps', cells, z)
        nb = len(P[0])
        if self.kind == 'unbinned':
            ll = -mp.fsum(r)
            for e in range(nb):
                lam = mp.fsum(r[s] * P[s][e] for s in range(self.S) if not mp.isnan(P[s][e]))
                on_clamp = (self.outlier != 0 and not lam > 0) if clamped is None else e in clamped
                ll += mp.log(mp.mpf(self.outlier)) if on_clamp else mp.log(lam)
                if on_clamp:
                    self.last_clamped.add(e)
            return ll
        if self.kind == 'bb':
            i = self.bb
            a = self._interp('n_model', cells, z)[i]
            N = mp.fsum(a)
            p_cal = r[i] / N
            mu = []
            for b in range(nb):
                U = mp.fsum(r[s] * P[s][b] for s in range(self.S) if s != i)
                n = self.counts[b]
                p = P[i][b] / a[b] * N * p_cal
                if U == 0:
                    A = (n + a[b]) / (1 + p_cal)
                else:
                    disc = orc._bb_disc(a[b], p, U, n)
                    A = (-U * p - U + a[b] * p + n * p + mp.sqrt(disc)) / (2 * p * (p + 1))
                mu.append(U + A * p)
        else:
            mu = [mp.fsum(r[s] * P[s][b] for s in range(self.S)) for b in range(nb)]
        return mp.fsum((n * mp.log(m) if n > 0 else 0) - m - mp.loggamma(n + 1) for n, m in zip(self.counts, mu))

    def derivatives(self, z, rs, hessian):
        """-> (ll, grad, H or None) by mpmath differentiation.  Gradient: central differences inside a cell; at an interior
        anchor the one-sided difference into the point's cell (upwards), at the last anchor into the cell below.  Hessian: of
        the cell's polynomial (the function restricted to the point's cell), which those one-sided limits are."""
        theta = [mp.mpf(float(x)) for x in list(z) + list(rs)]
        F = len(theta)
        cells = self.cells(z)
        self.last_clamped = set()
        ll = self.value(theta)
        clamped = set(self.last_clamped)     # events on the outlier clamp at the point are constants around it
        g = np.zeros(F)
        for q in range(F):
            direction = 0
            if q < self.d and len(self.grids[q]) > 1 and float(z[q]) in self.grids[q]:
                direction = -1 if float(z[q]) == self.grids[q][-1] else 1

            def f(x, q=q):
                th = list(theta)
                th[q] = x
                return self.value(th, clamped=clamped)
            g[q] = float(mp.diff(f, theta[q], direction=direction)) if direction else float(mp.diff(f, theta[q]))
        H = None
        if hessian:
            H = np.zeros((F, F))
            fc = lambda *th: self.value(list(th), cells, clamped)
            for q in range(F):
                for p in range(q, F):
                    n = [0] * F
                    n[q] += 1
                    n[p] += 1
                    H[q, p] = H[p, q] = float(mp.diff(fc, theta, tuple(n)))
        return float(ll), g, H


def oracle_of(c, kind, z, rs, hessian, mutate=None):
    if kind == 'bb':
        return do.bb_gradient(c['model'], z, rs, c['counts'], c['bb_source'], mutate=mutate)
    if kind == 'unbinned':
        return do.derivatives(c['model'], z, rs, unbinned=True, outlier=c['outlier'], hessian=hessian, mutate=mutate)
    return do.derivatives(c['model'], z, rs, counts=c['counts'], hessian=hessian, mutate=mutate)


def check_against_mpmath(c, kind, hessian, seed):
    m = MpModel(c, kind)
    with mp.workdps(40):
        for z, rs in points(c, seed):
            o = oracle_of(c, kind, z, rs, hessian)
            if not np.isfinite(o['ll']):
                continue
            ll, g, H = m.derivatives(z, rs, hessian)
            do.check_entries(o['ll'], ll, o['ll_cond'], ORACLE_C, 'll')
            do.check_entries(o['grad'], g, o['grad_cond'], ORACLE_C, 'grad')
            if hessian:
                do.check_entries(o['hess'], H, o['hess_cond'], ORACLE_C, 'hess')
                assert np.array_equal(o['hess'], o['hess'].T)
            for i, gr in enumerate(m.grids):      # single-anchor axes: exactly zero
                if len(gr) == 1:
                    assert o['grad'][i] == 0 and (not hessian or not o['hess'][i].any())


@pytest.mark.parametrize('name', BINNED)
def test_binned_oracle_matches_mpmath(name):
    c = case(name)
    check_against_mpmath(c, 'binned', True, seed=len(name))


@pytest.mark.parametrize('name', BB)
def test_beeston_barlow_gradient_matches_mpmath(name):
    c = case(name)
    check_against_mpmath(c, 'bb', False, seed=len(name))


@pytest.mark.parametrize('name', UNBINNED)
def test_unbinned_oracle_matches_mpmath(name):
    c = case(name)
    check_against_mpmath(c, 'unbinned', 'nan' not in name, seed=len(name))


def test_zero_u_block_takes_the_special_case():
    c = mini4bb_zero_u()
    S, B = c['S'], int(np.prod(c['counts'].shape))
    ps = c['model']['ps'].reshape(c['model']['ps'].shape[:c['d']] + (S, B))
    assert (ps[..., 1:, 40:55] == 0).all() and (ps[..., 1:, :40] > 0).all()


def test_the_oracle_sums_blocks_like_one_block(monkeypatch):
    """Many bin blocks give what one block gives (the block walk drops or repeats no bin)."""
    from blueice_amd.synthetic import SyntheticModel
    m = SyntheticModel(2, (3,), (1000,))
    model, counts = m.dense_model(), m.counts()
    z, rs = np.array([0.3]), np.array([1.1, 0.8])
    one = do.derivatives(model, z, rs, counts=counts)
    monkeypatch.setattr(do, 'BLOCK', 77)
    many = do.derivatives(model, z, rs, counts=counts)
    do.check_entries(many['grad'], one['grad'], one['grad_cond'], 1)
    do.check_entries(many['hess'], one['hess'], one['hess_cond'], 1)


# ---- the bound catches real bugs ------------------------------------------------------------------------------------

KINDS = {'binned': 'd2_nonuniform', 'unbinned': 'unb_shape_2src', 'bb': 'bb_d2'}


def typical(kind):
    c = case(KINDS[kind])
    rng = np.random.default_rng(5)
    z = np.array([rng.uniform(g[0], g[-1]) for g in c['model']['anchor_z']])
    return c, z, rng.uniform(0.7, 1.3, c['S'])


def assert_breaks(good, bad, keys):
    broken = []
    for k in keys:
        try:
            do.check_entries(bad[k], good[k], good[k + '_cond'], do.C_POISSON, k)
        except AssertionError as e:
            broken.append(str(e))
    assert broken, 'the mutation passed the bound'
    return broken


@pytest.mark.parametrize('kind', list(KINDS))
def test_bound_catches_a_corner_coefficient_off_by_1e_9(kind):
    c, z, rs = typical(kind)
    good = oracle_of(c, kind, z, rs, kind != 'bb')
    # row: corner 0, source 1 (not the Beeston-Barlow source); column: d / d z_0
    bad = oracle_of(c, kind, z, rs, kind != 'bb', mutate={'coef': (1, 1, 1e-9)})
    assert_breaks(good, bad, ['grad'])


@pytest.mark.parametrize('kind', list(KINDS))
def test_bound_catches_a_dropped_bin(kind):
    c, z, rs = typical(kind)
    good = oracle_of(c, kind, z, rs, kind != 'bb')
    bad = oracle_of(c, kind, z, rs, kind != 'bb', mutate={'drop_bin': 7})
    assert_breaks(good, bad, ['grad'] + (['hess'] if kind != 'bb' else []))


@pytest.mark.parametrize('kind', ['binned', 'unbinned'])
def test_bound_catches_a_flipped_gram_pair(kind):
    c, z, rs = typical(kind)
    good = oracle_of(c, kind, z, rs, True)
    bad = oracle_of(c, kind, z, rs, True, mutate={'gram_flip': (0, 3)})
    assert_breaks(good, bad, ['hess'])


@pytest.mark.parametrize('kind', list(KINDS))
def test_bound_catches_the_wrong_cell_at_an_anchor(kind):
    c, z, rs = typical(kind)
    z = np.array(z)
    z[0] = c['model']['anchor_z'][0][1]          # an interior anchor of axis 0: assigned to the cell above
    good = oracle_of(c, kind, z, rs, kind != 'bb')
    bad = oracle_of(c, kind, z, rs, kind != 'bb', mutate={'cell_shift': {0: -1}})
    assert abs(bad['ll'] - good['ll']) <= 1e-12 * abs(good['ll'])     # the same value: only the slopes differ
    assert_breaks(good, bad, ['grad'])
