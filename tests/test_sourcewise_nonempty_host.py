"""The non-empty-bin form of source-wise models without a GPU: its NumPy specification against the exact oracle of the expanded
grid (check_entries, C = C_POISSON = 256: the bar of every source-wise test), the header / binding / build list of the new
symbols, and the Python class over a recording context."""
import os
import re

import numpy as np
import pytest

import factored_oracle as fo
import sourcewise_nonempty_oracle as no
from derivative_oracle import C_POISSON, check_entries, derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ANCHOR, OWN = (3, 2, 4), ((0,), (1, 2), ())
# (bins, listed bins): no entry; a few; exactly one tile and one tile plus a bin; every bin
LISTS = [(63, 0), (63, 5), (1027, 512), (1027, 513), (1001, 1001)]


def small_points(model, rng):
    """points inside a cell, on interior anchors, and on the upper edge of the box (z [d], rs [S])"""
    g = model['anchor_z']
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    pts = [(lo + (hi - lo) * rng.uniform(0.05, 0.95, 3), rng.uniform(0.5, 1.6, 3))]
    on = lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)
    on[0], on[2] = g[0][1], g[2][2]
    pts.append((on, rng.uniform(0.5, 1.6, 3)))
    pts.append((hi.copy(), rng.uniform(0.5, 1.6, 3)))
    return pts


def list_counts(rng, model, z, rs, B, nnz):
    """counts with exactly nnz listed bins; every bin: a Poisson draw at the expectation scaled to 3 events per bin, plus one"""
    if nnz == B:
        mu = fo.expectation(model, z, rs)
        return rng.poisson(mu * (3.0 * B / mu.sum())).astype(float) + 1.0
    return no.sparse_counts(rng, B, nnz)


@pytest.mark.parametrize('B,nnz', LISTS)
def test_specification_against_the_oracle_of_the_expansion(B, nnz):
    """The terms being added are the dense form's -- the non-negative n log mu of the listed bins, the rates, the lgamma sums --
    so cond is the same; the specification must stay below C on the CPU before any device result is held to it."""
    rng = np.random.default_rng(7000 + B + nnz)
    worst, cond_ratio = 0.0, []
    for k in range(2):
        # (where a source has zero bins a listed bin could expect nothing: kept to the model without them here; the -inf of
        # such a bin is a case of its own below)
        model = fo.random_model(rng, N_ANCHOR, OWN, B)
        full = fo.expand(model)
        for z, rs in small_points(model, rng):
            counts = list_counts(rng, model, z, rs, B, nnz)
            got = no.nonempty_derivatives(model, z, rs, counts)
            assert got['nnz'] == nnz
            want = derivatives(full, z, rs, counts, hessian=False)
            worst = max(worst, check_entries(got['ll'], want['ll'], want['ll_cond'], what='ll B=%d nnz=%d' % (B, nnz)))
            worst = max(worst, check_entries(got['grad'], want['grad'], want['grad_cond'], what='grad B=%d nnz=%d' % (B, nnz)))
            dense = fo.factored_derivatives(model, z, rs, counts)
            cond_ratio.append(got['ll_cond'] / dense['ll_cond'])
    print('B = %d, %d listed: worst |err| / (2^-52 cond) = %.3g of C = %d; cond(non-empty) / cond(dense) of ll in [%.3g, %.3g]'
          % (B, nnz, worst, C_POISSON, min(cond_ratio), max(cond_ratio)))


def test_specification_edge_values():
    rng = np.random.default_rng(11)
    model = fo.random_model(rng, N_ANCHOR, OWN, 63)
    for s in range(3):
        model['ps'][s][..., 5] = 0.0
    z, rs = small_points(model, rng)[0]
    counts = no.sparse_counts(rng, 63, 5)
    counts[5] = 0.0
    assert np.isfinite(no.nonempty_derivatives(model, z, rs, counts)['ll'])        # n = 0 where mu = 0: not listed
    hit = counts.copy()
    hit[5] = 2.0
    got = no.nonempty_derivatives(model, z, rs, hit)
    assert got['ll'] == -np.inf and np.isnan(got['grad']).all()                     # a listed bin that expects nothing
    assert derivatives(fo.expand(model), z, rs, hit, hessian=False)['ll'] == -np.inf
    half = counts.copy()
    half[7] = 2.5
    assert no.nonempty_derivatives(model, z, rs, half)['ll'] == -np.inf             # a listed count that is no integer
    # no entry at all: ll = -sum_s lambda_s, the gradient from the row totals alone
    empty = no.nonempty_derivatives(model, z, rs, np.zeros(63))
    mu = fo.expectation(model, z, rs)
    assert abs(empty['ll'] + mu.sum()) <= 1e-12 * mu.sum() and empty['nnz'] == 0


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ['bi_sourcewise_build_nonempty', 'bi_sourcewise_drop_nonempty']


def test_header_binding_and_build_list_agree_on_the_new_symbols():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(bi_[a-z_0-9]+)\s*\(', text))
    build.build()
    lib = _capi.load()
    for s in NEW_SYMBOLS:
        assert 'factored' not in s
        assert s in declared, "%s is not declared in include/blueice_hip.h" % s
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text).group(1)
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.split(',') if a.strip()]), s
    assert 'tu_sourcewise_nonempty' in build.UNITS
    assert os.path.exists(os.path.join(build.CSRC, 'tu_sourcewise_nonempty.hip'))
    # the three parameters, with their access
    import ctypes as C
    n = lib.bi_list_params(None, 0)
    buf = C.create_string_buffer(n)
    lib.bi_list_params(buf, n)
    params = dict(line.split() for line in buf.value.decode().splitlines())
    assert params['sourcewise_nonempty_ready'] == 'r' and params['sourcewise_nonempty_bytes'] == 'r' and params['sourcewise_form'] == 'rw'
    assert not any('factored' in p for p in ('sourcewise_nonempty_ready', 'sourcewise_nonempty_bytes', 'sourcewise_form'))


def test_a_null_context_is_an_error_code_at_both_entry_points():
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    nnz = np.zeros(4, dtype=np.int64)
    assert lib.bi_sourcewise_build_nonempty(None, _capi.ptr(nnz)) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_build_nonempty(None, None) == _capi.ERR_INVALID
    assert lib.bi_sourcewise_drop_nonempty(None) == _capi.ERR_INVALID


# ---- the Python class over a recording context ----------------------------------------------------------------------------

class RecordingContext:
    """Stands where SourceWiseContext would: records uploads, toy calls and builds of the non-empty-bin form; cannot evaluate."""

    def __init__(self, device=None):
        self.T = 0
        self._counts = None
        self.log = []
        self.toy_fill = 0.1                      # the share of bins the 'toys' fill

    def begin_model(self, anchor_z, S, B, own_axes):
        self.d, self.S, self.B = len(anchor_z), S, B

    def set_anchor(self, s, local_index, ps_row, mu):
        pass

    def end_model(self):
        pass

    def set_counts(self, counts):
        c = np.array(counts, float).reshape(-1, self.B)
        self._counts, self.T = c, len(c)
        self.log.append('counts')

    def generate_toys_points(self, z, rate_scale=None, n_toys=1, seed=0):
        n_toys = np.atleast_1d(n_toys)
        self._counts, self.T = None, int(n_toys.sum())
        self.log.append('toys')
        return np.zeros(len(n_toys), dtype=np.int32)

    def build_nonempty(self):
        self.log.append('build')
        if self._counts is not None:
            return np.count_nonzero(self._counts, axis=1).astype(np.int64)
        return np.full(self.T, int(self.toy_fill * self.B), dtype=np.int64)

    def drop_nonempty(self):
        self.log.append('drop')

    def close(self):
        pass


def recorded_likelihood(monkeypatch, **likelihood_config):
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingContext)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False, **likelihood_config))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names[:2]:
        lf.add_shape_parameter(n, (-1., 0., 1.))
    lf.prepare()
    assert isinstance(lf.ctx, RecordingContext)
    return lf


def test_the_default_never_builds(monkeypatch):
    for config in (dict(), dict(nonempty_bins=False)):
        lf = recorded_likelihood(monkeypatch, **config)
        lf.set_binned_data(np.eye(6, 5))
        lf.simulate_toys_points({}, 3, seed=1)
        assert lf.ctx.log == ['counts', 'toys']


def test_true_builds_after_every_change_of_the_counts(monkeypatch):
    lf = recorded_likelihood(monkeypatch, nonempty_bins=True)
    lf.set_binned_data(np.ones((6, 5)))                       # every bin filled: True builds all the same
    assert lf.ctx.log == ['counts', 'build']
    lf.simulate_toys_points({}, 3, seed=1)
    assert lf.ctx.log == ['counts', 'build', 'toys', 'build'] and lf.ctx.T == 3
    lf.set_binned_data(np.zeros((2, 6, 5)))
    assert lf.ctx.log[-2:] == ['counts', 'build']


def test_auto_builds_exactly_up_to_a_quarter_of_the_bins(monkeypatch):
    lf = recorded_likelihood(monkeypatch, nonempty_bins='auto')
    B = 30
    for filled, T in ((0, 1), (7, 1), (8, 1), (15, 2), (16, 2), (30, 1)):
        counts = np.zeros((T, B))
        counts.reshape(-1)[:filled] = 2.0                     # `filled` bins of all T datasets together
        lf.ctx.log.clear()
        lf.set_binned_data(counts.reshape(T, 6, 5))
        want = 4 * filled <= T * B
        assert lf.ctx.log == (['counts', 'build'] if want else ['counts']), (filled, T)
    # toys exist on the device only: the build counts them, and the form is dropped again where they are too dense
    for fill, want in ((0.1, ['toys', 'build']), (0.5, ['toys', 'build', 'drop'])):
        lf.ctx.log.clear()
        lf.ctx.toy_fill = fill
        lf.simulate_toys_points({}, 4, seed=2)
        assert lf.ctx.log == want, fill
    lf.config['nonempty_bins'] = 'sometimes'
    with pytest.raises(ValueError, match='nonempty_bins'):
        lf.set_binned_data(np.zeros((6, 5)))
