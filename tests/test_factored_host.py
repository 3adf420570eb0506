"""Source-wise (factored) models without a GPU: the NumPy specification against the exact oracle of the expanded grid, the
Python class over a recording context, and the header / binding of the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import factored_oracle as fo
from derivative_oracle import C_POISSON, check_entries, derivatives

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ANCHOR, OWN = (3, 2, 4), ((0,), (1, 2), ())


def small_points(model, rng):
    """points inside cells, exactly on an interior anchor, and on the upper edge of the box (z [d], rs [S])"""
    g = model['anchor_z']
    lo, hi = np.array([a[0] for a in g]), np.array([a[-1] for a in g])
    pts = [(lo + (hi - lo) * rng.uniform(0.05, 0.95, 3), rng.uniform(0.5, 1.6, 3)) for _ in range(2)]
    on = lo + (hi - lo) * rng.uniform(0.05, 0.95, 3)
    on[0], on[2] = g[0][1], g[2][2]                         # interior anchors of axes 0 and 2
    pts.append((on, rng.uniform(0.5, 1.6, 3)))
    pts.append((hi.copy(), rng.uniform(0.5, 1.6, 3)))       # the closed last cell of every axis
    return pts


@pytest.mark.parametrize('B', [63, 1001])
def test_specification_against_the_oracle_of_the_expansion(B):
    rng = np.random.default_rng(100 + B)
    worst, cond_ratio = 0.0, []
    for k in range(3):
        model = fo.random_model(rng, N_ANCHOR, OWN, B, zero_quarter=(1,) if k else ())
        full = fo.expand(model)
        assert full['ps'].shape == N_ANCHOR + (3, B)
        for z, rs in small_points(model, rng):
            counts = rng.poisson(fo.expectation(model, z, rs)).astype(float)
            got = fo.factored_derivatives(model, z, rs, counts)
            want = derivatives(full, z, rs, counts, hessian=False)
            worst = max(worst, check_entries(got['ll'], want['ll'], want['ll_cond'], what='ll B=%d' % B))
            worst = max(worst, check_entries(got['grad'], want['grad'], want['grad_cond'], what='grad B=%d' % B))
            cond_ratio.append(got['ll_cond'] / want['ll_cond'])
            cond_ratio.extend((got['grad_cond'] / want['grad_cond']).tolist())
    print('B = %d: worst |err| / (2^-52 cond) = %.3g of C = %d; cond(factored) / cond(expanded) in [%.3g, %.3g]'
          % (B, worst, C_POISSON, min(cond_ratio), max(cond_ratio)))


# ---- the Python class over a recording context ----------------------------------------------------------------------

class RecordingSourceWiseContext:
    """Stands where SourceWiseContext would: records uploads, cannot evaluate."""
    instances = []

    def __init__(self, device=None):
        self.device = device
        self.rows = {}
        self.begun = 0
        self.T = 0
        RecordingSourceWiseContext.instances.append(self)

    def begin_model(self, anchor_z, S, B, own_axes):
        self.anchor_z, self.S, self.B, self.own_axes = [np.asarray(g, float) for g in anchor_z], S, B, [tuple(o) for o in own_axes]
        self.rows = {}
        self.begun += 1

    def set_anchor(self, s, local_index, ps_row, mu):
        assert (s, local_index) not in self.rows
        self.rows[(s, local_index)] = (np.array(ps_row, float).reshape(self.B), float(mu))

    def end_model(self):
        self.ended = True

    def set_counts(self, counts):
        self.counts = np.array(counts, float)
        self.T = self.counts.size // self.B

    def close(self):
        pass


def test_prepare_builds_projected_anchors_only(monkeypatch):
    """The example's shape (8 shape parameters x 5 anchors, 4 sources with two own parameters each): Model.__init__ runs once
    for the base model and once per distinct projected anchor (4 x 25), the adapter receives 4 x 25 rows, and nothing walks
    the 5^8 product grid."""
    import blueice_amd.likelihood as lk
    import blueice_amd.pdf_morphers as pm
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    monkeypatch.setattr(sw, 'SourceWiseContext', RecordingSourceWiseContext)
    RecordingSourceWiseContext.instances.clear()
    built, grids = [], []
    real_init = lk.Model.__init__

    def counting_init(self, config, **kw):
        built.append(1)
        real_init(self, config, **kw)

    real_grid = pm.arrays_to_grid

    def counting_grid(arrays):
        out = real_grid(arrays)
        grids.append(out.shape)
        return out

    monkeypatch.setattr(lk.Model, '__init__', counting_init)
    monkeypatch.setattr(pm, 'arrays_to_grid', counting_grid)
    conf, names, own = many_nuisances_config(n_bins=(6, 5))
    lf = sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    for s in range(4):
        lf.add_rate_parameter('s%d' % s)
    for n in names:
        lf.add_shape_parameter(n, (-2., -1., 0., 1., 2.))
    n_before = len(built)
    assert n_before == 1                                     # the base model
    lf.prepare()
    rec = lf.ctx
    assert isinstance(rec, RecordingSourceWiseContext) and rec.begun == 1 and rec.ended
    assert len(built) == 1 + 4 * 25
    assert len(rec.rows) == 4 * 25 and rec.S == 4 and rec.B == 30 and len(rec.anchor_z) == 8
    assert rec.own_axes == [tuple(names.index(k) for k in o) for o in own]
    assert lf.morpher is None and len(lf.anchor_models) == 0
    assert all(int(np.prod(shape[:-1])) <= 25 for shape in grids), grids          # only the sources' own 5 x 5 grids
    # the rows are the sources' own anchors in C order: row (s, a * 5 + b) is source s at its own (z_a, z_b)
    zs = (-2., -1., 0., 1., 2.)
    for s in range(4):
        for a in range(5):
            for b in range(5):
                row, mu = rec.rows[(s, a * 5 + b)]
                src = lf.anchor_sources['s%d' % s][(zs[a], zs[b])]
                np.testing.assert_array_equal(row, src.get_pmf_grid()[0].ravel())
                assert mu == src.expected_events
    lf.set_binned_data(np.ones((6, 5)))
    assert rec.T == 1 and lf.is_data_set
    for name in ('hesse', 'simulate_toys', 'goodness_of_fit', 'asimov', 'fisher_information', 'grid_scan', 'sample_posterior',
                 'expected_coarse'):
        with pytest.raises(NotImplementedError, match='source-wise'):
            getattr(lf, name)()
    with pytest.raises(NotImplementedError, match='source-wise'):
        lf(compute_pdf=True)


def test_limits_and_refusals_of_the_class():
    import blueice_amd.source_wise as sw
    from blueice_amd.synthetic import many_nuisances_config
    conf, names, own = many_nuisances_config(n_bins=(4, 4))
    with pytest.raises(NotImplementedError, match='Beeston-Barlow'):
        sw.SourceWiseBinnedLogLikelihood(conf, likelihood_config=dict(model_statistical_uncertainty_handling='bb_single', bb_single_source=0))
    conf2, _, _ = many_nuisances_config(n_bins=(4, 4))
    conf2['sources'][0]['extra_dont_hash_settings'] = names[4:]          # source 0 now responds to four parameters
    lf = sw.SourceWiseBinnedLogLikelihood(conf2, likelihood_config=dict(device_histograms=False))
    for n in names:
        lf.add_shape_parameter(n, (-1., 0., 1.))
    with pytest.raises(ValueError, match='at most 3'):
        lf.prepare()


def test_header_and_binding_agree_on_the_new_symbols():
    from blueice_amd import _capi, build
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(s for s in set(re.findall(r'\b(bi_[a-z_0-9]+)\s*\(', text)) if 'factored' in s)
    assert declared == ['bi_eval_factored', 'bi_factored_begin', 'bi_factored_end', 'bi_factored_set_anchor', 'bi_factored_set_counts',
                        'bi_fit_batched_factored']
    build.build()
    lib = _capi.load()
    for s in declared:
        assert hasattr(lib, s), "library does not export %s" % s
        assert s in _capi.SIGNATURES, "ctypes binding lacks %s" % s
        # one ctypes argument per declared parameter
        proto = re.search(r'\b%s\s*\(([^)]*)\)' % s, text).group(1)
        assert len(_capi.SIGNATURES[s][1]) == len([a for a in proto.split(',') if a.strip()]), s
    assert _capi.SIGNATURES['bi_fit_batched_factored'] == _capi.SIGNATURES['bi_fit_batched_real']
    assert 'tu_factored' in build.UNITS


def test_a_null_context_is_an_error_code_at_every_fit_and_evaluation_entry_point():
    """No entry point reads the context before it has tested it: bi_fit_batched and its siblings, the source-wise one among
    them, and the source-wise model's own calls return BI_ERR_INVALID for a NULL handle (as after DeviceContext.close())."""
    import ctypes as C
    from blueice_amd import _capi, build
    build.build()
    lib = _capi.load()
    one = np.ones(4)
    i32, i64 = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int64)
    p = _capi.ptr
    fit = (None, 1, 1, p(i32), p(i32), p(one), p(one), p(one), None, p(one), p(one), p(one), None, None, 1e-6, 10)
    out = (p(one.copy()), p(one.copy()), p(i32.copy()), p(i64.copy()))
    assert lib.bi_fit_batched(*fit, *out) == _capi.ERR_INVALID
    for name in ('bi_fit_batched_gauss', 'bi_fit_batched_real', 'bi_fit_batched_factored'):
        assert getattr(lib, name)(*fit, None, None, None, *out) == _capi.ERR_INVALID, name
    assert lib.bi_eval_factored(None, 1, p(one), None, None, p(one.copy()), None, None) == _capi.ERR_INVALID
    assert lib.bi_factored_begin(None, 0, None, None, 1, 4, p(i32), None) == _capi.ERR_INVALID
    assert lib.bi_factored_set_anchor(None, 0, 0, p(one), 1.0) == _capi.ERR_INVALID
    assert lib.bi_factored_end(None) == _capi.ERR_INVALID
    assert lib.bi_factored_set_counts(None, 1, p(one)) == _capi.ERR_INVALID
    assert C.c_void_p().value is None
