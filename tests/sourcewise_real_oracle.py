"""Inputs and oracle of the real-valued layer of source-wise models (test_sourcewise_real_gpu.py on the device,
test_sourcewise_real_host.py on the CPU).  No test lives here.

The models and truths are sourcewise_toy_cases'.  The oracle of bi_eval_sourcewise_real is real_counts_oracle.point on
factored_oracle.expand(model) -- the same likelihood on the full tensor-product grid, which bi_eval_real is held to -- with the
per-bin expectation cross-checked against sourcewise_toy_cases.exact_expectation (long double): where that is exactly 0 and the
dataset has an event, the value is +inf."""
import numpy as np

import factored_oracle as fo
import real_counts_oracle as rco
import sourcewise_toy_cases as cases

ST_OUT_OF_BOUNDS, ST_UNPHYSICAL = rco.ST_OUT_OF_BOUNDS, rco.ST_UNPHYSICAL
N_LIVE = 7                              # the batch of live points; two rejected ones follow it


def real_datasets(name, model, z, rs):
    """Real-valued datasets [T, B] >= 0 of a case: truth t's expectation times a factor in (0.4, 1.7) per bin, a quarter of the
    bins at exactly 0.  `zero_both_sides` gets a fourth: dataset 0 with an event in a bin where every source is zero."""
    rng = np.random.default_rng(sum(name.encode()) + 9100)
    B = fo.n_bins(model)
    out = []
    for t in range(3):
        n = fo.expectation(model, z[t], rs[t]) * rng.uniform(0.4, 1.7, B)
        if B > 1:
            n[rng.permutation(B)[:max(1, B // 4)]] = 0.0
        out.append(n)
    if name == 'zero_both_sides':
        hit = out[0].copy()
        hit[cases.ZERO_BINS[3]] = 0.75
        out.append(hit)
    counts = np.stack(out)
    assert np.all(counts >= 0) and np.all(np.isfinite(counts)) and (B == 1 or np.count_nonzero(counts[0] == 0) >= B // 4)
    return counts


def points_of(name, model, n_sets):
    """-> (z [9, d], rs [9, S], ds [9]): N_LIVE points inside the box (the last on its upper edge), one outside it, one with a
    negative rate; the datasets in turn"""
    rng = np.random.default_rng(sum(name.encode()) + 9200)
    z, rs = cases.box_points(model, rng, N_LIVE)
    z = np.concatenate([z, z[:2]])
    rs = np.concatenate([rs, rs[:2]])
    z[N_LIVE, -1] = model['anchor_z'][-1][-1] + 0.25
    rs[N_LIVE + 1, 0] = -0.5
    return z, rs, np.arange(len(z), dtype=np.int64) % n_sets


def want_point(model, full, counts, z, rs):
    """real_counts_oracle.point on the expansion, its expectation checked against the long-double one"""
    w = rco.point(full, counts, z, rs)
    if w['mu'] is not None:
        exact = cases.exact_expectation(model, z, rs)[0]
        assert np.all(np.abs(w['mu'] - exact.astype(float)) <= 1e-13 * np.maximum(1.0, exact.astype(float)))
        if np.any((np.asarray(counts) > 0) & (exact == 0)):
            assert w['half_deviance'] == np.inf
    return w


def likelihoods(model, device=0):
    """The source-wise likelihood of `model` and the plain BinnedLogLikelihood of the same sources on the full grid, through the
    ordinary config -> Model -> prepare() route from one Source class (as test_factored_gpu.tensor_likelihoods); every source has
    a rate parameter, every axis is a shape parameter, no priors, NO data."""
    from blueice_amd import BinnedLogLikelihood, SourceWiseBinnedLogLikelihood
    from blueice_amd.source import Source
    d, S, B = len(model['anchor_z']), len(model['own']), fo.n_bins(model)
    names = ['shape%d' % i for i in range(d)]

    class TensorSource(Source):
        def __init__(self, config, *args, **kwargs):
            m, s = config['tensor_model'], config['source_index']
            idx = tuple(int(np.flatnonzero(np.asarray(m['anchor_z'][i]) == float(config[names[i]]))[0]) for i in m['own'][s])
            self._row = np.asarray(m['ps'][s])[idx]
            super().__init__(dict(config, events_per_day=float(np.asarray(m['mus'][s])[idx]), livetime_days=1), *args, **kwargs)

        def get_pmf_grid(self):
            return self._row.copy(), np.full(self._row.shape, np.inf)

    out = []
    for cls in (SourceWiseBinnedLogLikelihood, BinnedLogLikelihood):
        conf = dict(analysis_space=[('x', np.arange(B + 1, dtype=float))], default_source_class=TensorSource, tensor_model=model,
                    sources=[dict(name='s%d' % s, source_index=s,
                                  extra_dont_hash_settings=[n for i, n in enumerate(names) if i not in model['own'][s]]) for s in range(S)],
                    **{n: float(g[0]) for n, g in zip(names, model['anchor_z'])})
        lf = cls(conf, likelihood_config=dict(device=device, device_histograms=False))
        for s in range(S):
            lf.add_rate_parameter('s%d' % s)
        for n, g in zip(names, model['anchor_z']):
            lf.add_shape_parameter(n, tuple(float(v) for v in g))
        lf.prepare()
        out.append(lf)
    return out
