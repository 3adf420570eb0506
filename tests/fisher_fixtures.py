"""Models and points shared by tests/test_fisher_host.py and tests/test_fisher_gpu.py: golden fixtures with d = 0 .. 3 (one
with non-uniform anchors, one cut down to a single-anchor axis) and the points at which every one is evaluated -- inside
cells, on anchors, on the box's upper edge, with a rate scale of 0.  Test infrastructure only."""
import numpy as np

from golden_util import load_case

FIXTURES = ['d0_multi_source', 'c1_like', 'd2_nonuniform', 'd3_small', 'd2_single_anchor']


def fixture_model(name):
    """-> the oracle's model dict (anchor_z, ps [*anchors, S, *bins], mus [*anchors, S])"""
    if name == 'd2_single_anchor':          # d2_nonuniform with its second axis cut down to the anchor at 1.0
        m = load_case('d2_nonuniform')['model']
        return dict(anchor_z=[np.asarray(m['anchor_z'][0], dtype=float), np.array([1.0])], ps=np.ascontiguousarray(m['ps'][:, 1:2]),
                    mus=np.ascontiguousarray(m['mus'][:, 1:2]), n_model=None)
    m = load_case(name)['model']
    return dict(anchor_z=[np.asarray(g, dtype=float) for g in m['anchor_z']], ps=np.asarray(m['ps'], dtype=float),
                mus=np.asarray(m['mus'], dtype=float), n_model=None)


def fixture_points(name):
    """-> (z [8, d], rate_scale [8, S]): three points inside cells, one with every axis on an anchor (an interior one where
    there is one), one on the box's upper edge, one on the lower edge, one mixed (first axis on an anchor, the others inside),
    and an interior point again with the first rate scale 0"""
    model = fixture_model(name)
    grids = model['anchor_z']
    d, S = len(grids), model['mus'].shape[-1]
    rng = np.random.default_rng(17 + FIXTURES.index(name))

    def inside(g):
        return float(g[0]) if len(g) < 2 else float(rng.uniform(g[0], g[-1]))
    zs = [[inside(g) for g in grids] for _ in range(3)]
    zs.append([float(g[len(g) // 2]) for g in grids])
    zs.append([float(g[-1]) for g in grids])
    zs.append([float(g[0]) for g in grids])
    zs.append([float(g[(len(g) - 1) // 2]) if i == 0 else inside(g) for i, g in enumerate(grids)])
    zs.append([inside(g) for g in grids])
    rs = rng.uniform(0.4, 1.6, size=(len(zs), S))
    rs[-1, 0] = 0.0
    return np.array(zs, dtype=float).reshape(len(zs), d), rs


def synthetic_model(rng, d, S, B, anchors=(-1.0, 0.25, 1.0), holes=True):
    """Random templates on d axes of the given anchors, S sources, B bins.  holes: a few bins that only SOME anchors or only
    SOME sources fill (zeros elsewhere) and one bin nothing fills, where B allows it"""
    grids = [np.array(anchors, dtype=float) for _ in range(d)]
    shape = tuple(len(g) for g in grids)
    ps = rng.uniform(0.1, 1.0, size=shape + (S, B))
    if holes and B >= 8:
        ps[..., B // 3] = 0.0                                    # nothing is expected here, whatever the parameters
        ps[..., 1:, B // 2] = 0.0                                # only source 0 fills this one
        if d:
            ps[(0,) + (slice(None),) * (d - 1) + (slice(None), B // 5)] = 0.0      # the first anchor of axis 0 leaves this one empty
            ps[(slice(1, None),) + (slice(None),) * (d - 1) + (slice(None), B - 2)] = 0.0      # only the first anchor of axis 0 fills this one
    ps /= ps.sum(axis=-1, keepdims=True)
    mus = rng.uniform(20.0, 60.0, size=shape + (S,))
    return dict(anchor_z=grids, ps=ps, mus=mus, n_model=None)


def synthetic_points(rng, model, n):
    """n points: inside cells, then one on interior anchors, one on the upper edge; rate scales in (0.4, 1.6), the last
    point's first one 0"""
    grids = model['anchor_z']
    d, S = len(grids), model['mus'].shape[-1]
    zs = [[float(rng.uniform(g[0], g[-1])) for g in grids] for _ in range(n)]
    if n >= 3:
        zs[-2] = [float(g[len(g) // 2]) for g in grids]
        zs[-3] = [float(g[-1]) for g in grids]
    rs = rng.uniform(0.4, 1.6, size=(n, S))
    rs[-1, 0] = 0.0
    return np.array(zs, dtype=float).reshape(n, d), rs
