"""The walk of the tiled toy-MC dot kernels (k_dataset_dot_tiled, k_dataset_dot_multi: csrc/bi_k_toys.h) where a block's rings of
offsets and entries WRAP: a block walks its datasets in steps of 1024 / L rows through a ring of six steps, so it wraps once it
has more than 6 * 1024 / L datasets -- which only the workload-sized tests reached.  One wide, thin model (S = 2, two anchors,
about 2400 non-empty bins per dataset) whose tile count reaches the resident blocks, so that ONE block walks all 3100 datasets
of its tile (by = 1), for every lane count L and both entry widths.  The data hold
  * tiles in which no dataset has an entry (empty runs), and the tiles around them;
  * a tile with ~300 entries per dataset: runs longer than the (16 / W) L AHEAD <= 128 slots requested up front (the tail loop);
  * 3100 datasets: no multiple of the 64 ... 512 rows of a step;
  * a last tile that holds a single bin.
Against the NumPy / scipy oracle (1e-10), the row kernel (dot_tiled = 0: 1e-13) and, bitwise, a repeated call and a sub-range of
the datasets (other slices of the same rings), as tests/test_toys_gpu.py::test_tiled_dataset_kernel_random_shapes has them."""
import numpy as np
import pytest
from scipy import stats

pytestmark = pytest.mark.gpu

T = 3100                       # > 6 * 1024 / 2: the rings wrap for every L
Z, RS = 0.3, np.array([1.3, 0.8])
LOOK = (0, 1, 2, 3, 1500, 1501, T - 2, T - 1)          # the datasets held against the oracle


class Wide:
    """the model, its toys on the device, the oracle's values for the datasets LOOK and the row kernel's for all"""

    def __init__(self, n_tiles, tile):
        from blueice_amd.device import DeviceContext
        self.tile = tile
        self.B = B = n_tiles * tile + 1                               # the last tile holds ONE bin
        rng = np.random.default_rng(n_tiles)
        back = rng.random(B) + 0.5                                    # source 0: everywhere ...
        self.empty = (3 * 8192, 4 * 8192)
        back[self.empty[0]:self.empty[1]] = 0.0                       # ... but for 8192 bins: runs without an entry
        back[B - 1] = 0.0
        back *= 2100.0 / back.sum()
        back[B - 1] = 0.7                                             # the single bin of the last tile
        self.hot = (10 * 8192, 10 * 8192 + 4096)
        peak = np.zeros(B)                                            # source 1: ~300 events in half a tile of 8192 (one of 4096)
        peak[self.hot[0]:self.hot[1]] = rng.random(4096) + 0.5
        peak *= 300.0 / peak.sum()
        f = np.stack([np.stack([back, peak]), np.stack([0.9 * back, 1.2 * peak])])      # [anchor][source][bin]
        self.mus = f.sum(axis=2)
        self.ps = f / self.mus[:, :, None]
        self.ctx = ctx = DeviceContext(0)
        ctx.upload_model([np.array([0.0, 1.0])], self.ps, self.mus)
        ctx.set_param('compact_budget', 1024)                         # (no compacted rows: only the toy-MC form is used)
        ctx.generate_toys([Z], None, T, seed=4242 + n_tiles)
        self.nnz = ctx.get_param('nnz_total')
        self.counts = {t: ctx.download_counts(t) for t in LOOK}
        self._oracle = {}
        self.want = {t: self.oracle(Z, RS, t) for t in LOOK}
        ctx.set_param('dot_tiled', 0)
        self.rows, st = ctx.eval_datasets([Z], RS)
        ctx.set_param('dot_tiled', 1)
        assert st == 0 and np.all(np.isfinite(self.rows))

    def oracle(self, z, rs, t):
        """log L of dataset t (one of LOOK) at (z, rs); computed once"""
        key = (float(z), tuple(float(x) for x in rs), t)
        if key not in self._oracle:
            w = np.array([1.0 - z, z])
            rate = (w[:, None] * self.mus).sum(axis=0) * rs           # both linear in z, as the reference interpolates them
            pdf = (w[:, None, None] * self.ps).sum(axis=0)
            self._oracle[key] = float(np.sum(stats.poisson((rate[:, None] * pdf).sum(axis=0)).logpmf(self.counts[t])))
        return self._oracle[key]

    def check_data(self, slots):
        """the cases the walk has to get right are in the data (and in the datasets held against the oracle)"""
        looked = np.stack([self.counts[t] for t in LOOK])
        assert self.B % self.tile == 1 and looked[:, -1].sum() > 0                            # the single bin of the last tile is in use
        assert looked[:, self.empty[0]:self.empty[1]].sum() == 0                              # empty runs
        assert np.all((looked[:, self.hot[0]:self.hot[1]] > 0).sum(axis=1) > slots)           # runs beyond the slots requested up front
        assert looked.max() <= 7                                                              # (two-byte entries can hold the counts)


@pytest.fixture(scope='module')
def single():
    w = Wide(128, 8192)                                               # B = 128 * 8192 + 1: 129 tiles of the single-point lists
    yield w
    w.ctx.close()


@pytest.fixture(scope='module')
def multi():
    w = Wide(129, 4096)                                               # B = 129 * 4096 + 1: 130 tiles of the multi-point lists
    yield w
    w.ctx.close()


@pytest.mark.parametrize('width,lanes', [(2, 0), (2, 8), (4, 0), (4, 16)])     # <4, 3, 2>, <8, 2, 2>, <8, 3, 4>, <16, 2, 4>
def test_single_point_walk_over_wrapping_rings(single, width, lanes):
    w, ctx = single, single.ctx
    n_tl = (w.B + 8191) // 8192
    assert n_tl == 129 and w.nnz >= 16 * T * n_tl                     # the gates of the tiled kernel: n_tl >= 4, entries per tile
    w.check_data(128)
    ctx.set_param('dot_blocks_per_cu', 1)                             # one resident block per CU < 129 tiles: by = 1, a block walks all T
    ctx.set_param('dot_entry16', 1 if width == 2 else 0)
    ctx.set_param('dot_lanes', lanes)
    try:
        polled = ctx.get_param('n_toy_polled')
        ll, st = ctx.eval_datasets([Z], RS)
        assert st == 0 and ctx.get_param('tm_entry_bytes') == width
        assert ctx.get_param('n_toy_polled') == polled + 1            # the tiled kernels took the call (and published its word)
        np.testing.assert_allclose(ll, w.rows, rtol=1e-13, atol=0)
        np.testing.assert_allclose(ll[list(LOOK)], [w.want[t] for t in LOOK], rtol=1e-10)
        again, _ = ctx.eval_datasets([Z], RS)
        np.testing.assert_array_equal(again, ll)
        for lo, hi in ((1, T), (517, 517 + 1537), (T - 64, T)):       # other slices: other ring positions, the same sums
            part, _ = ctx.eval_datasets([Z], RS, lo, hi)
            np.testing.assert_array_equal(part, ll[lo:hi])
    finally:
        ctx.set_param('dot_lanes', 0)
        ctx.set_param('dot_entry16', 1)
        ctx.set_param('dot_blocks_per_cu', 0)


@pytest.mark.parametrize('width,lanes,pp', [(2, 2, 0), (2, 4, 0), (2, 8, 0), (4, 4, 0), (4, 8, 0), (2, 4, 2), (4, 8, 2)])
def test_multi_point_walk_over_wrapping_rings(multi, width, lanes, pp):
    w, ctx = multi, multi.ctx
    n_tl = (w.B + 4095) // 4096
    assert n_tl == 130 and w.nnz >= 8 * T * n_tl                      # the gates of the multi-point kernels
    w.check_data(64)
    z = np.array([[Z], [Z], [0.0], [0.85], [Z]])                      # five points of the one cell: two passes of four (or three of two)
    rs = np.array([RS, [0.5, 2.0], [1.0, 1.0], [1.1, 0.0], [2.0, 1.0]])
    ctx.set_param('dot_entry16', 1 if width == 2 else 0)
    ctx.set_param('toy_points_lanes', lanes)
    ctx.set_param('toy_points_pp', pp)
    try:
        before = ctx.get_param('n_toy_points_passes')
        ll, st = ctx.eval_datasets_points(z, rs)
        assert not st.any() and ctx.get_param('tmm_entry_bytes') == width
        assert ctx.get_param('n_toy_points_passes') == before + (3 if pp == 2 else 2)     # the multi-point kernels took the call
        np.testing.assert_allclose(ll[0], w.rows, rtol=1e-13, atol=0)
        ctx.set_param('dot_tiled', 0)                                 # point by point through the row kernel
        rows, _ = ctx.eval_datasets_points(z, rs)
        ctx.set_param('dot_tiled', 1)
        np.testing.assert_allclose(ll, rows, rtol=1e-13, atol=0)
        for p in range(len(z)):
            want = [w.oracle(z[p, 0], rs[p], t) for t in LOOK[::3]]
            np.testing.assert_allclose(ll[p, list(LOOK[::3])], want, rtol=1e-10)
        again, _ = ctx.eval_datasets_points(z, rs)
        np.testing.assert_array_equal(again, ll)
        for lo, hi in ((1, T), (517, 517 + 1537), (T - 64, T)):
            part, _ = ctx.eval_datasets_points(z, rs, lo, hi)
            np.testing.assert_array_equal(part, ll[:, lo:hi])
    finally:
        ctx.set_param('toy_points_pp', 0)
        ctx.set_param('toy_points_lanes', 0)
        ctx.set_param('dot_entry16', 1)
