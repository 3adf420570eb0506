"""OracleLikelihood with toys, for CPU tests of the toy-MC drivers (toy_test_statistics): `simulate_toys` draws numpy
Poisson counts -- toy D = toy_offset + t of a seed from its own generator, as the device numbers its toys --, `eval_points`
takes a `dataset` per point, and a small stand-in for the device context keeps toy_offset and hands the resident counts out.
Test infrastructure only: nothing in the package imports it."""
import numpy as np

from oracle import blueice_oracle as orc
from oracle_lf import OracleLikelihood


class _Context:
    def __init__(self, lf):
        self.lf, self.params = lf, {'toy_offset': 0}
        self.offsets_seen = []

    def set_param(self, name, value):
        self.params[name] = value
        if name == 'toy_offset':
            self.offsets_seen.append(int(value))

    def get_param(self, name):
        return self.params[name]

    @property
    def T(self):
        return len(self.lf.datasets)

    def download_counts(self, t=0):
        return self.lf.datasets[t].ravel().copy()


class OracleToysLikelihood(OracleLikelihood):
    def __init__(self, model, counts, shape_names):
        OracleLikelihood.__init__(self, model, counts, shape_names)
        self.bin_shape = self.counts.shape
        self.datasets = self.counts[None]                       # [T, *bins]
        self.is_data_set = True
        self.ctx = _Context(self)
        self.toy_numbers = None                                 # the numbers D of the resident toys
        self.n_restored = 0

    def __getattr__(self, name):
        """the inference helpers as methods, as on the package's likelihoods"""
        from blueice_amd import inference
        if name in inference.__all__:
            import functools
            return functools.partial(getattr(inference, name), self)
        raise AttributeError(name)

    def set_binned_data(self, counts):
        counts = np.asarray(counts, dtype=float)
        self.datasets = counts.reshape((-1,) + tuple(self.bin_shape))
        self.counts = self.datasets[0]
        self.toy_numbers = None
        self.n_restored += 1

    def expectation(self, **truth):
        z, r = self._arrays({k: np.array([v]) for k, v in truth.items()})
        mus = orc.interpolate(self.model['anchor_z'], self.model['mus'], z[0]) if len(self.shape_parameters) else self.model['mus']
        ps = orc.interpolate(self.model['anchor_z'], self.model['ps'], z[0]) if len(self.shape_parameters) else self.model['ps']
        return ((mus * r[0]) @ ps.reshape(self.S, -1)).reshape(self.bin_shape)

    def toy(self, seed, number, **truth):
        return np.random.default_rng([int(seed), int(number)]).poisson(self.expectation(**truth)).astype(float)

    def simulate_toys(self, n_toys, seed=0, livetime_days=None, **truth):
        first = self.ctx.get_param('toy_offset')
        self.toy_numbers = first + np.arange(n_toys)
        self.datasets = np.stack([self.toy(seed, D, **truth) for D in self.toy_numbers])
        self.counts = self.datasets[0]

    def eval_points(self, points, livetime_days=None, dataset=None):
        if dataset is None:
            return OracleLikelihood.eval_points(self, points)
        z, r = self._arrays(points)
        P = max(len(z), np.size(dataset))
        z, r, dataset = np.broadcast_to(z, (P, z.shape[1])), np.broadcast_to(r, (P, r.shape[1])), np.broadcast_to(np.asarray(dataset), (P,))
        self.n_batches += 1
        self.n_calls += len(z)
        out = np.empty(len(z))
        for t in np.unique(dataset):
            rows = dataset == t
            out[rows] = orc.loglikelihood_batch(self.model, self.datasets[t], z[rows], r[rows])
        return out
