"""Gridded likelihoods without a GPU: the host engine of blueice_amd.grid (the executable specification of bi_grid_reduce)
against brute force over a duck-typed NumPy likelihood, the trapezoid weights, the posterior and credible limit against
NumPy trapezoid sums of a known density, the argument errors, and the refusals that come before any device work."""
import numpy as np
import pytest
from scipy.special import logsumexp

from blueice_amd.grid import GridResult, grid_scan, reduce_cells, trapezoid_weights


class NumpyLikelihood:
    """log L = a correlated Gaussian in (a, b, c), zero likelihood for b < -1 and nan at c == 7; counts its calls"""

    def __init__(self):
        self.calls = self.points = 0

    def value(self, a, b, c):
        with np.errstate(invalid='ignore'):
            ll = -0.5 * ((a - 1.0) ** 2 / 0.3 + (b - 0.2 * a) ** 2 / 0.5 + (c + b) ** 2 / 2.0) - 3.0
            ll = np.where(c == 7.0, np.nan, ll)
            return np.where(b < -1.0, -np.inf, ll)

    def eval_points(self, points, livetime_days=None):
        unknown = set(points) - {'a', 'b', 'c'}
        if unknown:
            raise KeyError(sorted(unknown))
        n = max(np.size(v) for v in points.values())
        a, b, c = (np.broadcast_to(np.asarray(points.get(k, 0.0), dtype=float), (n,)) for k in 'abc')
        self.calls += 1
        self.points += n
        return self.value(a, b, c)


A = np.array([0.0, 0.4, 1.0, 1.1, 2.5])
B = np.array([-1.5, -1.0, -0.3, 0.0, 0.1, 0.7, 2.0])
C = np.linspace(-3.0, 3.0, 9)


def brute(lf, n_keep, weights):
    axes = [A, B, C]
    mesh = np.meshgrid(*axes, indexing='ij')
    t = lf.value(*mesh)
    K = int(np.prod(t.shape[:n_keep]))
    t = t.reshape(K, -1)
    if weights is None:
        q = np.zeros(t.shape[1])
    else:
        ws = np.meshgrid(*[np.log(w) for w in weights], indexing='ij') if weights else []
        q = sum(ws).reshape(-1) if ws else np.zeros(1)
    lm, prof, arg = np.empty(K), np.empty(K), np.empty(K, dtype=np.int64)
    for k in range(K):
        ok = t[k] > -np.inf
        lm[k] = logsumexp((t[k] + q)[ok]) if ok.any() else -np.inf
        prof[k] = t[k][ok].max() if ok.any() else -np.inf
        arg[k] = np.flatnonzero(ok & (t[k] == prof[k]))[0] if ok.any() else -1
    return lm, prof, arg, int((t == -np.inf).sum())


@pytest.mark.parametrize('n_keep', [0, 1, 2, 3])
@pytest.mark.parametrize('weights', ['trapezoid', None, 'arrays'])
@pytest.mark.parametrize('chunk', [None, 1, 7, 100])
def test_host_engine_against_brute_force(n_keep, weights, chunk):
    lf = NumpyLikelihood()
    axes = [('a', A), ('b', B), ('c', C)]
    rng = np.random.default_rng(n_keep)
    if weights == 'arrays':
        w = [rng.uniform(0.0, 2.0, len(v)) for _, v in axes[n_keep:]]
        if w:
            w[0][0] = 0.0                        # a weight of zero: out of the marginal, still in the profile
        given = w
    elif weights == 'trapezoid':
        w, given = [trapezoid_weights(v) for _, v in axes[n_keep:]], 'trapezoid'
    else:
        w = given = None
    res = grid_scan(lf, keep=axes[:n_keep], reduce=axes[n_keep:], weights=given, chunk=chunk)
    with np.errstate(divide='ignore'):
        lm, prof, arg, excluded = brute(lf, n_keep, w)
    shape = tuple(len(v) for _, v in axes[:n_keep])
    assert res.engine == 'host' and res.log_marginal.shape == res.profile.shape == res.argmax.shape == shape
    assert res.excluded == excluded == res.counters[2] and res.counters[1] == lf.points == 5 * 7 * 9
    assert res.counters[0] == lf.calls == -(-315 // (chunk or 1 << 16))
    assert np.array_equal(res.profile.ravel(), prof) and np.array_equal(res.argmax.ravel(), arg)
    fin = np.isfinite(lm)
    assert np.array_equal(np.isfinite(res.log_marginal.ravel()), fin)
    assert np.all(np.abs(res.log_marginal.ravel()[fin] - lm[fin]) <= 1e-12 * np.maximum(1.0, np.abs(lm[fin])))
    assert np.all(res.log_marginal.ravel()[~fin] == -np.inf)
    # where the maximum sits
    at = np.unravel_index(np.maximum(arg, 0), tuple(len(v) for _, v in axes[n_keep:])) if n_keep < 3 else ()
    for (name, nodes), i in zip(axes[n_keep:], at):
        want = np.where(arg >= 0, nodes[i], np.nan).reshape(shape)
        assert np.array_equal(res.best[name], want, equal_nan=True)
    assert np.array_equal(res.likelihood_ratio(), np.max(res.profile) - res.profile)


def test_empty_cells_and_nan_cells():
    lf = NumpyLikelihood()
    res = grid_scan(lf, keep=[('b', B)], reduce=[('a', A), ('c', np.array([-1.0, 7.0, 2.0]))], weights=None)
    assert np.all(np.isnan(res.log_marginal[1:])) and np.all(np.isnan(res.profile[1:])) and np.all(res.argmax[1:] == -1)
    assert res.log_marginal[0] == res.profile[0] == -np.inf and res.argmax[0] == -1          # b = -1.5: no point left
    assert res.excluded == 15 and np.isnan(res.best['a'][0]) and np.isnan(res.best['c'][3])
    lm, prof, arg, n = reduce_cells(np.array([[-np.inf, -np.inf], [1.0, 1.0], [np.nan, 0.0], [-np.inf, 2.0]]), np.array([0.0, -np.inf]))
    assert np.array_equal(lm, [-np.inf, 1.0, np.nan, -np.inf], equal_nan=True)
    assert np.array_equal(prof, [-np.inf, 1.0, np.nan, 2.0], equal_nan=True) and list(arg) == [-1, 0, -1, 1] and n == 3


def test_datasets_axis_leads():
    class Stack(NumpyLikelihood):
        def eval_points(self, points, livetime_days=None, dataset=None):
            return NumpyLikelihood.eval_points(self, points) + 10.0 * np.asarray(dataset)
    lf = Stack()
    one = grid_scan(NumpyLikelihood(), keep=[('a', A)], reduce=[('c', C)], b=0.3)
    res = grid_scan(lf, keep=[('a', A)], reduce=[('c', C)], datasets=[2, 0, 1], b=0.3)
    assert res.profile.shape == (3, 5) and res.best['c'].shape == (3, 5)
    for e, t in enumerate([2, 0, 1]):
        assert np.allclose(res.profile[e], one.profile + 10.0 * t, rtol=0, atol=1e-12)
        assert np.allclose(res.log_marginal[e], one.log_marginal + 10.0 * t, rtol=0, atol=1e-12)
        assert np.array_equal(res.argmax[e], one.argmax)
    assert np.allclose(res.likelihood_ratio(), np.broadcast_to(one.likelihood_ratio(), (3, 5)), rtol=0, atol=1e-12)
    assert res.credible_upper_limit(0.9).shape == (3,)


def test_trapezoid_weights():
    assert np.array_equal(trapezoid_weights([2.0]), [1.0])
    assert np.array_equal(trapezoid_weights([0.0, 1.0]), [0.5, 0.5])
    x = np.array([0.0, 1.0, 3.0, 3.5, 7.0])
    w = trapezoid_weights(x)
    assert np.array_equal(w, [0.5, 1.5, 1.25, 2.0, 1.75])
    y = np.sin(x) + 2
    assert abs(w @ y - np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(x))) <= 1e-14
    for bad in ([0.0, 0.0, 1.0], [1.0, 0.0], [0.0, 2.0, 1.0]):
        with pytest.raises(ValueError, match='ascending'):
            trapezoid_weights(bad)
    with pytest.raises(ValueError, match='ascending nodes \\(c\\)'):
        grid_scan(NumpyLikelihood(), keep=[('a', A)], reduce=[('c', C[::-1])])
    grid_scan(NumpyLikelihood(), keep=[('a', A[::-1])], reduce=[('c', C[::-1])], weights=None)      # any order without the rule


def result_of(x, log_density, lead=False):
    lm = np.asarray(log_density, dtype=float)
    return GridResult([('x', x)], [], lm, lm.copy(), np.zeros(lm.shape, dtype=np.int64), 0, 'host', np.zeros(4, dtype=np.int64), lead)


def test_posterior_and_credible_limit_against_trapezoid_sums():
    x = np.concatenate([np.linspace(0.0, 2.0, 23), [2.5, 3.1, 4.0, 6.0, 9.0]])
    dens = x ** 2 * np.exp(-1.7 * x) + 0.01                        # any positive density: the rule itself is under test
    res = result_of(x, np.log(dens) - 123.0)
    norm = np.sum(0.5 * (dens[1:] + dens[:-1]) * np.diff(x))
    assert np.all(np.abs(res.posterior() - dens / norm) <= 1e-9)
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(x))]) / norm
    for cl in (0.05, 0.5, 0.9, 0.95, 0.999):
        i = np.searchsorted(cdf, cl)
        want = x[i - 1] + (cl - cdf[i - 1]) / (cdf[i] - cdf[i - 1]) * (x[i] - x[i - 1])
        assert abs(res.credible_upper_limit(cl) - want) <= 1e-9
    # nodes of zero posterior, and a leading dataset axis
    with np.errstate(divide='ignore'):
        two = result_of(x, np.stack([np.log(dens), np.log(np.where(x > 3, 0.0, dens))]), lead=True)
    assert two.posterior().shape == (2, len(x)) and np.all(two.posterior()[1][x > 3] == 0)
    lim = two.credible_upper_limit(0.9)
    assert abs(lim[0] - res.credible_upper_limit(0.9)) <= 1e-9 and lim[1] < lim[0]
    with pytest.raises(ValueError, match='cl must lie'):
        res.credible_upper_limit(1.0)
    both = GridResult([('x', x), ('y', x)], [], np.zeros((28, 28)), np.zeros((28, 28)), np.zeros((28, 28), dtype=np.int64), 0, 'host', None, False)
    for method in (both.posterior, both.credible_upper_limit, result_of(x[::-1], np.log(dens)).posterior, result_of(x[:1], [0.0]).posterior):
        with pytest.raises(ValueError, match='exactly one kept axis'):
            method()


def test_argument_errors_come_before_any_evaluation():
    lf = NumpyLikelihood()
    ax = [('a', A)]
    cases = [(dict(), 'at least one axis'),
             (dict(keep=ax, reduce=ax), 'only once'),
             (dict(keep=ax, a=1.0), 'only once'),
             (dict(keep=[('a', [])]), 'non-empty'),
             (dict(keep=[('a', [[1.0, 2.0]])]), 'one-dimensional'),
             (dict(keep=[('a', [0.0, np.inf])]), 'finite'),
             (dict(keep=[('a', [0.0, np.nan])]), 'finite'),
             (dict(keep=['a']), 'list of \\(name, nodes\\)'),
             (dict(keep=ax, engine='gpu'), 'engine must be'),
             (dict(keep=ax, chunk=0), 'chunk must lie'),
             (dict(keep=ax, chunk=2 ** 26 + 1), 'chunk must lie'),
             (dict(keep=ax, reduce=[('c', C)], weights='simpson'), "weights must be 'trapezoid'"),
             (dict(keep=ax, reduce=[('c', C)], weights=[np.ones(3)]), 'one array per reduced axis'),
             (dict(keep=ax, reduce=[('c', C)], weights=[]), 'one array per reduced axis'),
             (dict(keep=ax, reduce=[('c', C)], weights=[-np.ones(9)]), 'finite and >= 0'),
             (dict(keep=ax, datasets=[]), 'non-empty'),
             (dict(keep=[('n%d' % j, [0.0]) for j in range(17)]), 'at most 16 axes'),
             (dict(keep=[('a', np.zeros(4097)), ('b', np.zeros(4097))]), '2\\^24 cells')]
    for kwargs, match in cases:
        with pytest.raises(ValueError, match=match):
            grid_scan(lf, **kwargs)
    assert lf.calls == 0


def test_refusals_before_any_device_work():
    """what is no single device context cannot take the native engine, and says so instead of falling back when asked for it"""
    from blueice_amd.likelihood import LogLikelihoodSum
    lf = NumpyLikelihood()
    with pytest.raises(ValueError, match="engine='host'"):
        grid_scan(lf, keep=[('a', A)], engine='native')
    assert lf.calls == 0
    both = LogLikelihoodSum.__new__(LogLikelihoodSum)          # (no device is touched: the refusal looks at the type only)
    with pytest.raises(ValueError, match="engine='host'"):
        both.grid_scan(keep=[('a', A)], engine='native')
    assert grid_scan(lf, keep=[('a', A)], engine=None).engine == 'host'
    import blueice_amd
    assert blueice_amd.grid_scan is grid_scan and blueice_amd.GridResult is GridResult
    for cls in (blueice_amd.BinnedLogLikelihood, blueice_amd.UnbinnedLogLikelihood, blueice_amd.LogLikelihoodSum,
                blueice_amd.LogLikelihoodReParam, blueice_amd.LogAncillaryLikelihood):
        assert cls.grid_scan is grid_scan
