"""The host half of the unbinned toy-MC ensembles: the seed of toy D (toy_seed, written out in include/blueice_hip.h at
bi_simulate_event_toys) and the argument checks of `set_datasets` / `simulate_toys` that need no device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# toy_seed(seed, D), computed once with unsigned 64-bit numpy arithmetic from the header's text
TABLE = {
    (0, 0): 0xE220A8397B1DCDAF,
    (0, 1): 0x6E789E6AA1B965F4,
    (12345, 0): 0x22118258A9D111A0,
    (12345, 5): 0x5647E55AD933F62E,
    (4294967295, 4294967296): 0xA512F4AC64AB242C,
    (18446744073709551615, 281474976710655): 0x16F121024A961ED3,
    (9223372036854775808, 7): 0x6250485B3CDEFBBD,
}


def header_toy_seed(seed, D):
    """the header's definition, constants read from the header itself"""
    text = open(os.path.join(ROOT, 'include', 'blueice_hip.h')).read()
    m = re.search(r'toy_seed\(seed, D\):\s+x = seed \+ \(D \+ 1\) (0x[0-9A-F]+);\s+x = \(x \^ x >> (\d+)\) (0x[0-9A-F]+);\s*\*?\s*'
                  r'x = \(x \^ x >> (\d+)\) (0x[0-9A-F]+);\s+toy_seed = x \^ x >> (\d+)', text)
    assert m, "include/blueice_hip.h does not write toy_seed out"
    c0, s1, c1, s2, c2, s3 = m.groups()
    mask = (1 << 64) - 1
    x = (seed + (D + 1) * int(c0, 16)) & mask
    x = ((x ^ (x >> int(s1))) * int(c1, 16)) & mask
    x = ((x ^ (x >> int(s2))) * int(c2, 16)) & mask
    return x ^ (x >> int(s3))


def test_toy_seed_is_the_headers_and_injective():
    from blueice_amd import toy_seed
    for (seed, D), want in TABLE.items():
        assert toy_seed(seed, D) == want == header_toy_seed(seed, D), (seed, D)
        assert toy_seed(seed, D) == toy_seed(seed, D)
    rng = np.random.default_rng(1)
    for seed in (0, 12345, 2 ** 64 - 1):
        Ds = set(range(2000)) | set(int(x) for x in rng.integers(0, 2 ** 48, 20000)) | {2 ** 48 - 1, 2 ** 32 - 1, 2 ** 32}
        assert len({toy_seed(seed, D) for D in Ds}) == len(Ds)
        assert all(0 <= toy_seed(seed, D) < 2 ** 64 for D in list(Ds)[:100])


def histogram_lf():
    import model_zoo
    ns = model_zoo.namespace_of('blueice_amd')
    space = [['x', np.linspace(-4, 4, 9)], ['y', np.array([0., 0.4, 1., 2.2, 3.5, 5., 6.])]]
    conf = dict(sources=[], default_source_class=model_zoo.morphed_source_class(ns), analysis_space=space, force_recalculation=True,
                never_save_to_cache=True, shift=0., stretch=0., tilt=0.)
    rng = np.random.default_rng(3)
    for s in range(2):
        conf['sources'].append(dict(name='s%d' % s, events_per_day=40., data=model_zoo.sample(rng, 500, space), strength=1.0))
    lf = ns.UnbinnedLogLikelihood(conf, likelihood_config=dict(device_histograms=False))
    lf.add_rate_parameter('s0')
    lf.add_shape_parameter('shift', (-1., 0., 1.))
    lf.prepare()
    return lf, space


def test_set_datasets_and_simulate_toys_check_their_arguments():
    lf, space = histogram_lf()
    with pytest.raises(ValueError, match='at least one dataset'):
        lf.set_datasets([])
    good = np.zeros(3, dtype=[('x', float), ('y', float), ('source', int)])
    bad = np.zeros(3, dtype=[('x', float), ('source', int)])
    with pytest.raises(ValueError, match='dataset 1 lacks the analysis dimensions y'):
        lf.set_datasets([good, bad])
    with pytest.raises(ValueError, match='dataset 0 lacks'):
        lf.set_datasets([np.zeros(3)])
    for n in (0, -2):
        with pytest.raises(ValueError, match='n_toys must be at least 1'):
            lf.simulate_toys(n)


def test_simulate_toys_needs_histogram_sources():
    from blueice_amd import UnbinnedLogLikelihood
    from blueice_amd.test_helpers import conf_for_test
    lf = UnbinnedLogLikelihood(conf_for_test(events_per_day=3.), likelihood_config=dict(device_histograms=False))     # analytic pdf
    lf.add_rate_parameter('s0')
    lf.prepare()
    with pytest.raises(NotImplementedError, match='histogram'):
        lf.simulate_toys(4)
    with pytest.raises(NotImplementedError, match='histogram'):
        lf.simulate_toy()


def test_toy_mc_fits_names_both_likelihoods():
    from blueice_amd.inference import toy_mc_fits

    class NoToys:
        ctx = None
    with pytest.raises(NotImplementedError, match='binned or an unbinned likelihood'):
        toy_mc_fits(NoToys(), 3)
