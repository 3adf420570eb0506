"""The inputs of the toy replay: shared by tests/test_toy_replay_gpu.py (which runs them on the device) and
tests/test_toy_oracle.py (which holds the oracle's undecided share and the mutants to them on the CPU).  Expectations are
dyadic, so that the device's mu = rate x p -- and every partial sum of its prefix sum -- is the oracle's bit for bit."""
import numpy as np

NZ_CHUNK = 2048                  # kNzChunk: bins per block of k_toy_count / k_toy_scatter
SEED = 12345
SEEDS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)

# stream A.  p = mu 2^-21 and rate = 2^21 are exact for every entry (2^-1000 2^-21 is still a normal number)
RATE_A = 2.0 ** 21
MU_ROW = np.array([0.0, 2.0 ** -1000, 2.0 ** -20, 0.5, np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, np.inf), 37.25, 250.0, 2.0 ** 20,
                   # neighbours: one, both or neither of a pair take PTRS, whichever the parity of the first
                   3.0, 40.0, 60.0, 2.0, 1.5, 0.25, 12.0, 11.0, 0.75])


def per_bin_mu(B, shift=0):
    return MU_ROW[(np.arange(B) + shift) % len(MU_ROW)]


PER_BIN_CASES = [(B, shift) for B in (1, 2, 3) for shift in range(len(MU_ROW))] + \
                [(B, shift) for B in (NZ_CHUNK - 1, NZ_CHUNK, NZ_CHUNK + 1, 2 * NZ_CHUNK + 1) for shift in (0, 1)]
T_PER_BIN = 8
SEAM_A = dict(B=64, T=32771, first=32766)                          # launch chunks of 32 768 toys
OFFSETS = ((2 ** 32 - 2, 4), (2 ** 47, 2))                         # (toy_offset, T): the dataset-word seams


# stream B.  Multiples of 2^-16 throughout; M a multiple of 2^-13
RATE_B = 2.0 ** 11


def event_mu(B, M):
    """Zero plateaus (the first bins, the run before the busy bin, six of every seven bins of the bulk), one bin with M / 2,
    the last bin with M / 8, the rest spread evenly with the remainder in bin 11."""
    M = round(M * 8192) / 8192
    mu = np.zeros(B)
    busy = B // 3
    live = np.arange(10, B - 1)
    live = live[(live % 7 == 3) & ((live < busy - 50) | (live > busy))]
    rest = 3 * M / 8
    q = np.floor(rest / len(live) * 65536) / 65536
    mu[live] = q
    mu[11] = rest - q * len(live)
    mu[busy] = M / 2
    mu[B - 1] = M / 8
    assert mu.sum() == M and np.all(mu * 65536 == np.floor(mu * 65536)) and mu[11] >= 0
    return mu


# (B, M, T, path): path 1 = event by event, 0 = the call must fall back to one draw per bin
EVENT_CASES = [(B, M, 6, 1) for B in (4096, 4097, 65536, 65537) for M in (2.5, 9.999, 10.0)] + \
              [(B, 1900.0, 6, 1) for B in (65536, 65537)] + \
              [(16384, 1024.0, 6, 1), (131072, 15000.0, 3, 1), (262144, 31000.0, 2, 0)]
SEAM_B = dict(B=4096, M=2.5, T=65538, first=65533)                  # launch chunks of 65 535 toys

# bi_simulate_events: the edges of tests/test_unbinned_gpu.py, three sources, one morphing parameter
SIM_EDGES = [np.linspace(-4, 4, 17), np.array([0., 0.4, 1., 2.2, 3.5, 5.]), np.linspace(-1, 1, 6)]
SIM_ANCHORS = np.array([-1.0, 0.0, 1.0])
SIM_Z = 0.35
# (dims, method, mus of the three sources, score_sorted)
SIM_CASES = [(1, 'linear', (3.0, 400.0, 0.0), 1), (1, 'piecewise', (400.0, 0.0, 3.0), 1), (2, 'linear', (0.0, 3.0, 400.0), 1),
             (2, 'piecewise', (3.0, 400.0, 0.0), 0), (3, 'piecewise', (400.0, 3.0, 0.0), 1), (3, 'linear', (3.0, 5000.0, 0.0), 1)]


def sim_model(dims, mus):
    """-> (edges, ps [3 anchors, 3 sources, B] densities with zero plateaus, mus [3 anchors, 3])"""
    edges = SIM_EDGES[:dims]
    B = int(np.prod([len(e) - 1 for e in edges]))
    rng = np.random.default_rng(500 + dims)
    ps = rng.random((3, 3, B)) + 0.01
    ps[:, :, :2] = 0.0                                               # the first bins
    ps[:, :, B // 2:B // 2 + 3] = 0.0                                # a run in the middle, the same at every anchor
    ps[:, 1, B - 1] = 0.0                                            # source 1: the last bin as well
    return edges, ps, np.tile(np.asarray(mus, dtype=float), (3, 1))


def sim_point(ps, mus):
    """The densities [S, B] and rates [S] at SIM_Z: linear between the two anchors around it."""
    i = int(np.searchsorted(SIM_ANCHORS, SIM_Z, side='right')) - 1
    w = (SIM_Z - SIM_ANCHORS[i]) / (SIM_ANCHORS[i + 1] - SIM_ANCHORS[i])
    return ps[i] * (1.0 - w) + ps[i + 1] * w, mus[i] * (1.0 - w) + mus[i + 1] * w
