"""The inputs of tests/test_toy_truths_gpu.py: toys at several truth points in one generator call.  The model is the d = 0
one-source context of the toy replay and the truths differ by a power-of-two rate_scale, so every mu_h = scale_h mu -- and
every partial sum of its prefix sum -- is exact.  Each case: the mu row of scale 1, the context's rate, the scales and numbers
of toys per truth, the methods the truths must take."""
import toy_replay_cases as cases

SEED = cases.SEED

# stream A, mixed truths (toy_events = 0): a truth without toys between the others
A_BINS = (3, cases.NZ_CHUNK - 1, cases.NZ_CHUNK + 1)
A_SCALES = (1.0, 2.0, 0.5, 1.0)
A_N_TOYS = (3, 0, 1, 4)
A_OFFSETS = (0, 2 ** 32 - 2)

# stream B, mixed truths
B_BINS = (4096, 4097)
B_M = 2.5
B_SCALES = (1.0, 4.0, 1.0)
B_N_TOYS = (2, 3, 1)

# both methods in one call: M = 100 is below B / 8 = 512 and 800 is not, so the per-bin truth sits between two event truths
MIX_B, MIX_M = 4096, 100.0
MIX_SCALES = (1.0, 8.0, 1.0)
MIX_N_TOYS = (3, 3, 2)
MIX_METHODS = (1, 0, 1)

# a truth boundary two toys below the launch-chunk seam of 32 768 toys (the shape of the replay's SEAM_A)
SEAM_B_BINS = cases.SEAM_A['B']
SEAM_N_TOYS = (32766, 5)
SEAM_SCALES = (1.0, 2.0)


def first_toys(n_toys):
    """first toy (number within the call) of every truth"""
    out, run = [], 0
    for n in n_toys:
        out.append(run)
        run += n
    return out
