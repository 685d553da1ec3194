"""The one link case of the channel-state-weighted LLR tests: 64 frames of one turbo code block each over a two-path channel
whose |H|^2 runs from 0.01 to 1.99 across the band, at a noise level where the per-frame-sigma LLRs of ofdm_demap_frames lose
blocks and the channel-weighted ones lose none.  test_csi_ref_host.py asserts that on the oracle's receiver (estimated H),
test_gpu_csi.py runs the same case end to end on the device."""
import numpy as np

import turbo_cases as tc

N, CP, KS, KD = 64, 16, 62, 60
MOD, BPS = "16QAM", 4
N_SYM = 12                                   # (1, 3) patterns: 9 data symbols = 2160 coded bits per frame
N_DSYM = 9
SEG_BITS = N_DSYM * KD * BPS
K = 512                                      # one block of 3K + 12 = 1548 coded bits per frame, then filler zeros
F1, F2 = tc.QPP[K]
N_ITER = 6
N_FRAMES = 64
TAPS = np.array([1.0, 0.0, 0.0, 0.9]) / np.linalg.norm([1.0, 0.0, 0.0, 0.9])
SNR_ARG = 30.0                               # the receiver's snr argument (UTSA law: SNR_lin = 10^(snr/20))
GATE = 0.5                                   # sync gate: the two paths split the correlation peak (0.74 of MM), 0.7 sits on it
LEAD = 0                                     # the device channel writes a frame from its sample 0
FRAME_LEN = N_SYM * (N + CP) + len(TAPS) - 1   # the whole convolution: what ofdm_channel_apply can write
# Noise: complex AWGN of this variance per time sample on a signal of unit variance, the counter-based noise of
# ofdm_channel_apply with seed SEED_NOISE (tests/channel_ref.py restates it), so that the host test and the device see the same
# samples.  The level was found by search on the oracle's receiver (estimated H), not assumed: with this seed the per-frame-sigma
# LLRs lose 3 / 4 / 14 / 28 / 49 of 64 blocks at 0.09 / 0.10 / 0.11 / 0.126 / 0.139 and the channel-weighted ones none up to 0.15;
# test_csi_ref_host.test_benefit_on_the_reference asserts what the case has to satisfy.
NOISE_VAR = 0.11
NOISE_VAR_1DB = NOISE_VAR * 10.0 ** 0.1
SEED_BITS, SEED_NOISE = 20260, 20261


def info_bits():
    return np.random.default_rng(SEED_BITS).integers(0, 2, (N_FRAMES, 1, K)).astype(np.uint8)
