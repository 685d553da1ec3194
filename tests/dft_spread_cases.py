"""The one link case of the DFT-spread OFDM tests: 64 frames of one turbo code block each, transform-precoded (M = 60) and sent
over the two-path channel of csi_cases.py, whose |H|^2 runs from 0.01 to 1.99 across the band.  test_dft_spread_ref_host.py
asserts what the case has to satisfy on the oracle's receiver (estimated H) with the restated despreading stage,
test_gpu_dft_spread.py runs the same case end to end on the device."""
import numpy as np

import csi_cases as cc

N, CP, KS, KD = cc.N, cc.CP, cc.KS, cc.KD      # 64-pt, Kd = M = 60
MOD, BPS = cc.MOD, cc.BPS                      # 16-QAM
N_SYM, N_DSYM, SEG_BITS = cc.N_SYM, cc.N_DSYM, cc.SEG_BITS
K, F1, F2, N_ITER = cc.K, cc.F1, cc.F2, cc.N_ITER
N_FRAMES = cc.N_FRAMES
TAPS = cc.TAPS
SNR_ARG, GATE, LEAD, FRAME_LEN = cc.SNR_ARG, cc.GATE, cc.LEAD, cc.FRAME_LEN
# Noise: complex AWGN of this variance per time sample on a signal of unit variance, the counter-based noise of
# ofdm_channel_apply with seed SEED_NOISE (tests/channel_ref.py restates it).  The weights use OFDM_DESPREAD_NOISE_RHO: one code
# block per segment, and a max-log decoder does not see a common scale of its LLRs.
# The level was found by search on the oracle's receiver with the restated stage, not assumed.  With this seed the chain loses
# 0 / 0 / 0 / 0 / 0 / 1 / 3 / 11 of 64 blocks at 0.01 / 0.02 / 0.04 / 0.045 / 0.0567 / 0.06 / 0.07 / 0.08, while the undecoded
# hard bits of the code blocks have 4.6 / 7.8 / 12.4 / 13.3 / 15.1 / 15.6 / 16.9 / 18.2 % errors: behind the MMSE equaliser the
# despread symbol carries the residual interference and the noise of the faded bins in every symbol, so the case sits 4.4 dB
# below the plain-OFDM one of csi_cases.py.  test_dft_spread_ref_host.test_link_case_on_the_reference asserts what the case has
# to satisfy at NOISE_VAR and 1 dB further up (0.0504); the first loss is 1.8 dB above NOISE_VAR.
# The filler zeros behind a frame's 3K + 12 coded bits are one spectral line after the precoder; they belong to no block and are
# left out of the error rate.
NOISE_VAR = 0.04
NOISE_VAR_1DB = NOISE_VAR * 10.0 ** 0.1
SEED_BITS, SEED_NOISE = 36211, 36212


def info_bits():
    return np.random.default_rng(SEED_BITS).integers(0, 2, (N_FRAMES, 1, K)).astype(np.uint8)
