"""The link case of the receive-diversity combining tests: the case of csi_cases.py received over two branches.  Branch 0 is that
case's channel and noise stream; branch 1 has taps [1, 0, 0.9j, 0]/|.| (its fades lie in other bins) and the noise seed
SEED_NOISE + 1.  The noise level is one where either branch alone, through the channel-state-weighted LLRs, loses blocks (15 and
61 of 64 on the oracle's receiver) and the combined branches lose none, also 1 dB further up.  test_mrc_ref_host.py asserts that
on the reference alone, test_gpu_mrc.py runs the same case end to end on the device."""
import numpy as np

import csi_cases as cc

N, CP, KS, KD = cc.N, cc.CP, cc.KS, cc.KD
MOD, BPS = cc.MOD, cc.BPS
N_SYM, N_DSYM, SEG_BITS = cc.N_SYM, cc.N_DSYM, cc.SEG_BITS
K, F1, F2, N_ITER = cc.K, cc.F1, cc.F2, cc.N_ITER
N_FRAMES = cc.N_FRAMES
SNR_ARG, GATE, LEAD, FRAME_LEN = cc.SNR_ARG, cc.GATE, cc.LEAD, cc.FRAME_LEN
N_BRANCH = 2
_T1 = np.array([1.0, 0.0, 0.9j, 0.0])
TAPS = [cc.TAPS, _T1 / np.linalg.norm(_T1)]
# one ofdm_channel_apply / channel_ref.noise call of N_FRAMES frames per branch, with seed SEED_NOISE + b
SEED_BITS, SEED_NOISE = cc.SEED_BITS, cc.SEED_NOISE
NOISE_VAR = 0.175
NOISE_VAR_1DB = NOISE_VAR * 10.0 ** 0.1

info_bits = cc.info_bits
