"""The link case of the tests of receive diversity for DFT-spread OFDM: the two branches of mrc_cases.py (taps, seeds, 64 frames
of one turbo code block each, 64-pt, 16-QAM, K = 512) with the transform precoding of dft_spread_cases.py (M = 60).
test_mrc_despread_ref_host.py asserts what the case has to satisfy on the oracle's receiver (estimated H) with the restated
stages; test_gpu_mrc_despread.py runs the same case end to end on the device."""
import mrc_cases as mc

N, CP, KS, KD = mc.N, mc.CP, mc.KS, mc.KD      # 64-pt, Kd = M = 60
MOD, BPS = mc.MOD, mc.BPS                      # 16-QAM
N_SYM, N_DSYM, SEG_BITS = mc.N_SYM, mc.N_DSYM, mc.SEG_BITS
K, F1, F2, N_ITER = mc.K, mc.F1, mc.F2, mc.N_ITER
N_FRAMES = mc.N_FRAMES
SNR_ARG, GATE, LEAD, FRAME_LEN = mc.SNR_ARG, mc.GATE, mc.LEAD, mc.FRAME_LEN
N_BRANCH, TAPS = mc.N_BRANCH, mc.TAPS
SEED_BITS, SEED_NOISE = mc.SEED_BITS, mc.SEED_NOISE
# Noise: complex AWGN of this variance per time sample on a signal of unit variance, one ofdm_channel_apply / channel_ref.noise
# call of N_FRAMES frames per branch with seed SEED_NOISE + b; the stages are given the same number as every branch's variance.
# The level was found by search on the oracle's receiver with the restated stages, not assumed.  Blocks lost of 64 at
# 0.045 / 0.06 / 0.08 / 0.1 / 0.126 / 0.159 / 0.2 / 0.25 / 0.32 / 0.4 / 0.5:
#   branch 0 alone (dft_spread_ref, noise given)   0 /  1 / 10 / 27 / 51 / 63 / 64 / 64 / 64 / 64 / 64
#   branch 1 alone                                 0 /  3 / 28 / 55 / 64 / 64 / 64 / 64 / 64 / 64 / 64
#   combined (mrc_despread_ref)                    0 /  0 /  0 /  0 /  0 /  0 /  0 /  2 / 32 / 62 / 64
# All three conditions of the case hold from 0.06 to 0.159: each branch alone loses blocks, the combined stage loses none at the
# level and 1 dB further up.  NOISE_VAR sits where both single branches lose many blocks; the first combined loss is 4 dB above it.
NOISE_VAR = 0.1
NOISE_VAR_1DB = NOISE_VAR * 10.0 ** 0.1

info_bits = mc.info_bits
