"""The link case of the tests of receive diversity for multi-user allocations of DFT-spread OFDM: the two branches of mrc_cases.py
(taps, seeds, 64 frames of one turbo code block each, 64-pt, 16-QAM, K = 512), transmitted through the allocation precoder
(ofdm_tx_modulate_frames_alloc / dft_alloc_ref.spread_alloc) with two users that tile Kd = 60.  A frame's code block is spread
over both users; the receiver's LLRs come back allocation-major and are put back into row order before the decoder.
test_mrc_despread_alloc_ref_host.py asserts what the case has to satisfy on the oracle's receiver (estimated H) with the
restated stages; test_gpu_mrc_despread_alloc.py runs the same case end to end on the device."""
import numpy as np

import mrc_despread_cases as dc

N, CP, KS, KD = dc.N, dc.CP, dc.KS, dc.KD      # 64-pt, Kd = 60
MOD, BPS = dc.MOD, dc.BPS                      # 16-QAM
N_SYM, N_DSYM, SEG_BITS = dc.N_SYM, dc.N_DSYM, dc.SEG_BITS
K, F1, F2, N_ITER = dc.K, dc.F1, dc.F2, dc.N_ITER
N_FRAMES = dc.N_FRAMES
SNR_ARG, GATE, LEAD, FRAME_LEN = dc.SNR_ARG, dc.GATE, dc.LEAD, dc.FRAME_LEN
N_BRANCH, TAPS = dc.N_BRANCH, dc.TAPS
SEED_BITS, SEED_NOISE = dc.SEED_BITS, dc.SEED_NOISE
ALLOCS = [(0, 36, 4), (36, 24, 4)]             # (start, M, bits per symbol): two users, no gap
# Noise: as mrc_despread_cases.py (complex AWGN of this variance per time sample, one call of N_FRAMES frames per branch with seed
# SEED_NOISE + b; the stages are given the same number as every branch's variance).  The level was found by search on the
# oracle's receiver with the restated stages, starting from mrc_despread_cases.NOISE_VAR, not assumed.  Blocks lost of 64 at
# 0.06 / 0.08 / 0.1 / 0.126 / 0.159 / 0.2 / 0.25:
#   branch 0 alone (dft_alloc_ref, noise given)    0 /  8 / 22 / 59 / 64 / 64 / 64
#   branch 1 alone                                 6 / 32 / 55 / 63 / 64 / 64 / 64
#   combined (mrc_despread_alloc_ref)              0 /  0 /  0 /  0 /  0 /  0 /  2
# All conditions of the case hold from 0.1 to 0.159: each branch alone loses at least a quarter of the blocks (16), the combined
# stage loses none at the level and 1 dB further up.  The search stopped at its starting point; the first combined loss is 4 dB
# above it.
NOISE_VAR = 0.1
NOISE_VAR_1DB = NOISE_VAR * 10.0 ** 0.1
MIN_LOST_ALONE = N_FRAMES // 4                 # each branch alone loses at least a quarter of the blocks
LOST_AT_LEVEL = {"combined": 0, "branch 0 alone": 22, "branch 1 alone": 55}     # the oracle's own counts at NOISE_VAR

info_bits = dc.info_bits


def rows_from_blocks(blocks, n_frames=N_FRAMES, rows=N_DSYM, allocs=ALLOCS, row_len=KD):
    """allocation-major LLRs (block u: [n_frames][rows][M_u][bps], one after the other) -> [n_frames][rows*row_len*bps] in row
    order, the order of the transmitter's coded bits"""
    blocks = np.asarray(blocks)
    bps = allocs[0][2]
    out = np.zeros((n_frames, rows, row_len, bps), blocks.dtype)
    at = 0
    for start, M, b in allocs:
        assert b == bps
        n = n_frames * rows * M * bps
        out[:, :, start:start + M, :] = blocks[at:at + n].reshape(n_frames, rows, M, bps)
        at += n
    assert at == blocks.size
    return out.reshape(n_frames, rows * row_len * bps)
