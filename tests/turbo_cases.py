"""Seeded inputs of the turbo codec tests, shared by tests/test_turbo_ref_host.py (which asserts on the reference alone that the
decoder inputs sit at an operating point with wrong AND right decisions) and tests/test_gpu_turbo.py (which holds the kernels
against the reference on the same arrays).  Plain NumPy, no GPU.  Every function is deterministic."""
import functools

import numpy as np

import turbo_ref

# (f1, f2) per K, each checked to be a permutation (test_turbo_ref_host.py asserts it).  72 and 520 are linear interleavers
# (f2 = 0, f1 coprime to K); IDENTITY is pi(i) = i at K = 40.
QPP = {40: (3, 10), 48: (7, 12), 56: (19, 42), 64: (7, 16), 72: (5, 0), 104: (7, 26), 120: (103, 90), 512: (31, 64), 520: (3, 0),
       1024: (31, 64), 6144: (263, 480)}
IDENTITY = (40, 1, 0)
ENC_KS = (40, 48, 56, 64, 72, 104, 120, 512, 520, 1024, 6144)

# Decoder: every K mod 32 class of the checkpointed tiles (K = 8 .. 32 mod 32 and K = 40, 48, 56 mod 64) and K < 64.
DEC_KS = (40, 48, 56, 64, 72, 104, 120, 512, 520)
DEC_ITERS = (1, 2, 6)
DEC_COUNTS = (1, 7, 8, 9, 17)                                # partial 8-block groups of the decoder's waves
DEC_BLOCKS = 17
# Es/N0 of the BPSK-over-AWGN LLRs per K, chosen on the CPU so that the reference decodes 10 % .. 60 % of the DEC_BLOCKS blocks
# wrongly at n_iter = 1 and strictly fewer at n_iter = 6 (asserted in test_turbo_ref_host.py).
ESN0_DB = {40: -4.0, 48: -3.5, 56: -3.5, 64: -3.5, 72: -3.5, 104: -3.0, 120: -3.0, 512: -2.0, 520: -2.0, 1024: -3.0, 6144: -3.5}
BIG_K, BIG_BLOCKS, BIG_ITERS = 6144, 9, 2

GRID_K, GRID_SRC, GRID_BLOCKS = 40, 16, 20000


def noisy_blocks(K, n=DEC_BLOCKS, seed=0):
    """-> (llr [n][3K + 12] float32 at ESN0_DB[K], info [n][K])"""
    f1, f2 = QPP[K]
    rng = np.random.default_rng(5000 + K + seed)
    c = rng.integers(0, 2, (n, K)).astype(np.uint8)
    return turbo_ref.awgn_llrs(turbo_ref.encode(c, f1, f2), ESN0_DB[K], rng), c


@functools.lru_cache(maxsize=None)
def decoded(K, n_iter, n=DEC_BLOCKS):
    """-> (llr, info, bits, llr_out) of turbo_ref.decode on noisy_blocks(K, n): computed once and shared; treat as read-only"""
    llr, c = noisy_blocks(K, n)
    bits, out = turbo_ref.decode(llr, *QPP[K], n_iter)
    for a in (llr, c, bits, out):
        a.setflags(write=False)
    return llr, c, bits, out


def edge_blocks(K):
    """-> llr [8][3K + 12] float32: 0 noisy, 1 NaN / +-inf sprinkled in, 2 all zero (every max ties), 3 integers in {-1, 0, 1},
    4 integers in {-2 .. 2}, 5 signed zeros and subnormals by bit pattern, 6 all NaN, 7 noiseless"""
    rng = np.random.default_rng(6000 + K)
    llr, c = noisy_blocks(K, 8, seed=1)
    llr = llr.copy()
    n = 3 * K + 12
    llr[1, rng.integers(0, n, K // 4)] = np.nan
    llr[1, rng.integers(0, n, K // 4)] = np.inf
    llr[1, rng.integers(0, n, K // 4)] = -np.inf
    llr[2] = 0.0
    llr[3] = rng.integers(-1, 2, n)
    llr[4] = rng.integers(-2, 3, n)
    pat = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000], np.uint32)
    llr[5] = pat[rng.integers(0, len(pat), n)].view(np.float32)
    llr[6] = np.nan
    llr[7] = (1.0 - 2.0 * turbo_ref.encode(c[7:8], *QPP[K])[0]).astype(np.float32)
    return llr


def grid_source():
    """-> llr [16][132]: 12 noisy K = 40 blocks and 4 integer blocks in {-1, 0, 1}"""
    llr, _ = noisy_blocks(GRID_K, GRID_SRC, seed=2)
    llr = llr.copy()
    llr[12:] = np.random.default_rng(7000).integers(-1, 2, (4, 3 * GRID_K + 12))
    return llr
