"""Seeded inputs of the turbo rate-matching tests, shared by tests/test_turbo_rm_ref_host.py (which asserts the HARQ operating
point on the reference alone) and tests/test_gpu_turbo_rm.py (which holds the kernels against the reference on the same
arrays).  Plain NumPy, no GPU.  Every function is deterministic."""
import functools

import numpy as np

import turbo_ref
import turbo_rm_ref as rm
from turbo_cases import QPP

# K = 40, 48, 56, 64 give ND = 20, 12, 4, 28 and R = 2, 2, 2, 3: every ND, and a buffer whose rows are not a power of two
SMALL_KS = (40, 48, 56, 64)
BIG_K = 6144
RVS = (0, 1, 2, 3)


def ncbs(K):
    """the three buffer limits of the tests: the smallest (v0 alone), an odd one that ends inside the interlaced part, all of w"""
    _, _, Kpi, _, Kw = rm.dims(K)
    return (Kpi, 2 * Kpi + 1, Kw)


def enc_es(K):
    """E below D (not even the systematic bits), odd and between, the whole block, and more than the buffer (wraps)"""
    return (K + 1, 2 * K + 3, 3 * K + 12, 4 * K + 1)


# HARQ operating points: (K, E, Es/N0 in dB) at which, with HARQ_BLOCKS blocks and HARQ_ITERS iterations, the reference decodes at
# least half the blocks wrongly from the rv 0 transmission alone and none after the rv 2 transmission is added
# (tests/test_turbo_rm_ref_host.py asserts every one of them on the reference).
#
# HARQ_NOISE_POINTS: soft combining near the code's threshold.  E is a little above K + 4, so rv 0 carries every systematic bit
# and some parity (rate 0.8 and 0.75) and fails BECAUSE OF THE NOISE; rv 2 starts inside the interlaced parity part and the two
# rounds together (rate 0.4 and 0.375) decode.  BPSK over AWGN, host only.
#
# HARQ_POINTS: the points the GPU chain test runs, behind a real receiver.  That receiver equalises with the unsmoothed LS
# estimate of ONE sync symbol whose Ks = 62 bins share the power a data symbol puts into Kd = 40, so an equalised data bin sees
# 1 / snr_eff = (1 + Ks / Kd) / snr plus the product term: the LLRs sit 4.1 dB and more below the channel's Es/N0, and by how
# much more depends on the receiver, not on the rate matcher.  A point at the code's threshold would therefore test the
# receiver's loss.  Instead E is below K + 4: rv 0 -- which starts in the systematic part -- leaves information bits unsent and
# carries no parity, so the first round fails whatever the noise is, and rv 2 brings the block to rate 1/2, which needs about
# 0 .. 1 dB.  + 13 dB leaves 12 dB over that: room for a receiver loss of twice the model's and more.  What this point tests
# on the device is that accumulate adds the rv 2 values into the rv 0 buffer at the right places; the soft buffer, the decoded
# bits and the CRC flags are held to the reference bit for bit at both rounds either way.
HARQ_NOISE_POINTS = ((512, 640, 1.0), (120, 160, 1.0))
HARQ_POINTS = ((512, 500, 13.0), (120, 116, 13.0))
HARQ_BLOCKS, HARQ_ITERS = 17, 6


def info_bits(K, n_seg, bps, seed=0):
    return np.random.default_rng(9000 + K + 131 * seed).integers(0, 2, (n_seg, bps, K)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def harq_rounds(K, E, esn0_db, n=HARQ_BLOCKS):
    """-> (info [n][K], l0 [n][E], l2 [n][E]): the rv 0 and the rv 2 transmission of the same blocks over independent noise;
    treat as read-only"""
    f1, f2 = QPP[K]
    rng = np.random.default_rng(9100 + K)
    c = rng.integers(0, 2, (n, K)).astype(np.uint8)
    e = turbo_ref.encode(c, f1, f2)
    l0 = turbo_ref.awgn_llrs(rm.rate_match(e, E, 0, 0), esn0_db, rng)
    l2 = turbo_ref.awgn_llrs(rm.rate_match(e, E, 0, 2), esn0_db, rng)
    for a in (c, l0, l2):
        a.setflags(write=False)
    return c, l0, l2


def awgn_rows(n, E, seed):
    """[n][E] float32 noise-like LLRs"""
    return (4.0 * np.random.default_rng(9200 + seed).standard_normal((n, E))).astype(np.float32)


def edge_rows(E, seed):
    """[6][E] float32: 0 noise, 1 NaN / +-inf sprinkled in, 2 rows of +-3e38 whose sums overflow or cancel depending on the order
    of the additions, 3 signed zeros and subnormals by bit pattern, 4 all -0.0, 5 all NaN"""
    rng = np.random.default_rng(9300 + seed)
    l = awgn_rows(6, E, seed + 1).copy()
    for val in (np.nan, np.inf, -np.inf):
        l[1, rng.integers(0, E, max(1, E // 5))] = val
    l[2] = np.array([3e38, 3e38, -3e38, 1.0, -3e38, 3e38], np.float32)[rng.integers(0, 6, E)]
    pat = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff], np.uint32)
    l[3] = pat[rng.integers(0, len(pat), E)].view(np.float32)
    l[4] = -0.0
    l[5] = np.nan
    return l
