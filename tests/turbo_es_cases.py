"""Seeded inputs of the early-termination tests, shared by tests/test_turbo_es_ref_host.py (which pins tests/turbo_es_ref.py and
asserts the operating points on the reference alone) and tests/test_gpu_turbo_es.py (which holds the kernel to the reference on
the same arrays).  Plain NumPy, no GPU.  Every function is deterministic; cached results are read-only."""
import functools

import numpy as np

import lte_bits_ref as lb
import turbo_cases as tc
import turbo_es_ref as er
import turbo_ref as tr

MAX_ITER = 6
ITER_PAIRS = ((1, 6), (2, 6), (1, 1), (6, 6), (3, 4))        # (min_iter, max_iter)
# The tile-remainder classes of turbo_cases.DEC_KS; 72 has a linear interleaver.
SPREAD_KS = (40, 48, 56, 64, 72, 104, 120, 512)
SPREAD_BLOCKS = 17
# (Es/N0 in dB, seed) per K, searched on the CPU (lowest seed from 0 at the stated Es/N0) so that at (1, 6) one 8-block group
# of the 17 CRC24B-terminated blocks holds a block that stops at 1, one that stops strictly between 1 and 6 and one that never
# passes: test_turbo_es_ref_host.py asserts it.
SPREAD = {40: (-4.0, 0), 48: (-4.0, 0), 56: (-4.0, 0), 64: (-4.5, 0), 72: (-4.0, 1), 104: (-4.0, 0), 120: (-4.0, 0), 512: (-3.75, 174)}
KIND_KS = {lb.CRC24A: 64, lb.CRC24B: 64, lb.CRC16: 56, lb.CRC8: 48}      # blocks terminated with each kind, at -3.5 dB
KIND_DB = -3.5
FALSE_PASS_K, FALSE_PASS_BLOCKS, FALSE_PASS_SEED = 40, 64, 0            # CRC8 on noise-only LLRs (seed searched on the CPU)
BIG_K, BIG_BLOCKS, BIG_MAX_ITER = 6144, 9, 2


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def crc_blocks(K, n, kind, rng):
    """-> info [n][K]: K - L random payload bits and their CRC of `kind` (zero mask)"""
    return lb.crc_attach(rng.integers(0, 2, (n, K - lb.CRC_BITS[kind])).astype(np.uint8), kind, 0)


def noisy(K, n, esn0_db, kind=lb.CRC24B, seed=0):
    """-> (llr [n][3K + 12] float32 at esn0_db, info [n][K] CRC-terminated)"""
    rng = np.random.default_rng(9000 + 131 * K + seed)
    info = crc_blocks(K, n, kind, rng)
    return tr.awgn_llrs(tr.encode(info, *tc.QPP[K]), esn0_db, rng), info


def noiseless(info, K):
    """-> llr [n][3K + 12]: +1 for a coded 0, -1 for a coded 1"""
    return (1.0 - 2.0 * tr.encode(info, *tc.QPP[K])).astype(np.float32)


def noise_only(K, n, seed=0):
    """-> llr [n][3K + 12]: Gaussian LLRs that carry no codeword"""
    return (4.0 * np.random.default_rng(9500 + K + seed).standard_normal((n, 3 * K + 12))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def spread(K):
    """-> (llr, info) of the K's spread case"""
    db, seed = SPREAD[K]
    return _ro(*noisy(K, SPREAD_BLOCKS, db, lb.CRC24B, seed))


@functools.lru_cache(maxsize=None)
def spread_ref(K, min_iter, max_iter):
    """-> (bits, llr, iters, crc_ok) of the reference on spread(K), checked as CRC24B"""
    return _ro(*er.decode_es(spread(K)[0], *tc.QPP[K], lb.CRC24B, min_iter, max_iter))


@functools.lru_cache(maxsize=None)
def kind_case(kind):
    """-> (K, llr, info, (bits, llr, iters, crc_ok) at (1, MAX_ITER)): 9 blocks terminated with and checked as `kind`"""
    K = KIND_KS[kind]
    llr, info = noisy(K, 9, KIND_DB, kind, seed=1)
    return (K,) + _ro(llr, info) + (_ro(*er.decode_es(llr, *tc.QPP[K], kind, 1, MAX_ITER)),)


@functools.lru_cache(maxsize=None)
def false_pass():
    """-> (llr, sent, (bits, llr, iters, crc_ok) at (1, MAX_ITER) checked as CRC8): noise-only LLRs at K = 40"""
    K = FALSE_PASS_K
    sent = crc_blocks(K, FALSE_PASS_BLOCKS, lb.CRC8, np.random.default_rng(9700 + FALSE_PASS_SEED))
    llr = noise_only(K, FALSE_PASS_BLOCKS, FALSE_PASS_SEED)
    return _ro(llr, sent) + (_ro(*er.decode_es(llr, *tc.QPP[K], lb.CRC8, 1, MAX_ITER)),)


def neighbour_wave(K, pos):
    """-> llr [8][3K + 12]: 7 noiseless CRC24B blocks and one noise-only block at position pos"""
    llr = noiseless(crc_blocks(K, 8, lb.CRC24B, np.random.default_rng(9800 + K)), K)
    llr[pos] = noise_only(K, 1, seed=7)[0]
    return llr


def flipped_bit(K, at):
    """-> llr [1][3K + 12]: a noiseless CRC24B block whose systematic LLR `at` has the wrong sign and dominates (1000 against
    the 1 of every other LLR: more than all the others of the block together can outvote at K <= 120, and at K = 512 more than
    any error event the decoder would have to accept instead)"""
    llr = noiseless(crc_blocks(K, 1, lb.CRC24B, np.random.default_rng(9900 + K)), K)
    llr[0, 3 * at] *= -1000.0
    return llr


@functools.lru_cache(maxsize=None)
def big():
    """-> (llr, (bits, llr, iters, crc_ok) at (1, BIG_MAX_ITER)): K = 6144, 8 noiseless CRC24B blocks and a noisy one (index 4)"""
    K = BIG_K
    rng = np.random.default_rng(9999)
    info = crc_blocks(K, BIG_BLOCKS, lb.CRC24B, rng)
    e = tr.encode(info, *tc.QPP[K])
    llr = (1.0 - 2.0 * e).astype(np.float32)
    llr[4] = tr.awgn_llrs(e[4], -4.5, rng)
    return _ro(llr) + (_ro(*er.decode_es(llr, *tc.QPP[K], lb.CRC24B, 1, BIG_MAX_ITER)),)
