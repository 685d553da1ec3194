"""Seeded inputs and small helpers of the transport-block tests, shared by tests/test_tb_ref_host.py, tests/test_tb_host.py
(no GPU) and tests/test_gpu_tb.py.  Plain NumPy, no GPU.  Every function is deterministic."""
import functools
import math

import numpy as np

import tb_ref
import turbo_ref
from turbo_cases import QPP

# the hand-derived segmentations of the issue: (A, Z) -> (C, K-, C-, K+, C+, F, L)
HAND = {(80, 64): (3, 56, 2, 64, 1, 0, 24), (72, 64): (3, 48, 0, 56, 3, 0, 24), (88, 64): (3, 56, 1, 64, 2, 0, 24),
        (48, 64): (2, 56, 1, 64, 1, 0, 24), (976, 528): (2, 512, 0, 528, 2, 8, 24), (496, 528): (1, 0, 0, 528, 1, 8, 0),
        (496, 6144): (1, 0, 0, 528, 1, 8, 0), (6120, 6144): (1, 0, 0, 6144, 1, 0, 0), (6128, 6144): (2, 3072, 1, 3136, 1, 8, 24),
        (75376, 6144): (13, 5760, 0, 5824, 13, 0, 24)}
SWEEP_ZS = (64, 512, 528, 6144)
SWEEP_AS = tuple(range(8, 4097, 8))
QS = (1, 2, 4, 6, 12)


def qpp_for(K):
    """a pair ofdm_turbo_qpp_check accepts: tests/turbo_cases.py's where it has one, else f1 = the smallest odd number >= 3
    coprime to K and f2 = the product of K's distinct prime factors (K is a multiple of 8, so this is sufficient)"""
    if K in QPP:
        return QPP[K]
    rad, n, p = 1, K, 2
    while n > 1:
        if n % p == 0:
            rad *= p
            while n % p == 0:
                n //= p
        p += 1
    f1 = next(f for f in range(3, K, 2) if math.gcd(f, K) == 1)
    assert rad < K
    return f1, rad


def pairs(A, Z):
    """-> (qpp_minus, qpp_plus) for the geometry of (A, Z); (0, 0) for a K- without blocks"""
    g = tb_ref.segmentation(A, Z)
    return (qpp_for(g["K_minus"]) if g["C_minus"] else (0, 0)), qpp_for(g["K_plus"])


def full_g(A, Z):
    """G at which every block sends each coded bit once: sum (3 K_r + 12)"""
    return tb_ref.geometry(A, Z)["soft_floats"]


def payloads(A, n_tb, seed=0):
    return np.random.default_rng(31000 + A + 977 * seed).integers(0, 2, (n_tb, A)).astype(np.uint8)


def noise(shape, seed):
    return (4.0 * np.random.default_rng(32000 + seed).standard_normal(shape)).astype(np.float32)


def g_sweep(C):
    """G' = G / q values around the multiples of C: every gamma class that matters (0, 1, C - 1) and some between"""
    base = 40 * C
    return sorted({base, base + 1, base + C - 1, base + C // 2, 3 * base + 2, 107 * C + (C - 1)})


# The device HARQ chain and its host-side condition: A = 976 at Z = 528 is two blocks of K = 528 with 8 filler bits.  G = 1000 in
# units of q = 2 (QPSK) gives E = 500 per block, below K + 4 = 532: rv 0 starts in the systematic part, so the first round leaves
# information bits unsent and carries no parity -- it fails whatever the noise is -- and rv 2 brings each block to rate 0.53,
# which + 13 dB leaves 12 dB over (the reasoning of HARQ_POINTS in tests/turbo_rm_cases.py, whose noise point this is).
HARQ_A, HARQ_Z, HARQ_G, HARQ_Q, HARQ_ESN0_DB = 976, 528, 1000, 2, 13.0
HARQ_TBS, HARQ_ITERS, HARQ_SEED = 17, 6, 1


@functools.lru_cache(maxsize=None)
def harq_rounds(seed=HARQ_SEED):
    """-> (payload [n][A], l0 [n][G], l2 [n][G]): the rv 0 and rv 2 transmissions over independent BPSK / AWGN noise; read-only"""
    rng = np.random.default_rng(33000 + seed)
    p = rng.integers(0, 2, (HARQ_TBS, HARQ_A)).astype(np.uint8)
    qm, qp = pairs(HARQ_A, HARQ_Z)
    l0 = turbo_ref.awgn_llrs(tb_ref.encode(p, HARQ_G, qm, qp, Z=HARQ_Z, q=HARQ_Q, rv=0), HARQ_ESN0_DB, rng)
    l2 = turbo_ref.awgn_llrs(tb_ref.encode(p, HARQ_G, qm, qp, Z=HARQ_Z, q=HARQ_Q, rv=2), HARQ_ESN0_DB, rng)
    for a in (p, l0, l2):
        a.setflags(write=False)
    return p, l0, l2
