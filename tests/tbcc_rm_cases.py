"""Seeded inputs of the rate-matching tests, shared by tests/test_tbcc_rm_ref_host.py (which asserts on the reference alone that
they hold what they are here for) and tests/test_gpu_tbcc_rm.py (which holds the kernels against the reference on the same
arrays).  Plain NumPy, no GPU.  Every function is deterministic; cached results are read-only."""
import functools

import numpy as np

import tbcc_ref
import tbcc_rm_ref as rm

# Every shape of the interleaver: R = 1 .. 8 with each ND in {0, 8, 16, 24} (K >= 24) at the short end, R = 63, 64 at the long end -- and
# with them every remainder of the decoder's last tile, as in tests/tbcc_cases.py.
K_SWEEP = tuple(range(24, 257, 8)) + tuple(range(1992, 2049, 8))
ALL_K = tuple(range(tbcc_ref.K_MIN, tbcc_ref.K_MAX + 1, 8))

# noiseless decoding (test_tbcc_rm_ref_host.py): (K, E) and blocks
NOISELESS = tuple((K, E, 64) for K, E in ((24, 72), (40, 72), (40, 144), (40, 288), (40, 576), (40, 1920), (48, 72), (56, 72), (64, 72),
                                          (64, 144), (72, 144), (24, 40), (120, 200), (256, 400))) + \
    ((1992, 3000, 8), (2048, 3100, 8), (2048, 6221, 8))

ENC_SEGS, ENC_BPS = 2, 3
ENC_FILLER = {False: 45, True: 40}      # by coded_packed, on top of blocks_per_seg * E rounded up to a byte for packed output


def enc_es(K):
    """puncturing, the permutation, repetition; 2K + 3 and 4K + 1 are odd: packed blocks start inside a byte"""
    return (2 * K + 3, 3 * K, 4 * K + 1)


def enc_info(K):
    return np.random.default_rng(5000 + K).integers(0, 2, (ENC_SEGS, ENC_BPS, K)).astype(np.uint8)


def enc_seg_bits(K, E, coded_packed):
    used = ENC_BPS * E
    return (used + 7) // 8 * 8 + ENC_FILLER[True] if coded_packed else used + ENC_FILLER[False]


# ---------------------------------------------------------------------------------------------- de-matching and decoding
DM_SEGS, DM_BPS, DM_PAD = 2, 4, 5       # 8 blocks per (K, E): 2 segments of 4 at a stride of 4E + 5 floats (NaN in the padding)
DM_DECODED = 6                          # blocks 0 .. 5 are inside the decoder's contract, 6 and 7 only de-matched
DM_ESN0_DB = 3.0
BIG = np.float32(3e38)
FULL_KS = (24, 40, 2048)                # with E = 48K: sixteen copies of every coded bit


def dm_es(K):
    es = (K + 1, 3 * K - 1, 3 * K, 3 * K + 1, 6 * K + 5)
    return es + (48 * K,) if K in FULL_KS else es


def dm_blocks(K, E):
    """-> (llr [8][E] float32, info [8][K]).  Rows: 0-2 AWGN at 3 dB of the rate-matched code word; 3 the same with NaN, +inf and
    -inf sprinkled in; 4 the same with every copy of each 5th repeated coded bit at 3e38 with one sign (the sum overflows to
    +-inf: the decoder takes 0) ; 5 the same with -0.0 at every 7th position; 6 values of +-3e38 with random signs (sums that
    overflow or cancel, by the order of the additions); 7 a mix of NaN, +-inf, -0.0 and small integers.  Rows 6 and 7 are
    outside the decoder's contract (finite LLRs whose branch metrics overflow) and are only de-matched."""
    rng = np.random.default_rng(7000 + 13 * K + E)
    c = rng.integers(0, 2, (8, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(rm.rate_match(tbcc_ref.encode(c), E), DM_ESN0_DB, rng)
    n3 = 3 * K
    llr[3, rng.integers(0, E, max(E // 6, 1))] = np.nan
    llr[3, rng.integers(0, E, max(E // 8, 1))] = np.inf
    llr[3, rng.integers(0, E, max(E // 8, 1))] = -np.inf
    for q in range(0, max(E - n3, 0), 5):                    # ranks with at least two copies
        llr[4, q::n3] = BIG if rng.integers(0, 2) else -BIG
    llr[5, ::7] = -0.0
    llr[6] = np.where(rng.integers(0, 2, E) == 1, BIG, -BIG)
    llr[7] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 2.0], np.float32), E)
    return llr, c


def dm_segments(llr, n_seg, bps, pad):
    """blocks [n_seg * bps][E] -> [n_seg][bps * E + pad] float32, NaN in the padding"""
    E = llr.shape[1]
    seg = np.full((n_seg, bps * E + pad), np.nan, np.float32)
    seg[:, :bps * E] = llr.reshape(n_seg, bps * E)
    return seg


@functools.lru_cache(maxsize=None)
def dm_reference(K):
    """-> dict E -> (llr [8][E], info, dematched [8][3K], (bits, metric, tb_ok) of rows 0 .. 5); one tbcc_ref.decode per K"""
    es = dm_es(K)
    rows = [dm_blocks(K, E) for E in es]
    dem = [rm.dematch(llr, K) for llr, _ in rows]
    b, m, ok = tbcc_ref.decode(np.concatenate([d[:DM_DECODED] for d in dem]))
    out = {}
    for n, E in enumerate(es):
        sl = slice(n * DM_DECODED, (n + 1) * DM_DECODED)
        vals = (rows[n][0], rows[n][1], dem[n], (b[sl].copy(), m[sl].copy(), ok[sl].copy()))
        for a in vals[:3] + vals[3]:
            a.setflags(write=False)
        out[E] = vals
    return out


# ---------------------------------------------------------------------------------------------- puncturing that fails tail-biting
PUNCTURED = ((64, 72), (56, 72))
PUNCTURED_BLOCKS, PUNCTURED_ESN0_DB = 64, 3.0
PUNCTURED_SEED = {(64, 72): 1, (56, 72): 3}     # seeds 1 .. 11 tried on the reference: (56, 72) has a wrong block with 3 and 4 only


@functools.lru_cache(maxsize=None)
def punctured_blocks(K, E):
    """-> (llr [64][E], info [64][K]): rate 8/9 and 7/9 at 3 dB, where the decoder makes errors and tail-biting fails"""
    rng = np.random.default_rng(PUNCTURED_SEED[(K, E)])
    c = rng.integers(0, 2, (PUNCTURED_BLOCKS, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(rm.rate_match(tbcc_ref.encode(c), E), PUNCTURED_ESN0_DB, rng)
    llr.setflags(write=False)
    c.setflags(write=False)
    return llr, c


# ---------------------------------------------------------------------------------------------- grid
GRID_K, GRID_E, GRID_SRC, GRID_SEGS, GRID_BPS = 24, 40, 16, 7000, 10     # 70 000 blocks: beyond 65 535
GRID_STRIDE = GRID_BPS * GRID_E + 3


def grid_source():
    """-> llr [16][40]: 8 AWGN blocks at 3 dB and 8 integer blocks in {-1, 0, 1}"""
    rng = np.random.default_rng(3100)
    c = rng.integers(0, 2, (GRID_SRC, GRID_K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(rm.rate_match(tbcc_ref.encode(c), GRID_E), DM_ESN0_DB, rng)
    llr[8:] = rng.integers(-1, 2, (8, GRID_E))
    return llr


def grid_segments(src):
    n = GRID_SEGS * GRID_BPS
    seg = np.full((GRID_SEGS, GRID_STRIDE), np.nan, np.float32)
    seg[:, :GRID_BPS * GRID_E] = src[np.arange(n) % GRID_SRC].reshape(GRID_SEGS, GRID_BPS * GRID_E)
    return seg
