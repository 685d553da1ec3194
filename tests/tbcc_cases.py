"""Seeded inputs of the TBCC edge tests, shared by tests/test_tbcc_ref_host.py (which asserts on the reference alone that the
inputs reach the paths they are meant to reach) and tests/test_gpu_tbcc_edges.py (which holds the kernels against the reference
on the same arrays).  Plain NumPy, no GPU.  Every function is deterministic: the same call returns the same arrays."""
import functools

import numpy as np

import tbcc_ref

# Every shape of the forward loop's last tile (64-step tiles of two 32-step halves in groups of 8: T mod 64 = (K + 192) mod 64
# runs through 0, 8, .. 56 four times below 256), every K < 96 (the warm-up of 96 steps wraps the block more than once), and the
# same eight remainders at the long end, where the survivors fill the most LDS.
K_SWEEP = tuple(range(24, 257, 8)) + tuple(range(1992, 2049, 8))
SWEEP_BLOCKS = 8
SWEEP_AWGN = slice(0, 4)                                    # the rows of sweep_blocks that carry noisy code words
SWEEP_ESN0_DB = -4.0

TIE_KS = (24, 48, 120, 256)
TIE_RANGES = ((-1, 2), (-2, 3))                             # integers(lo, hi): {-1, 0, 1} and {-2 .. 2}
TIE_BLOCKS = 64

SCALE_K, SCALE_BLOCKS, SCALE_SEED, SCALE_ESN0_DB = 120, 16, 7, 0.0
SCALE_EXPONENTS = (-140, -126, -60, 60, 100)

OUTPUT_KS = (24, 40, 2048)
OUTPUT_SEGS, OUTPUT_BPS, OUTPUT_PAD = 2, 5, 7               # 5 blocks per segment, stride = 5 * 3K + 7 floats

GRID_K, GRID_SRC, GRID_SEGS, GRID_BPS = 24, 16, 7000, 10    # 70 000 blocks: beyond 65 535
GRID_STRIDE = GRID_BPS * 3 * GRID_K + 5

ENC_SEGS, ENC_BPS = 2, 3
ENC_FILLER = {False: 45, True: 40}                          # by coded_packed: segment byte counts that are no multiple of 4


def noiseless(c):
    return (1.0 - 2.0 * tbcc_ref.encode(c)).astype(np.float32)


def sweep_blocks(K):
    """-> (llr [8][3K] float32, info [8][K] uint8): rows 0-3 AWGN at -4 dB, 4-5 integers in {-1, 0, 1}, 6 integers in {-2 .. 2},
    7 noiseless.  info is the transmitted word of rows 0-3 and 7 (rows 4-6 carry no code word: their info rows are unused)."""
    rng = np.random.default_rng(1000 + K)
    c = rng.integers(0, 2, (SWEEP_BLOCKS, K)).astype(np.uint8)
    llr = np.empty((SWEEP_BLOCKS, 3 * K), np.float32)
    llr[SWEEP_AWGN] = tbcc_ref.awgn_llrs(tbcc_ref.encode(c[SWEEP_AWGN]), SWEEP_ESN0_DB, rng)
    llr[4:6] = rng.integers(-1, 2, (2, 3 * K))
    llr[6] = rng.integers(-2, 3, 3 * K)
    llr[7] = noiseless(c[7])
    return llr, c


@functools.lru_cache(maxsize=None)
def sweep_reference(K):
    """-> (llr, info, (bits, metric, tb_ok) of tbcc_ref.decode), computed once per K and shared; treat as read-only"""
    llr, c = sweep_blocks(K)
    out = tbcc_ref.decode(llr)
    for a in (llr, c) + out:
        a.setflags(write=False)
    return llr, c, out


def tie_blocks(K, lo, hi):
    return np.random.default_rng(K).integers(lo, hi, (TIE_BLOCKS, 3 * K)).astype(np.float32)


def scale_blocks():
    """-> (llr [16][360] float32 at 0 dB, info [16][120])"""
    rng = np.random.default_rng(SCALE_SEED)
    c = rng.integers(0, 2, (SCALE_BLOCKS, SCALE_K)).astype(np.uint8)
    return tbcc_ref.awgn_llrs(tbcc_ref.encode(c), SCALE_ESN0_DB, rng), c


def scaled(llr, e):
    """llr * 2^e in float32 (one rounding per element, and only where the product is subnormal)"""
    return np.ldexp(np.asarray(llr, np.float32), e).astype(np.float32)


def output_segments(K):
    """-> llr_seg [2][5 * 3K + 7] float32 (NaN in the padding), the 10 blocks: 6 AWGN at -4 dB, 3 integer rows, 1 noiseless"""
    rng = np.random.default_rng(2000 + K)
    n = OUTPUT_SEGS * OUTPUT_BPS
    c = rng.integers(0, 2, (n, K)).astype(np.uint8)
    blocks = tbcc_ref.awgn_llrs(tbcc_ref.encode(c), SWEEP_ESN0_DB, rng)
    blocks[6:9] = rng.integers(-1, 2, (3, 3 * K))
    blocks[9] = noiseless(c[9])
    seg = np.full((OUTPUT_SEGS, OUTPUT_BPS * 3 * K + OUTPUT_PAD), np.nan, np.float32)
    seg[:, :OUTPUT_BPS * 3 * K] = blocks.reshape(OUTPUT_SEGS, OUTPUT_BPS * 3 * K)
    return seg


def grid_source():
    """-> llr [16][72]: 8 AWGN blocks at -4 dB and 8 integer blocks in {-1, 0, 1} (ties, tb_ok = 0 among them)"""
    rng = np.random.default_rng(3000)
    c = rng.integers(0, 2, (GRID_SRC, GRID_K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(tbcc_ref.encode(c), SWEEP_ESN0_DB, rng)
    llr[8:] = rng.integers(-1, 2, (8, 3 * GRID_K))
    return llr


def grid_segments(src):
    """block n of the batch = source block n mod 16 -> llr_seg [7000][10 * 72 + 5] (NaN in the padding)"""
    n = GRID_SEGS * GRID_BPS
    seg = np.full((GRID_SEGS, GRID_STRIDE), np.nan, np.float32)
    seg[:, :GRID_BPS * 3 * GRID_K] = src[np.arange(n) % GRID_SRC].reshape(GRID_SEGS, GRID_BPS * 3 * GRID_K)
    return seg


def encoder_info(K):
    return np.random.default_rng(4000 + K).integers(0, 2, (ENC_SEGS, ENC_BPS, K)).astype(np.uint8)


def impulse_positions(K):
    return (0, 1, 5, 6, K - 6, K - 1)


def impulse_info(K):
    """-> [2][3][K]: one block per impulse position.  k <= 5 makes the window positions i > k wrap below 0; K-6 .. K-1 are read
    THROUGH that wrap by the first steps' windows."""
    info = np.zeros((ENC_SEGS * ENC_BPS, K), np.uint8)
    for row, k in enumerate(impulse_positions(K)):
        info[row, k] = 1
    return info.reshape(ENC_SEGS, ENC_BPS, K)


def forward_stats(llr):
    """The contract's forward recursion once more (as in tbcc_ref.decode), counting what decode() does not report:
    -> dict(metric [n] float32 of the lowest-index best end state, ties [n] = steps x states with cand0 == cand1,
            end_tied [n] bool = several states share the largest metric, end_state [n] = the lowest such index)"""
    llr = np.ascontiguousarray(llr, np.float32)
    nb, K = llr.shape[0], llr.shape[1] // 3
    l = np.where(np.isfinite(llr), llr, np.float32(0)).astype(np.float32).reshape(nb, K, 3)
    p0, (sg0, sg1, sg2) = tbcc_ref._signs()
    pm = np.zeros((nb, 64), np.float32)
    ties = np.zeros(nb, np.int64)
    for t in range(K + 2 * tbcc_ref.W):
        i = (t - tbcc_ref.W) % K
        bm = (sg0 * l[:, i, 0:1] + sg1 * l[:, i, 1:2]) + sg2 * l[:, i, 2:3]
        c0, c1 = pm[:, p0] + bm, pm[:, p0 | 1] - bm
        ties += (c0 == c1).sum(axis=1)
        pm = np.where(c1 > c0, c1, c0)
    best = pm.max(axis=1)
    return dict(metric=best, ties=ties, end_tied=(pm == best[:, None]).sum(axis=1) > 1, end_state=np.argmax(pm, axis=1))
