"""The TBCC contract of include/ofdm_mi355x.h (LTE tail-biting convolutional code, TS 36.212 5.1.3.1) restated in NumPy float32,
vectorised over code blocks.  This is the yardstick the GPU kernels are held against: every float operation below is one IEEE
float32 operation in the order the contract writes it.  tests/test_tbcc_ref_host.py pins this file by independent means."""
import numpy as np

W = 96
GENERATORS = (0o133, 0o171, 0o165)      # bit 6 = current input, bit 6-i = delay i
K_MIN, K_MAX = 24, 2048


def valid_k(K) -> bool:
    return K_MIN <= K <= K_MAX and K % 8 == 0


def blocks(seg_bits: int, K: int) -> int:
    if not valid_k(K) or seg_bits < 0:
        raise ValueError("bad K or seg_bits")
    return seg_bits // (3 * K)


def encode(c: np.ndarray) -> np.ndarray:
    """c [..., K] bits -> e [..., 3K] coded bits, e[3k+j] = dj[k]."""
    c = np.asarray(c, dtype=np.uint8) & 1
    K = c.shape[-1]
    assert valid_k(K)

    def dl(i):
        return np.roll(c, i, axis=-1)                        # dl(i)[k] = c[(k - i) mod K]
    d0 = dl(0) ^ dl(2) ^ dl(3) ^ dl(5) ^ dl(6)
    d1 = dl(0) ^ dl(1) ^ dl(2) ^ dl(3) ^ dl(6)
    d2 = dl(0) ^ dl(1) ^ dl(2) ^ dl(4) ^ dl(6)
    return np.stack([d0, d1, d2], axis=-1).reshape(c.shape[:-1] + (3 * K,))


def encode_segments(info: np.ndarray, seg_bits: int) -> np.ndarray:
    """info [n_seg][blocks_per_seg][K] -> [n_seg][seg_bits]: the blocks back to back from bit 0, then zeros."""
    n_seg, bps, K = info.shape
    assert bps * 3 * K <= seg_bits
    out = np.zeros((n_seg, seg_bits), np.uint8)
    out[:, :bps * 3 * K] = encode(info).reshape(n_seg, bps * 3 * K)
    return out


def _parity(x):
    x = np.asarray(x, dtype=np.int64)
    p = np.zeros_like(x)
    for i in range(7):
        p ^= (x >> i) & 1
    return p


def _signs():
    s1 = np.arange(64)
    p0 = (s1 << 1) & 63
    tr = ((s1 >> 5) << 6) | p0
    sg = [np.where(_parity(tr & g) == 1, -1.0, 1.0).astype(np.float32) for g in GENERATORS]
    return p0, sg


def decode(llr: np.ndarray):
    """llr [n_blocks][3K] float32 -> (bits [n_blocks][K] uint8, metric [n_blocks] float32, tb_ok [n_blocks] int32)."""
    llr = np.ascontiguousarray(llr, dtype=np.float32)
    nb, n3 = llr.shape
    K = n3 // 3
    assert n3 == 3 * K and valid_k(K)
    T = K + 2 * W
    l = np.where(np.isfinite(llr), llr, np.float32(0)).astype(np.float32).reshape(nb, K, 3)
    p0, (sg0, sg1, sg2) = _signs()
    p1 = p0 | 1
    pm = np.zeros((nb, 64), np.float32)
    dec = np.zeros((T, nb, 64), np.bool_)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T):
            i = (t - W) % K
            l0, l1, l2 = l[:, i, 0:1], l[:, i, 1:2], l[:, i, 2:3]
            bm = (sg0 * l0 + sg1 * l1) + sg2 * l2
            assert bm.dtype == np.float32
            c0 = pm[:, p0] + bm
            c1 = pm[:, p1] - bm
            d = c1 > c0
            pm = np.where(d, c1, c0)
            dec[t] = d
    assert pm.dtype == np.float32
    s = np.argmax(pm, axis=1)                                # the first (lowest) index of the maximum
    metric = pm[np.arange(nb), s].copy()
    bits_t = np.zeros((T, nb), np.uint8)
    s_end = s_begin = None
    rows = np.arange(nb)
    for t in range(T - 1, -1, -1):
        if t + 1 == W + K:
            s_end = s.copy()
        bits_t[t] = s >> 5
        s = ((s << 1) & 63) | dec[t, rows, s]
        if t == W:
            s_begin = s.copy()
    bits = np.ascontiguousarray(bits_t[W:W + K].T)
    return bits, metric, (s_begin == s_end).astype(np.int32)


def decode_segments(llr_seg: np.ndarray, blocks_per_seg: int, K: int):
    """llr_seg [n_seg][>= blocks_per_seg*3K]: the decoder over every block of every segment (the filler is ignored).
    Returns bits [n_seg][blocks_per_seg][K], metric and tb_ok [n_seg][blocks_per_seg]."""
    n_seg = llr_seg.shape[0]
    x = np.ascontiguousarray(llr_seg[:, :blocks_per_seg * 3 * K]).reshape(n_seg * blocks_per_seg, 3 * K)
    b, m, ok = decode(x)
    return b.reshape(n_seg, blocks_per_seg, K), m.reshape(n_seg, blocks_per_seg), ok.reshape(n_seg, blocks_per_seg)


def awgn_llrs(coded: np.ndarray, esn0_db: float, rng) -> np.ndarray:
    """BPSK over AWGN: y = (1 - 2 e) + n, n ~ N(0, sigma^2), sigma^2 = 1 / (2 Es/N0); LLR = 2 y / sigma^2 (positive = bit 0)."""
    s2 = 1.0 / (2.0 * 10.0 ** (esn0_db / 10.0))
    y = 1.0 - 2.0 * coded.astype(np.float64) + rng.standard_normal(coded.shape) * np.sqrt(s2)
    return (2.0 * y / s2).astype(np.float32)
