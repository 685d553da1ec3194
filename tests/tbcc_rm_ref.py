"""The rate-matching contract of include/ofdm_mi355x.h (TS 36.212 5.1.4.2: sub-block interleaver and circular buffer of the
tail-biting convolutional code) restated in NumPy float32, vectorised over code blocks.  Encoding and decoding proper are
tests/tbcc_ref.py's; this file adds the bit order, the puncturing / repetition and the de-matching sum.  Every float operation
below is one IEEE float32 operation in the order the contract writes it.  tests/test_tbcc_rm_ref_host.py pins this file by
independent means."""
import functools

import numpy as np

import tbcc_ref

P = (1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30)
P_INV = tuple(int(x) for x in np.argsort(P))
MAX_COPIES = 16


def valid_e(K, E) -> bool:
    return tbcc_ref.valid_k(K) and 1 <= E <= 3 * MAX_COPIES * K


def rm_blocks(seg_bits: int, K: int, E: int) -> int:
    if not valid_e(K, E) or seg_bits < 0:
        raise ValueError("bad K, E or seg_bits")
    return seg_bits // E


def geometry(K):
    """-> (R, ND, nullmask): rows of the 32-column matrix, NULLs in front of a stream, bit c set iff column c starts with a NULL"""
    R = -(-K // 32)
    ND = 32 * R - K
    return R, ND, sum(1 << c for c in range(32) if P[c] < ND)


def _popcount(x):
    x = np.asarray(x, np.int64)
    n = np.zeros_like(x)
    for b in range(32):
        n += (x >> b) & 1
    return n


def rank(K, j, i):
    """position of coded bit dj[i] in the circular buffer with the NULLs taken out: 0 <= rank < 3K (j, i scalars or arrays)"""
    R, ND, nullmask = geometry(K)
    y = ND + np.asarray(i, np.int64)
    row, c = y >> 5, np.asarray(P_INV, np.int64)[y & 31]
    return np.asarray(j, np.int64) * K + c * R + row - _popcount(nullmask & ((np.int64(2) << c) - 1))


def inverse(K, q):
    """rank -> (j, i), the encoder's direction: c is the largest column with cum(c) <= the rank inside the stream"""
    R, ND, nullmask = geometry(K)
    q = np.asarray(q, np.int64)
    j, r = q // K, q % K
    cols = np.arange(32, dtype=np.int64)
    cum = cols * R - _popcount(nullmask & ((np.int64(1) << cols) - 1))
    c = np.searchsorted(cum, r, side="right") - 1
    p = np.asarray(P, np.int64)[c]
    row = r - cum[c] + (p < ND)
    return j, 32 * row + p - ND


@functools.lru_cache(maxsize=None)
def order(K):
    """-> pos [3K]: pos[q] = 3 i + j of the coded bit of rank q (an index into tbcc_ref.encode's output); read-only"""
    i = np.repeat(np.arange(K), 3)
    j = np.tile(np.arange(3), K)
    pos = np.empty(3 * K, np.int64)
    pos[rank(K, j, i)] = 3 * i + j
    pos.setflags(write=False)
    return pos


def rate_match(e, E):
    """e [..., 3K] coded bits in tbcc_ref.encode's order -> [..., E]: e_k = the coded bit of rank k mod 3K"""
    K = e.shape[-1] // 3
    assert valid_e(K, E)
    return e[..., order(K)[np.arange(E) % (3 * K)]]


def rm_encode_segments(info, E, seg_bits):
    """info [n_seg][blocks_per_seg][K] -> [n_seg][seg_bits]: E bits per block back to back from bit 0, then zeros"""
    n_seg, bps, K = info.shape
    assert bps * E <= seg_bits
    out = np.zeros((n_seg, seg_bits), np.uint8)
    out[:, :bps * E] = rate_match(tbcc_ref.encode(info), E).reshape(n_seg, bps * E)
    return out


def _v(x):
    return np.where(np.isfinite(x), x, np.float32(0)).astype(np.float32)


def dematch(llr, K):
    """llr [n_blocks][E] float32 -> [n_blocks][3K] float32 in tbcc_ref.decode's order.  Per rank q: +0 where q >= E, else
    v(l[q]) and then + v(l[q + m 3K]) for m = 1, 2, .. while the index is < E, one float32 addition at a time."""
    llr = np.ascontiguousarray(llr, np.float32)
    nb, E = llr.shape
    assert valid_e(K, E)
    n3 = 3 * K
    acc = np.zeros((nb, n3), np.float32)                       # by rank
    n = min(E, n3)
    acc[:, :n] = _v(llr[:, :n])
    with np.errstate(over="ignore"):
        for lo in range(n3, E, n3):
            n = min(E, lo + n3) - lo
            acc[:, :n] = acc[:, :n] + _v(llr[:, lo:lo + n])
    assert acc.dtype == np.float32
    out = np.empty_like(acc)
    out[:, order(K)] = acc
    return out


def decode_rm(llr, K):
    """llr [n_blocks][E] -> (bits, metric, tb_ok) of tbcc_ref.decode on the de-matched LLRs (it takes a sum that is not finite as 0)"""
    return tbcc_ref.decode(dematch(llr, K))


def decode_rm_segments(llr_seg, blocks_per_seg, K, E):
    """llr_seg [n_seg][>= blocks_per_seg*E] -> bits [n_seg][blocks_per_seg][K], metric and tb_ok [n_seg][blocks_per_seg]"""
    n_seg = llr_seg.shape[0]
    x = np.ascontiguousarray(llr_seg[:, :blocks_per_seg * E]).reshape(n_seg * blocks_per_seg, E)
    b, m, ok = decode_rm(x, K)
    return b.reshape(n_seg, blocks_per_seg, K), m.reshape(n_seg, blocks_per_seg), ok.reshape(n_seg, blocks_per_seg)
