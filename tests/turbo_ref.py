"""The LTE turbo codec of the frame-batched path as include/ofdm_mi355x.h defines it, in NumPy float32 and vectorised over code
blocks: the yardstick the kernels are held to with array_equal.  Nothing else lives here; tests/test_turbo_ref_host.py pins this
file by independent means."""
import numpy as np

F32 = np.float32
K_MIN, K_MAX, ITER_MAX = 40, 6144, 16
SIG = np.array([1.0, -1.0], F32)

# trellis of one constituent encoder: state s = 4 r1 + 2 r2 + r3, input u -> a = u ^ r2 ^ r3, z = a ^ r1 ^ r3, next = 4 a + (s >> 1)
NEXT = np.zeros((8, 2), np.int64)
PAR = np.zeros((8, 2), np.int64)
for _s in range(8):
    for _u in range(2):
        _r1, _r2, _r3 = _s >> 2, (_s >> 1) & 1, _s & 1
        _a = _u ^ _r2 ^ _r3
        NEXT[_s, _u], PAR[_s, _u] = 4 * _a + (_s >> 1), _a ^ _r1 ^ _r3
# the two branches (s, u) -> s' of every s', the lower s first
PRED_S = np.zeros((8, 2), np.int64)
PRED_U = np.zeros((8, 2), np.int64)
for _t in range(8):
    _br = sorted((s, u) for s in range(8) for u in range(2) if NEXT[s, u] == _t)
    assert len(_br) == 2
    for _b, (_s, _u) in enumerate(_br):
        PRED_S[_t, _b], PRED_U[_t, _b] = _s, _u
PRED_Z = PAR[PRED_S, PRED_U]


def valid_k(K):
    return K_MIN <= K <= K_MAX and K % 8 == 0


def blocks(seg_bits, K):
    return seg_bits // (3 * K + 12)


def qpp(K, f1, f2):
    """pi(i) = (f1 i + f2 i^2) mod K, i = 0 .. K-1, in Python integers"""
    return np.array([(f1 * i + f2 * i * i) % K for i in range(K)], np.int64)


def qpp_check(K, f1, f2):
    if not (valid_k(K) and 0 <= f1 < K and 0 <= f2 < K):
        return False
    return bool(np.array_equal(np.sort(qpp(K, f1, f2)), np.arange(K)))


def rsc(c):
    """one constituent encoder over c [n][K] -> (z [n][K], tail [n][6] = x_K z_K x_{K+1} z_{K+1} x_{K+2} z_{K+2}, end state [n])"""
    c = np.asarray(c, np.uint8)
    n, K = c.shape
    r1 = np.zeros(n, np.uint8)
    r2, r3 = r1.copy(), r1.copy()
    z = np.empty((n, K), np.uint8)
    for k in range(K):
        a = c[:, k] ^ r2 ^ r3
        z[:, k] = a ^ r1 ^ r3
        r1, r2, r3 = a, r1, r2
    tail = np.empty((n, 6), np.uint8)
    for j in range(3):
        tail[:, 2 * j] = r2 ^ r3                             # u: makes a = 0
        tail[:, 2 * j + 1] = r1 ^ r3
        r1, r2, r3 = np.zeros(n, np.uint8), r1, r2
    return z, tail, 4 * r1 + 2 * r2 + r3


def encode(c, f1, f2):
    """c [n][K] -> e [n][3K + 12]: e[3k + j] = dj[k], then the 12 tail bits"""
    c = np.asarray(c, np.uint8)
    n, K = c.shape
    z1, t1, _ = rsc(c)
    z2, t2, _ = rsc(c[:, qpp(K, f1, f2)])
    e = np.empty((n, 3 * K + 12), np.uint8)
    e[:, 0:3 * K:3], e[:, 1:3 * K:3], e[:, 2:3 * K:3] = c, z1, z2
    e[:, 3 * K:3 * K + 6], e[:, 3 * K + 6:] = t1, t2
    return e


def encode_segments(info, f1, f2, seg_bits):
    """info [n_seg][bps][K] -> [n_seg][seg_bits]: the blocks back to back from bit 0, filler zeros behind them"""
    n_seg, bps, K = info.shape
    out = np.zeros((n_seg, seg_bits), np.uint8)
    if bps:
        out[:, :bps * (3 * K + 12)] = encode(info.reshape(n_seg * bps, K), f1, f2).reshape(n_seg, -1)
    return out


def siso(ls, la, lp, t):
    """ls, la, lp [n][K], t [n][6], all float32 -> (post [n][K], ext [n][K])"""
    n, K = ls.shape
    with np.errstate(invalid="ignore", over="ignore"):
        x = ls + la
        A = np.empty((K + 1, n, 8), F32)
        A[0] = -np.inf
        A[0, :, 0] = 0
        for k in range(K):
            xk, lk = x[:, k:k + 1], lp[:, k:k + 1]
            c0 = A[k][:, PRED_S[:, 0]] + (SIG[PRED_U[:, 0]] * xk + SIG[PRED_Z[:, 0]] * lk)
            c1 = A[k][:, PRED_S[:, 1]] + (SIG[PRED_U[:, 1]] * xk + SIG[PRED_Z[:, 1]] * lk)
            m = np.maximum(c0, c1)
            A[k + 1] = m - m[:, 0:1] if (k + 1) % 8 == 0 else m
        g = []
        s = np.arange(8)
        for j in range(3):
            r1, r2, r3 = s >> 2, (s >> 1) & 1, s & 1
            g.append(SIG[r2 ^ r3] * t[:, 2 * j:2 * j + 1] + SIG[r1 ^ r3] * t[:, 2 * j + 1:2 * j + 2])
            s = s >> 1
        b = (g[0] + g[1]) + g[2]
        B = b - b[:, 0:1]
        post = np.empty((n, K), F32)
        ext = np.empty((n, K), F32)
        for k in range(K - 1, -1, -1):
            xk, lk = x[:, k:k + 1], lp[:, k:k + 1]
            g0 = SIG[0] * xk + SIG[PAR[:, 0]] * lk           # gamma_k(0, z) per state
            g1 = SIG[1] * xk + SIG[PAR[:, 1]] * lk
            b0, b1 = B[:, NEXT[:, 0]], B[:, NEXT[:, 1]]
            M0 = ((A[k] + g0) + b0).max(axis=1)
            M1 = ((A[k] + g1) + b1).max(axis=1)
            post[:, k] = F32(0.5) * (M0 - M1)
            ext[:, k] = F32(0.75) * (post[:, k] - x[:, k])
            nn = np.maximum(g0 + b0, g1 + b1)
            B = nn - nn[:, 0:1] if k % 8 == 0 else nn
    assert post.dtype == F32 and ext.dtype == F32 and A.dtype == F32 and B.dtype == F32
    return post, ext


def decode(llr, f1, f2, n_iter):
    """llr [n][3K + 12] float32 -> (bits [n][K] uint8, llr_out [n][K] float32)"""
    llr = np.ascontiguousarray(llr, F32)
    n, K = llr.shape[0], (llr.shape[1] - 12) // 3
    assert llr.shape[1] == 3 * K + 12 and qpp_check(K, f1, f2) and 1 <= n_iter <= ITER_MAX
    l = np.where(np.isfinite(llr), llr, F32(0)).astype(F32)
    pi = qpp(K, f1, f2)
    ls, lp1, lp2 = l[:, 0:3 * K:3], l[:, 1:3 * K:3], l[:, 2:3 * K:3]
    t1, t2 = l[:, 3 * K:3 * K + 6], l[:, 3 * K + 6:]
    la1 = np.zeros((n, K), F32)
    ls2 = ls[:, pi]
    for _ in range(n_iter):
        _, e1 = siso(ls, la1, lp1, t1)
        post2, e2 = siso(ls2, e1[:, pi], lp2, t2)
        la1 = np.empty((n, K), F32)
        la1[:, pi] = e2
    out = np.empty((n, K), F32)
    out[:, pi] = post2
    return (out < 0).astype(np.uint8), out


def decode_segments(llr_seg, bps, K, f1, f2, n_iter):
    """llr_seg [n_seg][stride] -> (bits [n_seg][bps][K], llr [n_seg][bps][K])"""
    n_seg = llr_seg.shape[0]
    blk = np.ascontiguousarray(llr_seg[:, :bps * (3 * K + 12)]).reshape(n_seg * bps, 3 * K + 12)
    bits, out = decode(blk, f1, f2, n_iter)
    return bits.reshape(n_seg, bps, K), out.reshape(n_seg, bps, K)


def awgn_llrs(e, esn0_db, rng):
    """BPSK (bit 0 -> +1) over AWGN at Es/N0, LLR = 2 y / sigma^2 -> float32"""
    sigma2 = 0.5 * 10.0 ** (-esn0_db / 10.0)
    y = (1.0 - 2.0 * np.asarray(e, np.float64)) + np.sqrt(sigma2) * rng.standard_normal(np.shape(e))
    return (2.0 * y / sigma2).astype(F32)
