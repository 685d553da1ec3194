"""Rate matching of the LTE turbo code (TS 36.212 5.1.4.1) as include/ofdm_mi355x.h defines it, written literally: NULL-prefixed
R x 32 matrices, the column permutation, pi2 for the third stream, the interlaced circular buffer and the walk that skips the
NULLs; de-matching as a float32 sum in scalar order.  It sits on top of tests/turbo_ref.py and is the yardstick the kernels are
held to with array_equal.  tests/test_turbo_rm_ref_host.py pins this file by means that do not share its code."""
import functools

import numpy as np

import turbo_ref

F32 = np.float32
NULL = -1
MAX_COPIES = 16
P = [0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31]


def dims(K):
    """-> (D, R, Kpi, ND, Kw)"""
    D = K + 4
    R = -(-D // 32)
    return D, R, 32 * R, 32 * R - D, 96 * R


def norm_ncb(K, Ncb):
    return dims(K)[4] if Ncb == 0 else Ncb


def valid_ncb(K, Ncb):
    _, _, Kpi, _, Kw = dims(K)
    return Ncb == 0 or Kpi <= Ncb <= Kw


@functools.lru_cache(maxsize=None)
def buffer_index(K):
    """w as coded-bit indices: w[k] = 3i + j of the coded bit dj[i] that sits there, NULL where the buffer holds a NULL"""
    D, R, Kpi, ND, Kw = dims(K)
    P_ = np.array(P)
    v = []
    for j in range(3):
        y = np.concatenate([np.full(ND, NULL, np.int64), 3 * np.arange(D, dtype=np.int64) + j])
        if j < 2:
            mat = y.reshape(R, 32)                                           # row by row
            perm = mat[:, P_]                                                # column c of the permuted matrix = column P[c]
            v.append(perm.T.reshape(-1))                                     # column by column
        else:
            k = np.arange(Kpi)
            v.append(y[(P_[k // R] + 32 * (k % R) + 1) % Kpi])
    w = np.full(Kw, NULL, np.int64)
    w[:Kpi] = v[0]
    w[Kpi::2] = v[1]
    w[Kpi + 1::2] = v[2]
    w.setflags(write=False)
    return w


def k0(K, Ncb, rv):
    _, R, _, _, _ = dims(K)
    Ncb = norm_ncb(K, Ncb)
    return R * (2 * (-(-Ncb // (8 * R))) * rv + 2)


def n_avail(K, Ncb):
    return int((buffer_index(K)[:norm_ncb(K, Ncb)] != NULL).sum())


def valid_e(K, Ncb, E):
    return 1 <= E <= MAX_COPIES * n_avail(K, Ncb)


def rm_blocks(seg_bits, K, E):
    return seg_bits // E


@functools.lru_cache(maxsize=4096)
def selection(K, E, Ncb, rv):
    """sel [E]: e_k = coded bit sel[k] of the block -- the circular walk from k0 over w[0 .. Ncb), NULLs skipped"""
    assert turbo_ref.valid_k(K) and valid_ncb(K, Ncb) and 0 <= rv <= 3 and valid_e(K, Ncb, E)
    w = buffer_index(K)
    Ncb = norm_ncb(K, Ncb)
    start = k0(K, Ncb, rv)
    turn = w[(start + np.arange(Ncb)) % Ncb]                 # one turn of the buffer from k0 ...
    turn = turn[turn != NULL]                                # ... with the NULLs skipped
    sel = np.tile(turn, -(-E // len(turn)))[:E].copy()       # and as many turns as E takes
    sel.setflags(write=False)
    return sel


def rate_match(e, E, Ncb, rv):
    """e [n][3K + 12] coded blocks (turbo_ref.encode) -> [n][E]"""
    e = np.asarray(e)
    K = (e.shape[1] - 12) // 3
    return e[:, selection(K, E, Ncb, rv)]


def encode_rm_segments(info, f1, f2, E, Ncb, rv, seg_bits):
    """info [n_seg][bps][K] -> [n_seg][seg_bits]: block b at segment bit b*E, filler zeros behind the last block; rv is one
    value or one per segment"""
    n_seg, bps, K = info.shape
    out = np.zeros((n_seg, seg_bits), np.uint8)
    rvs = np.broadcast_to(np.asarray(rv), (n_seg,))
    for s in range(n_seg):
        if bps:
            out[s, :bps * E] = rate_match(turbo_ref.encode(info[s], f1, f2), E, Ncb, int(rvs[s]) & 3).reshape(-1)
    return out


def dematch(l, K, Ncb, rv, old=None):
    """l [n][E] float32 -> [n][3K + 12] float32: per coded bit the copies added one at a time in increasing index of e, a bit
    that is never sent +0; with old [n][3K + 12], old + L in one more float32 addition (HARQ combining)"""
    l = np.ascontiguousarray(l, F32)
    n, E = l.shape
    sel = selection(K, E, Ncb, rv)
    v = np.where(np.isfinite(l), l, F32(0)).astype(F32)
    out = np.zeros((n, 3 * K + 12), F32)
    seen = np.zeros(3 * K + 12, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(E):                                   # scalar order: copy m of a bit is added after copy m - 1
            x = sel[k]
            out[:, x] = out[:, x] + v[:, k] if seen[x] else v[:, k]
            seen[x] = True
        if old is not None:
            out = np.ascontiguousarray(old, F32) + out
    assert out.dtype == F32
    return out


def dematch_segments(llr_seg, bps, K, E, Ncb, rv, old=None):
    """llr_seg [n_seg][stride] -> [n_seg][bps][3K + 12]; rv one value or one per segment, old [n_seg][bps][3K + 12] or None"""
    n_seg = llr_seg.shape[0]
    rvs = np.broadcast_to(np.asarray(rv), (n_seg,))
    out = np.empty((n_seg, bps, 3 * K + 12), F32)
    for s in range(n_seg):
        blk = np.ascontiguousarray(llr_seg[s, :bps * E]).reshape(bps, E)
        out[s] = dematch(blk, K, Ncb, int(rvs[s]) & 3, None if old is None else old[s])
    return out
