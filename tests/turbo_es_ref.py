"""The turbo decoder with early termination by CRC (ofdm_turbo_decode_es_frames) as include/ofdm_mi355x.h defines it, in NumPy:
one loop over iterations around turbo_ref.siso with a freeze mask per block and the CRC as lte_bits_ref.poly_mod over all K hard
decisions.  The yardstick of csrc/turbo_es.hip; tests/test_turbo_es_ref_host.py pins it by the definition (turbo_ref.decode at
every n_iter, first n whose bits pass lte_bits_ref.crc_check), which shares no control flow with this file."""
import numpy as np

import lte_bits_ref as lb
import turbo_ref as tr

F32 = np.float32


def decode_es(llr, f1, f2, crc_kind, min_iter, max_iter):
    """llr [n][3K + 12] float32 -> (bits [n][K] uint8, llr_out [n][K] float32, iters [n] uint8, crc_ok [n] uint8)"""
    llr = np.ascontiguousarray(llr, F32)
    n, K = llr.shape[0], (llr.shape[1] - 12) // 3
    assert llr.shape[1] == 3 * K + 12 and tr.qpp_check(K, f1, f2) and 1 <= min_iter <= max_iter <= tr.ITER_MAX
    l = np.where(np.isfinite(llr), llr, F32(0)).astype(F32)
    pi = tr.qpp(K, f1, f2)
    ls, lp1, lp2 = l[:, 0:3 * K:3], l[:, 1:3 * K:3], l[:, 2:3 * K:3]
    t1, t2 = l[:, 3 * K:3 * K + 6], l[:, 3 * K + 6:]
    ls2 = ls[:, pi]
    la1 = np.zeros((n, K), F32)
    out = np.zeros((n, K), F32)
    iters = np.zeros(n, np.uint8)
    ok = np.zeros(n, np.uint8)
    live = np.ones(n, bool)
    for it in range(1, max_iter + 1):
        w = np.flatnonzero(live)                             # frozen blocks are not touched again
        if not len(w):
            break
        _, e1 = tr.siso(ls[w], la1[w], lp1[w], t1[w])
        post2, e2 = tr.siso(ls2[w], e1[:, pi], lp2[w], t2[w])
        nxt = np.empty((len(w), K), F32)
        nxt[:, pi] = e2
        la1[w] = nxt
        if it < min_iter:
            continue
        post = np.empty((len(w), K), F32)
        post[:, pi] = post2
        out[w] = post
        iters[w] = it
        for j, blk in enumerate(w):
            if lb.poly_mod((post[j] < 0).astype(np.uint8), crc_kind) == 0:
                ok[blk] = 1
                live[blk] = False
    return (out < 0).astype(np.uint8), out, iters, ok


def tb_decode_es(llr, A, G, qpp_minus, qpp_plus, min_iter, max_iter, Z=0, q=1, N_IR=0, rv=0, soft=None):
    """tb_ref.decode with every code block through decode_es (CRC24B, or CRC24A when C = 1) ->
    (payload [n_tb][A], tb_ok [n_tb], cb_ok [n_tb][C], syndrome [n_tb] uint32, soft [n_tb][soft_floats], cb_iters [n_tb][C])"""
    import tb_ref
    import turbo_rm_ref as rm
    llr = np.asarray(llr, F32)
    n_tb = llr.shape[0]
    g = tb_ref.geometry(A, Z, G, q, N_IR)
    kind = lb.CRC24B if g["L"] else lb.CRC24A
    rvs = np.broadcast_to(np.asarray(rv, np.int64), (n_tb,)) & 3
    new_soft = np.zeros((n_tb, g["soft_floats"]), F32)
    cb_iters = np.zeros((n_tb, g["C"]), np.uint8)
    at, sat, bits = 0, 0, []
    for r in range(g["C"]):
        K, E = g["Ks"][r], g["Es"][r]
        n = 3 * K + 12
        for v in sorted(set(int(x) for x in rvs)):
            idx = np.flatnonzero(rvs == v)
            old = None if soft is None else np.asarray(soft, F32)[idx, sat:sat + n]
            new_soft[idx, sat:sat + n] = rm.dematch(llr[idx, at:at + E], K, g["Ncbs"][r], v, old)
        pair = qpp_minus if K == g["K_minus"] and g["C_minus"] else qpp_plus
        dec, _, cb_iters[:, r], _ = decode_es(new_soft[:, sat:sat + n], *pair, kind, min_iter, max_iter)
        bits.append(dec)
        at, sat = at + E, sat + n
    payload = np.zeros((n_tb, A), np.uint8)
    tb_ok = np.zeros(n_tb, np.uint8)
    cb_ok = np.zeros((n_tb, g["C"]), np.uint8)
    syn = np.zeros(n_tb, np.uint32)
    for t in range(n_tb):
        payload[t], tb_ok[t], cb_ok[t], syn[t] = tb_ref.desegment([b[t] for b in bits], A, Z)
    return payload, tb_ok, cb_ok, syn, new_soft, cb_iters
