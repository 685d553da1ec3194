"""The transport-block layer of include/ofdm_mi355x.h ("transport block") written literally: CRC by bit-serial long division
(tests/lte_bits_ref.py), segmentation as TS 36.212 5.1.2 words it, coding through tests/turbo_ref.py and tests/turbo_rm_ref.py,
concatenation, and the receive chain with a scalar-order soft buffer.  No table, no chunking, no byte arithmetic: this file is the
yardstick of csrc/tb.hip and csrc/capi_tb.hip, held to with array_equal; tests/test_tb_ref_host.py pins it by means that do not
share its code."""
import numpy as np

import lte_bits_ref as lb
import turbo_ref
import turbo_rm_ref as rm

F32 = np.float32
A_MIN, A_MAX = 8, (1 << 20) - 24
LTE_KS = tuple(list(range(40, 513, 8)) + list(range(528, 1025, 16)) + list(range(1056, 2049, 32)) + list(range(2112, 6145, 64)))


def k_next(bits):
    """the smallest valid K >= bits, None above 6144"""
    for K in LTE_KS:
        if K >= bits:
            return K
    return None


def segmentation(A, Z=0):
    """-> dict(A, Z, B, L, C, K_plus, K_minus, C_plus, C_minus, F, Ks = K_r per block), or None where the contract refuses"""
    Z = 6144 if Z == 0 else Z
    if Z not in LTE_KS or A % 8 or not A_MIN <= A <= A_MAX:
        return None
    B = A + 24
    if B <= Z:
        L, C, Bp = 0, 1, B
    else:
        L = 24
        C = -(-B // (Z - L))
        Bp = B + C * L
    K_plus = min(K for K in LTE_KS if C * K >= Bp)
    if C == 1:
        C_plus, K_minus, C_minus = 1, 0, 0
    else:
        below = [K for K in LTE_KS if K < K_plus]
        K_minus = max(below) if below else 0
        dK = K_plus - K_minus if below else 8
        C_minus = (C * K_plus - Bp) // dK
        C_plus = C - C_minus
        if C_minus > 0 and not below:
            return None
    F = C_plus * K_plus + C_minus * K_minus - Bp
    return dict(A=A, Z=Z, B=B, L=L, C=C, K_plus=K_plus, K_minus=K_minus, C_plus=C_plus, C_minus=C_minus, F=F,
                Ks=[K_minus] * C_minus + [K_plus] * C_plus)


def geometry(A, Z=0, G=0, q=1, N_IR=0):
    """segmentation plus, for G > 0, G, q, gamma, E0, E1, Es = E_r per block, Ncbs = Ncb_r per block; always soft_floats and
    groups = [dict(first, count, K, E, cw_bit_offset, soft_offset)]: the maximal runs of blocks with one (K, E).  None where the
    contract refuses."""
    g = segmentation(A, Z)
    if g is None:
        return None
    C, Ks = g["C"], g["Ks"]
    g["soft_floats"] = sum(3 * K + 12 for K in Ks)
    Es = [0] * C
    if G:
        if not 0 < G < 2 ** 31 or q < 1 or G % q or N_IR < 0:
            return None
        Gp = G // q
        gamma = Gp % C
        Es = [q * (Gp // C) if r <= C - gamma - 1 else q * (-(-Gp // C)) for r in range(C)]
        Ncbs = []
        for K in Ks:
            _, _, Kpi, _, Kw = rm.dims(K)
            Ncb = min(N_IR // C, Kw) if N_IR else Kw
            if Ncb < Kpi:
                return None
            Ncbs.append(Ncb)
        if any(not rm.valid_e(K, Ncb, E) for K, Ncb, E in zip(Ks, Ncbs, Es)):
            return None
        g.update(G=G, q=q, gamma=gamma, E0=Es[0], E1=Es[-1], Es=Es, Ncbs=Ncbs)
    groups, cw, soft = [], 0, 0
    for r in range(C):
        if groups and (groups[-1]["K"], groups[-1]["E"]) == (Ks[r], Es[r]):
            groups[-1]["count"] += 1
        else:
            groups.append(dict(first=r, count=1, K=Ks[r], E=Es[r], cw_bit_offset=cw, soft_offset=soft))
        cw, soft = cw + Es[r], soft + 3 * Ks[r] + 12
    g["groups"] = groups
    return g


def segment(payload, Z=0):
    """payload [A] bits -> (list of C code blocks, geometry): CRC24A attached, F filler zeros in front, CRC24B per block if C > 1"""
    payload = np.asarray(payload, np.uint8) & 1
    g = segmentation(payload.size, Z)
    b = np.concatenate([payload, lb.int_bits(lb.crc(payload, lb.CRC24A), 24)])
    seq = np.concatenate([np.zeros(g["F"], np.uint8), b])
    blocks, s = [], 0
    for K in g["Ks"]:
        part = seq[s:s + K - g["L"]]
        s += K - g["L"]
        if g["L"]:
            part = np.concatenate([part, lb.int_bits(lb.crc(part, lb.CRC24B), 24)])
        blocks.append(part)
    assert s == seq.size
    return blocks, g


def desegment(blocks, A, Z=0):
    """decoded code blocks -> (payload [A], tb_ok, cb_ok [C], syndrome)"""
    g = segmentation(A, Z)
    parts, cb_ok = [], []
    for blk in blocks:
        blk = np.asarray(blk, np.uint8) & 1
        if g["L"]:
            cb_ok.append(int(lb.crc(blk[:-24], lb.CRC24B) == lb.bits_int(blk[-24:])))
            parts.append(blk[:-24])
        else:
            cb_ok.append(1)
            parts.append(blk)
    b = np.concatenate(parts)[g["F"]:]
    assert b.size == g["B"]
    syn = lb.crc(b[:A], lb.CRC24A) ^ lb.bits_int(b[A:])
    return b[:A].copy(), int(syn == 0), np.array(cb_ok, np.uint8), syn


def _pair(K, g, qpp_minus, qpp_plus):
    return qpp_minus if K == g["K_minus"] and g["C_minus"] else qpp_plus


def encode_blocks(blocks, A, G, qpp_minus, qpp_plus, Z=0, q=1, N_IR=0, rv=0, cw_bits=None):
    """blocks[t][r] = code block r of transport block t, as segment() gives it or with bits changed on purpose ->
    codewords [n_tb][cw_bits]: block r's E_r rate-matched bits back to back, zeros from G on; rv one value or one per transport
    block"""
    n_tb = len(blocks)
    g = geometry(A, Z, G, q, N_IR)
    cw_bits = G if cw_bits is None else cw_bits
    rvs = np.broadcast_to(np.asarray(rv, np.int64), (n_tb,)) & 3
    out = np.zeros((n_tb, cw_bits), np.uint8)
    at = 0
    for r in range(g["C"]):                                  # block r of every transport block at once, one rv at a time
        K, E = g["Ks"][r], g["Es"][r]
        e = turbo_ref.encode(np.stack([np.asarray(blocks[t][r], np.uint8) for t in range(n_tb)]), *_pair(K, g, qpp_minus, qpp_plus))
        for v in sorted(set(int(x) for x in rvs)):
            idx = np.flatnonzero(rvs == v)
            out[idx, at:at + E] = rm.rate_match(e[idx], E, g["Ncbs"][r], v)
        at += E
    assert at == G
    return out


def encode(payloads, G, qpp_minus, qpp_plus, Z=0, q=1, N_IR=0, rv=0, cw_bits=None):
    """payloads [n_tb][A] -> codewords [n_tb][cw_bits]"""
    payloads = np.asarray(payloads, np.uint8)
    return encode_blocks([segment(p, Z)[0] for p in payloads], payloads.shape[1], G, qpp_minus, qpp_plus, Z, q, N_IR, rv, cw_bits)


def decode(llr, A, G, qpp_minus, qpp_plus, n_iter, Z=0, q=1, N_IR=0, rv=0, soft=None):
    """llr [n_tb][>= G] float32, soft [n_tb][>= soft_floats] or None (accumulate onto it) ->
    (payload [n_tb][A], tb_ok [n_tb], cb_ok [n_tb][C], syndrome [n_tb] uint32, soft [n_tb][soft_floats])"""
    llr = np.asarray(llr, F32)
    n_tb = llr.shape[0]
    g = geometry(A, Z, G, q, N_IR)
    rvs = np.broadcast_to(np.asarray(rv, np.int64), (n_tb,))
    payload = np.zeros((n_tb, A), np.uint8)
    tb_ok = np.zeros(n_tb, np.uint8)
    cb_ok = np.zeros((n_tb, g["C"]), np.uint8)
    syn = np.zeros(n_tb, np.uint32)
    new_soft = np.zeros((n_tb, g["soft_floats"]), F32)
    at, sat, bits = 0, 0, []
    for r in range(g["C"]):                                  # block r of every transport block at once, one rv at a time
        K, E = g["Ks"][r], g["Es"][r]
        n = 3 * K + 12
        dec = np.zeros((n_tb, K), np.uint8)
        for v in sorted(set(int(x) & 3 for x in rvs)):
            idx = np.flatnonzero((rvs & 3) == v)
            old = None if soft is None else np.asarray(soft, F32)[idx, sat:sat + n]
            s = rm.dematch(llr[idx, at:at + E], K, g["Ncbs"][r], v, old)
            new_soft[idx, sat:sat + n] = s
            dec[idx] = turbo_ref.decode(s, *_pair(K, g, qpp_minus, qpp_plus), n_iter)[0]
        bits.append(dec)
        at, sat = at + E, sat + n
    for t in range(n_tb):
        payload[t], tb_ok[t], cb_ok[t], syn[t] = desegment([b[t] for b in bits], A, Z)
    return payload, tb_ok, cb_ok, syn, new_soft
