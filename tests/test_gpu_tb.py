"""The transport-block layer on the GPU (-m gpu): ofdm_tx_tb_encode_frames and ofdm_tb_decode_frames -- csrc/tb.hip's segment,
concat and desegment kernels around the untouched encoder, de-matcher and decoder -- against tests/tb_ref.py (the contract
written literally).  Every comparison is array_equal, floats by their bit pattern, and every output sits between poisoned guard
bands.  The HARQ chain runs at the point tests/test_tb_ref_host.py asserts on the reference alone."""
import numpy as np
import pytest

import tb_cases as tc
import tb_ref
import turbo_ref as tr
import turbo_rm_ref as rm

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]       # (payload packed, codeword packed)


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def rx0(om, torch):
    """any receiver handle serves this layer (it reads LLR buffers, not the handle's numerology)"""
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


@pytest.fixture(scope="module")
def tx0(om, torch):
    return om.TxEngine(64, 16, 62, 60)


def pack_msb(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="big")


class Guarded:
    """nbytes of device memory at .addr = allocation + 64 + off, everything poisoned (or `fill`ed); read() returns the payload
    after asserting that the bytes in front of it and the 64 behind it are still poison"""

    def __init__(self, om, nbytes, off=0, fill=None):
        self.nbytes, self.lo = int(nbytes), GUARD + off
        self.total = self.lo + self.nbytes + GUARD
        raw = np.full(self.total, POISON, np.uint8)
        if fill is not None:
            raw[self.lo:self.lo + self.nbytes] = np.ascontiguousarray(fill).view(np.uint8).ravel()
        self.buf = om.DeviceBuffer(self.total).upload(raw)
        self.addr = self.buf.data_ptr() + self.lo

    def read(self, dtype=np.uint8):
        raw = self.buf.download(np.uint8, self.total)
        assert np.all(raw[:self.lo] == POISON), "%d bytes written IN FRONT of an output" % int((raw[:self.lo] != POISON).sum())
        tail = raw[self.lo + self.nbytes:]
        assert np.all(tail == POISON), "%d bytes written BEHIND an output" % int((tail != POISON).sum())
        return raw[self.lo:self.lo + self.nbytes].copy().view(dtype)

    def untouched(self):
        return bool(np.all(self.read() == POISON))


def dev(om, arr):
    arr = np.ascontiguousarray(arr)
    return om.DeviceBuffer(max(arr.nbytes, 4)).upload(arr)


def bits_equal(a, b):
    """float32 arrays equal by bit pattern"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_pairs(om, A, Z):
    qm, qp = tc.pairs(A, Z)
    g = tb_ref.segmentation(A, Z)
    assert om.turbo_qpp_check(g["K_plus"], *qp) and (not g["C_minus"] or om.turbo_qpp_check(g["K_minus"], *qm))
    return qm, qp


def gpu_encode(om, tx, p, Z, G, q=1, N_IR=0, rv=0, d_rv=None, cw_bits=None, pay_packed=False, cw_packed=False, off=0, pay_off=0):
    """p [n_tb][A] -> the codeword buffer's bytes [n_tb][row], written at allocation + 64 + off; the payload is read from
    its allocation + pay_off"""
    n_tb, A = p.shape
    qm, qp = tc.pairs(A, Z)
    cw_bits = G if cw_bits is None else cw_bits
    src = np.ascontiguousarray(pack_msb(p) if pay_packed else p).ravel()
    d_src = dev(om, np.concatenate([np.full(pay_off, POISON, np.uint8), src]))
    row = cw_bits // 8 if cw_packed else cw_bits
    g = Guarded(om, n_tb * row, off)
    tx.tb_encode_frames(d_src.data_ptr() + pay_off, n_tb, A, G, qp, g.addr, cw_bits, qpp_minus=qm, Z=Z, q=q, N_IR=N_IR, rv=rv, d_rv=d_rv,
                        payload_mode=om.BITS_PACKED if pay_packed else om.BITS_UNPACKED,
                        cw_mode=om.BITS_PACKED if cw_packed else om.BITS_UNPACKED)
    return g.read().reshape(n_tb, row)


def gpu_decode(om, rx, llr, A, Z, G, n_iter, q=1, N_IR=0, rv=0, d_rv=None, old=None, soft_pad=0, pay_packed=False, off=0):
    """llr [n_tb][stride] -> (payload [n_tb][A], tb_ok, cb_ok [n_tb][C], syndrome, soft [n_tb][soft_floats]), every output from a
    guarded buffer; old [n_tb][soft_floats]: the soft buffer holds it and the call accumulates; soft_pad extra floats per
    transport block must stay as they were"""
    llr = np.ascontiguousarray(llr, np.float32)
    n_tb, stride = llr.shape
    qm, qp = tc.pairs(A, Z)
    geo = tb_ref.geometry(A, Z)
    sf, C = geo["soft_floats"], geo["C"]
    ss = sf + soft_pad
    fill = None
    if old is not None:
        fill = np.full((n_tb, ss), np.float32(7.5), np.float32)
        fill[:, :sf] = old
    g_soft = Guarded(om, n_tb * ss * 4, fill=fill)
    g_pay = Guarded(om, n_tb * (A // 8 if pay_packed else A), off)
    g_tb, g_cb, g_syn = Guarded(om, n_tb), Guarded(om, n_tb * C), Guarded(om, n_tb * 4)
    rx.tb_decode_frames(dev(om, llr), n_tb, stride, A, G, qp, g_soft.addr, ss, n_iter, qpp_minus=qm, Z=Z, q=q, N_IR=N_IR, rv=rv, d_rv=d_rv,
                        accumulate=old is not None, d_payload=g_pay.addr, payload_mode=om.BITS_PACKED if pay_packed else om.BITS_UNPACKED,
                        d_tb_ok=g_tb.addr, d_cb_ok=g_cb.addr, d_syndrome=g_syn.addr)
    soft = g_soft.read(np.float32).reshape(n_tb, ss)
    if soft_pad:
        pad = soft[:, sf:].view(np.uint32)
        assert np.all(pad == (np.float32(7.5).view(np.uint32) if old is not None else 0xA5A5A5A5)), "the gap between soft buffers was written"
    pay = g_pay.read().reshape(n_tb, -1)
    if pay_packed:
        pay = np.unpackbits(pay, axis=1, bitorder="big")
    return pay, g_tb.read(), g_cb.read().reshape(n_tb, C), g_syn.read(np.uint32), soft[:, :sf].copy()


def strong(cw):
    """noiseless LLRs of a codeword: +-4"""
    return (4.0 * (1.0 - 2.0 * np.asarray(cw, np.float64))).astype(np.float32)


def same_outputs(got, want):
    pay, tb_ok, cb_ok, syn, soft = got
    assert np.array_equal(pay, want[0]) and np.array_equal(tb_ok, want[1]) and np.array_equal(cb_ok, want[2])
    assert np.array_equal(syn, want[3]) and bits_equal(soft, want[4])


# ------------------------------------------------------------------------------------------ segment and desegment
SEG_CASES = ((80, 64), (72, 64), (88, 64), (48, 64), (496, 528), (976, 528))


@pytest.mark.parametrize("pay_packed,cw_packed", LAYOUTS, ids=("p1c1", "p1c8", "p8c1", "p8c8"))
@pytest.mark.parametrize("A,Z", SEG_CASES)
def test_segment_and_desegment_alone(om, tx0, rx0, A, Z, pay_packed, cw_packed):
    """G = sum (3 K_r + 12) at rv 0: a block sends all its coded bits (K-) or all but a few (K+), so every bit the segment
    kernel writes -- filler, payload, CRC24A, each CRC24B -- shapes the codeword, and from noiseless LLRs the reference brings
    every payload back (asserted here on the reference too), so the desegment kernel sees every kind of bit as well.
    3 transport blocks; the codeword's row ends 8 (packed) or 5 bits behind G."""
    check_pairs(om, A, Z)
    qm, qp = tc.pairs(A, Z)
    G = tc.full_g(A, Z)
    cw_bits = G + (8 + (-G) % 8 if cw_packed else 5)
    p = tc.payloads(A, 3)
    want = tb_ref.encode(p, G, qm, qp, Z=Z, cw_bits=cw_bits)
    got = gpu_encode(om, tx0, p, Z, G, cw_bits=cw_bits, pay_packed=pay_packed, cw_packed=cw_packed)
    assert np.array_equal(got, pack_msb(want) if cw_packed else want), "%d bytes differ" % int((got != (pack_msb(want) if cw_packed else want)).sum())
    llr = np.full((3, G + 7), np.nan, np.float32)
    llr[:, :G] = strong(want[:, :G])
    ref = tb_ref.decode(llr, A, G, qm, qp, 2, Z=Z)
    assert np.array_equal(ref[0], p) and ref[1].all()
    out = gpu_decode(om, rx0, llr, A, Z, G, 2, pay_packed=pay_packed, soft_pad=3)
    same_outputs(out, ref)
    assert np.array_equal(out[0], p) and out[1].all() and out[2].all() and not out[3].any()


@pytest.mark.parametrize("n_tb", (1, 65))
def test_batch_sizes_and_unaligned_buffers(om, tx0, rx0, n_tb):
    """1 and 65 transport blocks (3 is everywhere else); payload read at base + 1 .. 3 and written at base + 1 .. 3, one bit per
    byte: no whole-word access may be used"""
    A, Z = 88, 64
    qm, qp = check_pairs(om, A, Z)
    G = tc.full_g(A, Z)
    p = tc.payloads(A, n_tb, seed=n_tb)
    want = tb_ref.encode(p, G, qm, qp, Z=Z)
    for off in ((0,) if n_tb > 1 else (1, 2, 3)):
        assert np.array_equal(gpu_encode(om, tx0, p, Z, G, pay_off=off, off=off), want), off
        out = gpu_decode(om, rx0, strong(want), A, Z, G, 1, off=off)
        assert np.array_equal(out[0], p) and out[1].all() and out[2].all(), off
    ones = np.where(p[:1] != 0, 0xFF, 0xFE).astype(np.uint8)                   # only bit 0 of an unpacked payload byte is read
    assert np.array_equal(gpu_encode(om, tx0, ones, Z, G), want[:1])


def test_two_large_blocks_with_filler(om, tx0, rx0):
    """A = 6128 at Z = 6144: K- = 3072 and K+ = 3136, one block each, 8 filler bits; expectation of the receive side from the
    payload itself (every coded bit is sent and noiseless, so the decode returns the blocks)"""
    A, Z = 6128, 6144
    qm, qp = check_pairs(om, A, Z)
    G = 2 * (3 * 3136 + 12)                                  # E = Navail of the larger block: every coded bit of both is sent
    p = tc.payloads(A, 2)
    want = tb_ref.encode(p, G, qm, qp, Z=Z)
    assert np.array_equal(gpu_encode(om, tx0, p, Z, G, pay_packed=True, cw_packed=True), pack_msb(want))
    out = gpu_decode(om, rx0, strong(want), A, Z, G, 1, pay_packed=True)
    assert np.array_equal(out[0], p) and out[1].all() and out[2].all() and not out[3].any()


# ------------------------------------------------------------------------------------------ long CRC
@pytest.mark.parametrize("A", (40, 8 * 255, 8 * 256, 8 * 257, 8 * 512, 6120))
def test_crc24a_at_every_chunking_edge(om, tx0, rx0, A):
    """L = 0 at Z = 6144, so CRC24A is the only CRC: 5 bytes (fewer than the 256 runs), 255, 256 and 257 bytes (one byte per
    run, minus and plus one: the first length with runs of two and a shorter last run), 512 and the largest single block (runs
    of three).  Transport block 0 is clean; 1 .. 4 carry one flipped bit at 0, A - 1, A and B - 1 of the B-bit sequence."""
    Z = 6144
    qm, qp = check_pairs(om, A, Z)
    geo = tb_ref.segmentation(A, Z)
    assert geo["L"] == 0 and geo["C"] == 1
    G, F = tc.full_g(A, Z), geo["F"]
    p = tc.payloads(A, 5, seed=3)
    assert np.array_equal(gpu_encode(om, tx0, p, Z, G, pay_packed=True), tb_ref.encode(p, G, qm, qp, Z=Z))
    blocks = [tb_ref.segment(p[t], Z)[0] for t in range(5)]
    for t, pos in enumerate((0, A - 1, A, A + 23), start=1):
        blocks[t][0][F + pos] ^= 1
    llr = strong(tb_ref.encode_blocks(blocks, A, G, qm, qp, Z=Z))
    out = gpu_decode(om, rx0, llr, A, Z, G, 1)
    same_outputs(out, tb_ref.decode(llr, A, G, qm, qp, 1, Z=Z))
    want = [tb_ref.desegment(b, A, Z) for b in blocks]                         # and the decode returned the blocks as they were sent
    assert np.array_equal(out[0], np.stack([w[0] for w in want])) and list(out[1]) == [w[1] for w in want] == [1, 0, 0, 0, 0]
    assert out[2].all() and list(out[3]) == [w[3] for w in want]


def test_large_transport_block_and_the_right_cb_ok(om, tx0, rx0):
    """A = 100 000 at Z = 6144: 17 blocks of 5888 and 5952 bits, 48 filler bits -- CRC24A over 12 500 bytes in runs of 49, CRC24B
    per block in runs of 12.  Transport block 1 has one flipped payload bit inside block 5, transport block 2 at B - 1 (the last
    block): exactly that cb_ok and that tb_ok clear.  The reference's turbo decoder takes 12 s on these 51 blocks, so here -- and
    only here -- the expected bits are the reference's desegmentation of the blocks as sent (E = 3 K+ + 12 sends every coded bit,
    noiselessly; that the device's decoder equals the reference's is test_gpu_turbo.py's subject, up to K = 6144); the soft
    buffer is held to the reference's de-matching of the same LLRs."""
    A, Z = 100000, 6144
    qm, qp = check_pairs(om, A, Z)
    geo = tb_ref.segmentation(A, Z)
    assert (geo["C"], geo["K_minus"], geo["C_minus"], geo["K_plus"], geo["F"]) == (17, 5888, 11, 5952, 48)
    G = 17 * (3 * 5952 + 12)                                 # every coded bit of every block is sent: the noiseless decode returns the blocks
    p = tc.payloads(A, 3)
    blocks = [tb_ref.segment(p[t], Z)[0] for t in range(3)]
    clean = [[b.copy() for b in tb] for tb in blocks]
    blocks[1][5][1234] ^= 1
    blocks[2][16][geo["K_plus"] - 25] ^= 1
    cw = tb_ref.encode_blocks(clean + blocks, A, G, qm, qp, Z=Z, cw_bits=G + 4)     # one pass of the reference encoder for both uses
    assert G % 8 == 4 and np.array_equal(gpu_encode(om, tx0, p, Z, G, cw_bits=G + 4, pay_packed=True, cw_packed=True), pack_msb(cw[:3]))
    llr = strong(cw[3:, :G])
    out = gpu_decode(om, rx0, llr, A, Z, G, 1, pay_packed=True)
    g = tb_ref.geometry(A, Z, G)
    soft, at = [], 0
    for K, E, Ncb in zip(g["Ks"], g["Es"], g["Ncbs"]):
        soft.append(rm.dematch(llr[:, at:at + E], K, Ncb, 0))
        at += E
    assert bits_equal(out[4], np.concatenate(soft, axis=1))
    want = [tb_ref.desegment(b, A, Z) for b in blocks]
    assert np.array_equal(out[0], np.stack([w[0] for w in want])) and list(out[1]) == [1, 0, 0]
    assert np.array_equal(out[2], np.stack([w[2] for w in want])) and list(out[3]) == [w[3] for w in want]
    assert out[2].sum() == 3 * 17 - 2 and out[2][1, 5] == 0 and out[2][2, 16] == 0


# ------------------------------------------------------------------------------------------ rate matching
@pytest.mark.parametrize("q", (1, 2, 6))
def test_rate_matching_over_gamma_q_rv_and_nir(om, tx0, q):
    """A = 80 at Z = 64 is K = 56, 56, 64: gamma = 0 (one E; two groups by K), 1 (the E cut falls on the K cut: two groups) and
    2 = C - 1 (E cut at block 1, K cut at block 2: three groups); N_IR = 3 * 100 limits Ncb to 100 of Kw = 192 / 288; the packed
    codeword's row is longer than G"""
    A, Z = 80, 64
    qm, qp = check_pairs(om, A, Z)
    p = tc.payloads(A, 3, seed=q)
    for gamma in (0, 1, 2):
        G = (3 * 31 + gamma) * q
        for N_IR in (0, 300):
            geo = tb_ref.geometry(A, Z, G, q, N_IR)
            assert geo["gamma"] == gamma and len(geo["groups"]) == (2, 2, 3)[gamma] and (N_IR == 0 or geo["Ncbs"] == [100] * 3)
            for rv in range(4):
                cw_bits = G + 16 + (-G) % 8
                want = tb_ref.encode(p, G, qm, qp, Z=Z, q=q, N_IR=N_IR, rv=rv, cw_bits=cw_bits)
                assert np.array_equal(gpu_encode(om, tx0, p, Z, G, q=q, N_IR=N_IR, rv=rv, cw_bits=cw_bits, cw_packed=True), pack_msb(want)), (gamma, N_IR, rv)
                assert np.array_equal(gpu_encode(om, tx0, p, Z, G, q=q, N_IR=N_IR, rv=rv), want[:, :G]), (gamma, N_IR, rv)
    G = (3 * 70 + 2) * q                                     # at q = 6 E is above 3K + 12: the walk wraps
    rvs = np.array([2 | 0x7FFFFF00, 1 | -4, 3 + 8], np.int64).astype(np.int32)               # one rv per transport block, high bits ignored
    want = tb_ref.encode(p, G, qm, qp, Z=Z, q=q, rv=rvs & 3)
    assert np.array_equal(gpu_encode(om, tx0, p, Z, G, q=q, rv=99, d_rv=dev(om, rvs)), want)


# ------------------------------------------------------------------------------------------ receive side
@pytest.mark.parametrize("n_iter", (1, 2))
def test_receive_noisy_llrs_accumulate_and_per_tb_rv(om, rx0, n_iter):
    """5 transport blocks of A = 80 at Z = 64 in three groups, at a level where the reference passes some and fails some; then
    a second transmission accumulated onto the first call's buffer; then one rv per transport block"""
    A, Z, q = 80, 64, 2
    qm, qp = check_pairs(om, A, Z)
    G = (3 * 60 + 2) * q
    p = tc.payloads(A, 5, seed=8)
    rng = np.random.default_rng(34000 + n_iter)
    kw = dict(Z=Z, q=q)
    l0 = np.full((5, G + 9), np.nan, np.float32)
    l0[:, :G] = tr.awgn_llrs(tb_ref.encode(p, G, qm, qp, rv=0, **kw), -2.0, rng)
    l2 = tr.awgn_llrs(tb_ref.encode(p, G, qm, qp, rv=2, **kw), -2.0, rng)
    want1 = tb_ref.decode(l0, A, G, qm, qp, n_iter, rv=0, **kw)
    got1 = gpu_decode(om, rx0, l0, A, Z, G, n_iter, q=q, rv=0, soft_pad=5)
    same_outputs(got1, want1)
    want2 = tb_ref.decode(l2, A, G, qm, qp, n_iter, rv=2, soft=want1[4], **kw)
    same_outputs(gpu_decode(om, rx0, l2, A, Z, G, n_iter, q=q, rv=2, old=got1[4], soft_pad=5), want2)
    print("n_iter %d: tb_ok %s -> %s, cb_ok %d -> %d of 15" % (n_iter, want1[1], want2[1], want1[2].sum(), want2[2].sum()))
    assert want2[1].sum() >= want1[1].sum() and 0 < want1[2].sum() and want1[1].sum() < 5
    rvs = np.array([3 + 4, 1 - 8, 0, 2, 1], np.int32)
    lr = tr.awgn_llrs(tb_ref.encode(p, G, qm, qp, rv=rvs & 3, **kw), 0.0, rng)
    same_outputs(gpu_decode(om, rx0, lr, A, Z, G, n_iter, q=q, rv=-5, d_rv=dev(om, rvs)), tb_ref.decode(lr, A, G, qm, qp, n_iter, rv=rvs & 3, **kw))


def test_a_transport_block_alone_equals_itself_in_a_batch(om, rx0):
    A, Z = 88, 64
    G = 3 * 130 + 1
    llr = tc.noise((6, G), 5)
    alone = [gpu_decode(om, rx0, llr[i:i + 1], A, Z, G, 2) for i in range(6)]
    wide = np.full((6, G + 37), np.nan, np.float32)
    wide[:, :G] = llr
    b1 = gpu_decode(om, rx0, wide, A, Z, G, 2, soft_pad=11)
    b2 = gpu_decode(om, rx0, wide, A, Z, G, 2, soft_pad=11)                      # repeated call
    for x, y in zip(b1, b2):
        assert x.tobytes() == y.tobytes()
    for i in range(6):
        for x, y in zip(alone[i], b1):
            assert x[0].tobytes() == y[i].tobytes(), i


def test_outputs_are_optional(om, rx0):
    """each output alone equals itself among all; an `out` without any pointer only de-matches"""
    A, Z = 88, 64
    qm, qp = tc.pairs(A, Z)
    G = 3 * 130 + 1
    llr = tc.noise((3, G), 6)
    allout = gpu_decode(om, rx0, llr, A, Z, G, 1)
    sf = tb_ref.geometry(A, Z)["soft_floats"]
    d_llr = dev(om, llr)
    for name, i, nbytes, dt in (("d_payload", 0, 3 * A, np.uint8), ("d_tb_ok", 1, 3, np.uint8), ("d_cb_ok", 2, 9, np.uint8),
                                ("d_syndrome", 3, 12, np.uint32), (None, None, 0, None)):
        g_soft, g = Guarded(om, 3 * sf * 4), Guarded(om, nbytes if name else 4)
        rx0.tb_decode_frames(d_llr, 3, G, A, G, qp, g_soft.addr, sf, 1, qpp_minus=qm, Z=Z, **({name: g.addr} if name else {}))
        assert bits_equal(g_soft.read(np.float32).reshape(3, sf), allout[4])
        if name:
            assert np.array_equal(g.read(dt).ravel(), allout[i].ravel()), name
        else:
            assert g.untouched()


# ------------------------------------------------------------------------------------------ scale
def test_grid_of_twenty_thousand_transport_blocks(om, tx0, rx0):
    """20 000 transport blocks of A = 48 at Z = 64 (K = 56 and 64): as many workgroups of the segment and desegment kernels"""
    A, Z, n_src, n_tb = 48, 64, 16, 20000
    qm, qp = check_pairs(om, A, Z)
    G = 2 * 151 + 1
    src = tc.payloads(A, n_src, seed=20)
    pick = np.arange(n_tb) % n_src
    want = tb_ref.encode(src, G, qm, qp, Z=Z, rv=1, cw_bits=G + 3)
    got = gpu_encode(om, tx0, src[pick], Z, G, rv=1, cw_bits=G + 3, pay_packed=True, cw_packed=False)
    assert np.array_equal(got, want[pick])
    l = tr.awgn_llrs(want[:, :G], -1.0, np.random.default_rng(35000))
    out = gpu_decode(om, rx0, l[pick], A, Z, G, 1, rv=1, pay_packed=True)
    ref = tb_ref.decode(l, A, G, qm, qp, 1, Z=Z, rv=1)
    same_outputs(out, tuple(x[pick] for x in ref))


# ------------------------------------------------------------------------------------------ the HARQ chain
def test_harq_chain_first_round_fails_second_round_decodes(om, torch):
    """payload -> tb_encode rv 0 (CRC24A, two blocks of K = 528 with 8 filler bits, CRC24B each, E = 500 per block) -> scramble
    -> modulate (64-pt QPSK) -> channel + AWGN -> demod_frames_soft -> descramble -> tb_decode; then the rv 2 retransmission
    through a second channel realisation, accumulated into the same soft buffer.  At both rounds tb_ok, cb_ok, the payload and
    the soft buffer are the reference's on the GPU's own LLRs; every transport block fails the first round (E < K + 4) and
    passes the second, the condition tests/test_tb_ref_host.py asserts on the reference alone.  One transport block per frame
    over a flat channel; noise_var = N ps / (2 Kd 10^(esn0 / 10)) as derived in tests/test_gpu_turbo_rm.py's chain."""
    A, Z, G, q, esn0, n = tc.HARQ_A, tc.HARQ_Z, tc.HARQ_G, tc.HARQ_Q, tc.HARQ_ESN0_DB, tc.HARQ_TBS
    qm, qp = check_pairs(om, A, Z)
    N, cp, Kd, n_sym = 64, 16, 40, 20
    L = N + cp
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), "QPSK")
    rxe = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 100, 0.7)
    rxe.set_max_trials(0)
    seg_bits = txe.bits_per_frame(n_sym)
    assert seg_bits >= G
    sf = tb_ref.geometry(A, Z)["soft_floats"]
    payload = tc.harq_rounds()[0]
    d_pay = dev(om, payload)
    d_cinit = dev(om, np.arange(n, dtype=np.uint32) * 2654435761 % (1 << 31))
    d_cw = om.DeviceBuffer(n * seg_bits)
    fl_tx, fl = n_sym * L, n_sym * L + cp
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = np.zeros(cp + 1, np.complex64)
    taps[0] = 1.0
    d_taps = dev(om, taps)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds * Kd * 2 == seg_bits
    d_eq, d_llr = om.DeviceBuffer(n * nds * Kd * 8), om.DeviceBuffer(n * seg_bits * 4)
    g_soft = Guarded(om, n * sf * 4)
    nv, old, oks = None, None, []
    for rnd, rv in enumerate((0, 2)):
        txe.tb_encode_frames(d_pay, n, A, G, qp, d_cw, seg_bits, qpp_minus=qm, Z=Z, q=q, rv=rv)
        cw = d_cw.download(np.uint8, n * seg_bits).reshape(n, seg_bits)
        assert np.array_equal(cw, tb_ref.encode(payload, G, qm, qp, Z=Z, q=q, rv=rv, cw_bits=seg_bits))
        txe.scramble_frames(d_cw, n, seg_bits, d_cinit, d_cw)
        txe.modulate_frames(d_cw, n, n_sym, d_tx)
        if nv is None:
            pw = (np.abs(d_tx.download(np.complex64, n * fl_tx).reshape(n, n_sym, L)) ** 2).mean(axis=(0, 2))
            ps = float(pw[np.arange(n_sym) % 4 != 0].mean())                    # the data symbols of the (1, 3) pattern
            nv = N * ps / (2.0 * Kd * 10.0 ** (esn0 / 10.0))
            print("HARQ chain: data ps = %.4g, noise_var = %.4g" % (ps, nv))
        txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx, fl, fl, noise_var=nv, seed=41 + rnd)
        assert rxe.demod_frames_soft(d_rx, n, fl, fl, d_eq, d_llr=d_llr) == nds
        rxe.descramble_llr_frames(d_llr, n, seg_bits, seg_bits, d_cinit, d_llr)
        llr = d_llr.download(np.float32, n * seg_bits).reshape(n, seg_bits)
        ber = ((llr[:, :G] < 0) != (cw[:, :G] != 0)).mean()
        g_pay, g_tb, g_cb, g_syn = Guarded(om, n * A), Guarded(om, n), Guarded(om, n * 2), Guarded(om, n * 4)
        rxe.tb_decode_frames(d_llr, n, seg_bits, A, G, qp, g_soft.addr, sf, tc.HARQ_ITERS, qpp_minus=qm, Z=Z, q=q, rv=rv, accumulate=rnd > 0,
                             d_payload=g_pay.addr, d_tb_ok=g_tb.addr, d_cb_ok=g_cb.addr, d_syndrome=g_syn.addr)
        want = tb_ref.decode(llr, A, G, qm, qp, tc.HARQ_ITERS, Z=Z, q=q, rv=rv, soft=old)
        got = (g_pay.read().reshape(n, A), g_tb.read(), g_cb.read().reshape(n, 2), g_syn.read(np.uint32), g_soft.read(np.float32).reshape(n, sf))
        same_outputs(got, want)
        old = want[4]
        oks.append(got[1])
        print("HARQ chain rv %d: raw BER %.4f, tb_ok %d of %d, cb_ok %d of %d" % (rv, float(ber), got[1].sum(), n, got[2].sum(), 2 * n))
    assert not oks[0].any() and oks[1].all() and np.array_equal(got[0], payload)


# ------------------------------------------------------------------------------------------ capture, errors
def test_both_calls_are_capturable_after_reserve(om, torch):
    """three groups on both sides; the decode replays de-match x 3, decode x 2 and the desegment kernel.  Handles of its own:
    their workspaces hold exactly what reserve_tb asked for, so a larger batch inside the capture has to be refused"""
    tx0, rx0 = om.TxEngine(64, 16, 62, 60), om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    A, Z, q, n_tb, rv = 80, 64, 1, 4, 1
    qm, qp = tc.pairs(A, Z)
    G = 3 * 120 + 2
    sf = tb_ref.geometry(A, Z)["soft_floats"]
    p = tc.payloads(A, n_tb, seed=12)
    want_cw = tb_ref.encode(p, G, qm, qp, Z=Z, rv=rv)
    l = tr.awgn_llrs(want_cw, 0.0, np.random.default_rng(36000))
    old = tc.noise((n_tb, sf), 13)
    want = tb_ref.decode(l, A, G, qm, qp, 2, Z=Z, rv=rv, soft=old)
    tx0.reserve_tb(n_tb, A, G, Z=Z)
    rx0.reserve_tb(n_tb, A, Z=Z)
    d_p, d_l = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(l.copy()).cuda()
    cw = torch.zeros(n_tb * G, dtype=torch.uint8, device="cuda")
    soft = torch.from_numpy(old.copy()).cuda()
    pay = torch.zeros(n_tb * A, dtype=torch.uint8, device="cuda")
    tb_ok = torch.full((n_tb,), 9, dtype=torch.uint8, device="cuda")
    cb_ok = torch.full((n_tb * 3,), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def call(stream):
        tx0.tb_encode_frames(d_p, n_tb, A, G, qp, cw, G, qpp_minus=qm, Z=Z, rv=rv, stream=stream)
        rx0.tb_decode_frames(d_l, n_tb, G, A, G, qp, soft, sf, 2, qpp_minus=qm, Z=Z, rv=rv, accumulate=True, d_payload=pay, d_tb_ok=tb_ok,
                             d_cb_ok=cb_ok, stream=stream)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="reserve_tb"):  # a batch the reserved workspace does not hold cannot grow it here
            tx0.tb_encode_frames(d_p, 4 * n_tb, A, G, qp, cw, G, qpp_minus=qm, Z=Z, stream=torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="reserve_tb"):
            rx0.tb_decode_frames(d_l, 4 * n_tb, G, A, G, qp, soft, sf, 2, qpp_minus=qm, Z=Z, d_tb_ok=tb_ok,
                                 stream=torch.cuda.current_stream().cuda_stream)
    assert not cw.any() and bits_equal(soft.cpu().numpy(), old)                # capture enqueues nothing
    for _ in range(2):
        cw.zero_()
        pay.zero_()
        soft.copy_(torch.from_numpy(old))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cw.cpu().numpy().reshape(n_tb, G), want_cw)
        assert bits_equal(soft.cpu().numpy(), want[4]) and np.array_equal(pay.cpu().numpy().reshape(n_tb, A), want[0])
        assert np.array_equal(tb_ok.cpu().numpy(), want[1]) and np.array_equal(cb_ok.cpu().numpy().reshape(n_tb, 3), want[2])


def test_argument_errors_leave_poisoned_outputs_untouched(om, rx0, tx0):
    A, Z, n_tb = 80, 64, 3
    qm, qp = tc.pairs(A, Z)
    G = 3 * 120 + 2
    sf = tb_ref.geometry(A, Z)["soft_floats"]
    U, P = om.BITS_UNPACKED, om.BITS_PACKED
    d_p = dev(om, tc.payloads(A, n_tb))
    g_cw = Guarded(om, n_tb * (G + 6))
    base = dict(n_tb=n_tb, A=A, G=G, qp=qp, qm=qm, Z=Z, q=1, N_IR=0, rv=0, cw_bits=G + 5, payload_mode=U, cw_mode=U)
    for kw in (dict(A=84), dict(A=0), dict(Z=60), dict(Z=520), dict(G=0), dict(G=2), dict(G=-G), dict(q=0), dict(q=7), dict(N_IR=-1),
               dict(N_IR=3 * 96 - 1), dict(G=16 * 3 * 180 + 3, cw_bits=10 ** 4), dict(qp=(2, 16)), dict(qp=(7, 64)), dict(qm=(2, 42)),
               dict(rv=4), dict(rv=-1), dict(cw_bits=G - 1), dict(cw_mode=P), dict(cw_mode=7), dict(payload_mode=om.BITS_NONE),
               dict(n_tb=-1), dict(n_tb=2 ** 31), dict(n_tb=2 ** 30, cw_bits=2 ** 12)):
        a = dict(base)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.tb_encode_frames(d_p, a["n_tb"], a["A"], a["G"], a["qp"], g_cw.addr, a["cw_bits"], qpp_minus=a["qm"], Z=a["Z"], q=a["q"],
                                 N_IR=a["N_IR"], rv=a["rv"], payload_mode=a["payload_mode"], cw_mode=a["cw_mode"])
    with pytest.raises(ValueError):
        tx0.tb_encode_frames(None, n_tb, A, G, qp, g_cw.addr, G + 6, qpp_minus=qm, Z=Z)
    tx0.tb_encode_frames(d_p, 0, A, G, qp, g_cw.addr, G + 6, qpp_minus=qm, Z=Z)                # no-op
    assert g_cw.untouched()
    g_72 = Guarded(om, n_tb * 300)                                                             # C- = 0: the K- pair is not looked at
    tx0.tb_encode_frames(d_p, n_tb, 72, 3 * 100, tc.qpp_for(56), g_72.addr, 300, qpp_minus=(99, 99), Z=Z)
    p72 = tc.payloads(A, n_tb).ravel()[:n_tb * 72].reshape(n_tb, 72)
    # d_p read as dense [n_tb][72]: the first 216 bytes of the payloads above
    assert np.array_equal(g_72.read().reshape(n_tb, 300), tb_ref.encode(p72, 300, (0, 0), tc.qpp_for(56), Z=Z))
    for bad in (dict(A=84), dict(G=0)):
        with pytest.raises(ValueError):
            tx0.reserve_tb(1, bad.get("A", A), bad.get("G", G), Z=Z)
    with pytest.raises(ValueError):
        rx0.reserve_tb(-1, A, Z=Z)
    with pytest.raises(ValueError):
        rx0.reserve_tb(1, A, Z=60)

    d_llr = dev(om, np.ones((n_tb, G + 4), np.float32))
    g_soft, g_pay, g_tb = Guarded(om, n_tb * sf * 4), Guarded(om, n_tb * A), Guarded(om, n_tb)
    base = dict(n_tb=n_tb, stride=G + 4, A=A, G=G, qp=qp, qm=qm, Z=Z, q=1, N_IR=0, rv=0, n_iter=2, soft_stride=sf, payload_mode=U)
    for kw in (dict(A=84), dict(Z=60), dict(G=0), dict(G=2), dict(q=7), dict(N_IR=3 * 96 - 1), dict(qp=(2, 16)), dict(qm=(2, 42)), dict(rv=4),
               dict(rv=-1), dict(n_iter=0), dict(n_iter=17), dict(stride=G - 1), dict(soft_stride=sf - 1), dict(payload_mode=7),
               dict(n_tb=-1), dict(n_tb=2 ** 31), dict(n_tb=2 ** 30, stride=2 ** 12), dict(stride=2 ** 41)):
        a = dict(base)
        a.update(kw)
        with pytest.raises(ValueError):
            rx0.tb_decode_frames(d_llr, a["n_tb"], a["stride"], a["A"], a["G"], a["qp"], g_soft.addr, a["soft_stride"], a["n_iter"],
                                 qpp_minus=a["qm"], Z=a["Z"], q=a["q"], N_IR=a["N_IR"], rv=a["rv"], d_payload=g_pay.addr,
                                 payload_mode=a["payload_mode"], d_tb_ok=g_tb.addr)
    with pytest.raises(ValueError):
        rx0.tb_decode_frames(None, n_tb, G + 4, A, G, qp, g_soft.addr, sf, 2, qpp_minus=qm, Z=Z, d_tb_ok=g_tb.addr)
    with pytest.raises(ValueError):
        rx0.tb_decode_frames(d_llr, n_tb, G + 4, A, G, qp, None, sf, 2, qpp_minus=qm, Z=Z, d_tb_ok=g_tb.addr)
    rx0.tb_decode_frames(d_llr, 0, G + 4, A, G, qp, g_soft.addr, sf, 2, qpp_minus=qm, Z=Z, d_tb_ok=g_tb.addr)     # no-op
    assert g_soft.untouched() and g_pay.untouched() and g_tb.untouched()
