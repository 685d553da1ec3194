"""The turbo rate-matching kernels of csrc/turbo_rm.hip on the GPU (-m gpu): ofdm_tx_turbo_encode_rm_frames and
ofdm_turbo_rate_dematch_frames against tests/turbo_rm_ref.py (the contract written literally).  Every comparison is array_equal
-- bits, and float32 values by their bit pattern -- and every output sits between poisoned guard bands.  The HARQ chain runs at
the operating point tests/test_turbo_rm_ref_host.py asserts on the reference alone."""
import numpy as np
import pytest

import turbo_cases as tc
import turbo_ref as tr
import turbo_rm_cases as rc
import turbo_rm_ref as rm

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]       # (info packed, coded packed)


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
    """any receiver handle serves the de-matcher (it reads LLR buffers, not the handle's numerology)"""
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
    """float32 arrays equal by bit pattern (so that -0 != +0 and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gpu_encode(om, tx, info, f1, f2, E, Ncb, rv, seg_bits, info_packed=False, coded_packed=False, off=0, d_rv=None):
    """info [n_seg][bps][K] -> the coded buffer's bytes [n_seg][seg_bytes], written at allocation + 64 + off"""
    n_seg, bps, K = info.shape
    src = pack_msb(info) if info_packed else info
    seg_bytes = seg_bits // 8 if coded_packed else seg_bits
    g = Guarded(om, n_seg * seg_bytes, off)
    tx.turbo_encode_rm_frames(dev(om, src), n_seg, bps, K, f1, f2, E, g.addr, seg_bits, Ncb=Ncb, rv=rv, d_rv=d_rv,
                              info_mode=om.BITS_PACKED if info_packed else om.BITS_UNPACKED,
                              coded_mode=om.BITS_PACKED if coded_packed else om.BITS_UNPACKED)
    return g.read().reshape(n_seg, seg_bytes)


def gpu_dematch(om, rx, llr_seg, bps, K, E, Ncb, rv, old=None, out_pad=0, d_rv=None):
    """llr_seg [n_seg][stride] -> [n_seg][bps][3K + 12] from a guarded buffer (poisoned, or holding `old` [n_seg][bps][3K + 12]:
    then the call accumulates); out_pad extra floats per segment must stay as they were"""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    per = bps * (3 * K + 12)
    out_stride = per + out_pad
    fill = None
    if old is not None:
        fill = np.full((n_seg, out_stride), np.float32(7.5), np.float32)
        fill[:, :per] = np.asarray(old, np.float32).reshape(n_seg, per)
    g = Guarded(om, n_seg * out_stride * 4, fill=fill)
    rx.turbo_rate_dematch_frames(dev(om, llr_seg), n_seg, stride, bps, K, E, g.addr, out_stride, Ncb=Ncb, rv=rv, d_rv=d_rv,
                                 accumulate=old is not None)
    got = g.read(np.float32).reshape(n_seg, out_stride)
    if out_pad:
        pad = got[:, per:].view(np.uint32)
        assert np.all(pad == (np.float32(7.5).view(np.uint32) if old is not None else 0xA5A5A5A5)), "the gap between segments was written"
    return got[:, :per].reshape(n_seg, bps, 3 * K + 12)


# ------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("info_packed,coded_packed", LAYOUTS, ids=("i1c1", "i1c8", "i8c1", "i8c8"))
@pytest.mark.parametrize("K", rc.SMALL_KS)
def test_encoder_equals_reference_over_e_rv_ncb(om, tx0, K, info_packed, coded_packed):
    """2 segments x 3 blocks: with an odd E the second and third packed block start inside a byte; the filler is written"""
    f1, f2 = tc.QPP[K]
    info = rc.info_bits(K, 2, 3)
    for E in rc.enc_es(K):
        seg_bits = 3 * E + 8 + (-(3 * E)) % 8 if coded_packed else 3 * E + 5
        for Ncb in rc.ncbs(K):
            for rv in rc.RVS:
                want = rm.encode_rm_segments(info, f1, f2, E, Ncb, rv, seg_bits)
                got = gpu_encode(om, tx0, info, f1, f2, E, Ncb, rv, seg_bits, info_packed, coded_packed)
                if coded_packed:
                    want = pack_msb(want)
                assert np.array_equal(got, want), "E=%d Ncb=%d rv=%d: %d bytes differ" % (E, Ncb, rv, int((got != want).sum()))


@pytest.mark.parametrize("bps", (1, 9))
@pytest.mark.parametrize("K", (40, 64))
def test_encoder_block_counts_and_small_e(om, tx0, K, bps):
    """1 and 9 blocks per segment (9: a full group of 8 and a group of 1 for odd E), E from 1 (a byte spans 8 blocks) upwards"""
    f1, f2 = tc.QPP[K]
    info = rc.info_bits(K, 2, bps, seed=bps)
    for E, Ncb, rv in ((1, 0, 0), (3, 0, 1), (7, 0, 2), (12, 0, 3), (K + 1, 0, 2), (2 * K + 3, rc.ncbs(K)[1], 3), (3 * K + 12, 0, 1),
                       (3 * K + 14, 0, 0)):
        for coded_packed in (False, True):
            seg_bits = bps * E + (16 + (-(bps * E)) % 8 if coded_packed else 3)
            want = rm.encode_rm_segments(info, f1, f2, E, Ncb, rv, seg_bits)
            got = gpu_encode(om, tx0, info, f1, f2, E, Ncb, rv, seg_bits, True, coded_packed)
            assert np.array_equal(got, pack_msb(want) if coded_packed else want), (E, Ncb, rv, coded_packed)


def test_encoder_largest_block(om, tx0):
    K = rc.BIG_K
    f1, f2 = tc.QPP[K]
    info = rc.info_bits(K, 1, 3)
    for E, Ncb, rv, packed in ((2 * K + 3, 0, 3, True), (3 * K + 12, 2 * rm.dims(K)[2] + 1, 2, False)):
        seg_bits = 3 * E + (16 + (-(3 * E)) % 8 if packed else 7)
        want = rm.encode_rm_segments(info, f1, f2, E, Ncb, rv, seg_bits)
        got = gpu_encode(om, tx0, info, f1, f2, E, Ncb, rv, seg_bits, True, packed)
        assert np.array_equal(got, pack_msb(want) if packed else want), (E, Ncb, rv)


def test_encoder_filler_only_unaligned_output_per_segment_rv_and_bit0(om, tx0):
    K = 48
    f1, f2 = tc.QPP[K]
    E = 2 * K + 3
    for packed in (False, True):                             # no block at all: the segment is filler
        got = gpu_encode(om, tx0, np.zeros((3, 0, K), np.uint8), f1, f2, E, 0, 0, 104, False, packed)
        assert got.shape == (3, 13 if packed else 104) and not got.any()
    info = rc.info_bits(K, 3, 2, seed=5)
    seg_bits = 2 * E + 5
    want = rm.encode_rm_segments(info, f1, f2, E, 0, 1, seg_bits)
    for off in (1, 2, 3):                                    # one bit per byte at base + 1 .. 3: no whole-word store may be used
        assert np.array_equal(gpu_encode(om, tx0, info, f1, f2, E, 0, 1, seg_bits, True, False, off=off), want), off
    rvs = np.array([2 | 0x7FFFFF00, 1 | -4, 3 + 8], np.int64).astype(np.int32)               # high bits set: ignored
    want = rm.encode_rm_segments(info, f1, f2, E, 0, rvs & 3, seg_bits)
    assert len({w.tobytes() for w in want}) == 3
    got = gpu_encode(om, tx0, info, f1, f2, E, 0, 99, seg_bits, d_rv=dev(om, rvs))           # the scalar is not used, nor checked
    assert np.array_equal(got, want)
    ones = np.full((1, 3, K), 0xFF, np.uint8)                # only bit 0 of an unpacked information byte is read
    assert np.array_equal(gpu_encode(om, tx0, ones, f1, f2, E, 0, 0, 3 * E), rm.encode_rm_segments(ones & 1, f1, f2, E, 0, 0, 3 * E))


# ------------------------------------------------------------------------------------------ de-matching
@pytest.mark.parametrize("K", rc.SMALL_KS)
def test_dematch_equals_reference_over_e_rv_ncb(om, rx0, K):
    """the six rows of edge_rows -- noise, NaN / +-inf, +-3e38 sums that overflow or cancel by order, signed zeros and subnormals,
    -0.0, all NaN -- as 2 segments x 3 blocks"""
    for Ncb in rc.ncbs(K):
        navail = rm.n_avail(K, Ncb)
        for E in rc.enc_es(K) + ((3 * navail + 1, 16 * navail) if K == 40 else (2 * navail + 5,)):
            if E > 16 * navail:
                continue
            l = rc.edge_rows(E, K).reshape(2, 3 * E)
            seg = np.full((2, 3 * E + 9), np.nan, np.float32)
            seg[:, :3 * E] = l
            for rv in rc.RVS:
                want = rm.dematch_segments(seg, 3, K, E, Ncb, rv)
                got = gpu_dematch(om, rx0, seg, 3, K, E, Ncb, rv, out_pad=3)
                assert bits_equal(got, want), (E, Ncb, rv)


def test_dematch_keeps_negative_zero_and_wraps_past_ncb_at_rv3(om, rx0):
    K = 40
    Kpi = rm.dims(K)[2]
    Ncb = 2 * Kpi + 1
    navail = rm.n_avail(K, Ncb)
    E = navail + 7                                           # rv 3 starts at 3/4 of the buffer: the walk wraps, 7 bits twice
    l = np.full((1, E), -0.0, np.float32)
    got = gpu_dematch(om, rx0, l, 1, K, E, Ncb, 3)
    want = rm.dematch_segments(l, 1, K, E, Ncb, 3)
    assert bits_equal(got, want)
    sent = np.zeros(3 * K + 12, bool)
    sent[rm.selection(K, E, Ncb, 3)] = True
    assert sent.sum() == navail < 3 * K + 12
    assert np.all(np.signbit(got[0, 0, sent])) and not np.any(np.signbit(got[0, 0, ~sent]))
    awgn = rc.awgn_rows(1, E, 3)
    assert bits_equal(gpu_dematch(om, rx0, awgn, 1, K, E, Ncb, 3), rm.dematch_segments(awgn, 1, K, E, Ncb, 3))


@pytest.mark.parametrize("K", (40, 64))
def test_dematch_accumulates_onto_noise_nan_and_an_earlier_call(om, rx0, K):
    E, n_seg, bps = 2 * K + 3, 2, 3
    per = 3 * K + 12
    l0, l2 = rc.awgn_rows(n_seg, bps * E, K), rc.awgn_rows(n_seg, bps * E, K + 1)
    old = rc.awgn_rows(n_seg, bps * per, K + 2).reshape(n_seg, bps, per).copy()
    old[0, 1, ::5] = np.nan
    old[1, 0, ::7] = np.inf
    old[1, 2, 3::4] = -0.0
    got = gpu_dematch(om, rx0, l0, bps, K, E, 0, 1, old=old, out_pad=5)
    assert bits_equal(got, rm.dematch_segments(l0, bps, K, E, 0, 1, old=old))
    first = gpu_dematch(om, rx0, l0, bps, K, E, 0, 0)                            # rv 0, then rv 2 onto the result of that call
    both = gpu_dematch(om, rx0, l2, bps, K, E, 0, 2, old=first)
    want1 = rm.dematch_segments(l0, bps, K, E, 0, 0)
    assert bits_equal(first, want1) and bits_equal(both, rm.dematch_segments(l2, bps, K, E, 0, 2, old=want1))
    rvs = np.array([3 + 4, 1 - 8], np.int32)                                    # one rv per segment, high bits ignored
    got = gpu_dematch(om, rx0, l0, bps, K, E, 0, -5, old=old, d_rv=dev(om, rvs))
    assert bits_equal(got, rm.dematch_segments(l0, bps, K, E, 0, rvs & 3, old=old))


def test_dematch_largest_block(om, rx0):
    K = rc.BIG_K
    E = 4 * K + 1
    l = rc.awgn_rows(1, 2 * E, 17)
    for Ncb, rv in ((0, 3), (2 * rm.dims(K)[2] + 1, 1)):
        assert bits_equal(gpu_dematch(om, rx0, l, 2, K, E, Ncb, rv), rm.dematch_segments(l, 2, K, E, Ncb, rv)), (Ncb, rv)


def test_a_block_alone_in_a_batch_at_a_larger_stride_and_on_a_repeated_call(om, rx0):
    K, E, n = 56, 2 * 56 + 3, 12
    l = rc.awgn_rows(n, E, 56)
    alone = [gpu_dematch(om, rx0, l[i:i + 1], 1, K, E, 0, 2) for i in range(n)]
    one = gpu_dematch(om, rx0, l.reshape(1, n * E), n, K, E, 0, 2)               # one segment of 12 blocks
    wide = np.full((4, 3 * E + 37), np.nan, np.float32)                          # 4 segments of 3, poisoned gaps
    wide[:, :3 * E] = l.reshape(4, 3 * E)
    w1 = gpu_dematch(om, rx0, wide, 3, K, E, 0, 2, out_pad=11)
    w2 = gpu_dematch(om, rx0, wide, 3, K, E, 0, 2, out_pad=11)                   # repeated call
    assert one.tobytes() == w1.tobytes() == w2.tobytes()
    for i in range(n):
        assert alone[i].tobytes() == one[0, i].tobytes(), i
    assert bits_equal(one[0], rm.dematch(l, K, 0, 2))


def test_grid_of_forty_thousand_blocks(om, tx0, rx0):
    """40 000 blocks of K = 40: 5 000 encoder groups of 8 (odd E, packed) and 20 625 de-matching workgroups"""
    K, E, n_src, n_seg, bps = 40, 101, 16, 4000, 10
    f1, f2 = tc.QPP[K]
    src_info = rc.info_bits(K, 1, n_src, seed=7)[0]
    src_l = rc.awgn_rows(n_src, E, 77)
    pick = np.arange(n_seg * bps) % n_src
    seg_bits = bps * E + 6
    want_src = rm.rate_match(tr.encode(src_info, f1, f2), E, 0, 1)
    want = np.zeros((n_seg, seg_bits), np.uint8)
    want[:, :bps * E] = want_src[pick].reshape(n_seg, bps * E)
    got = gpu_encode(om, tx0, src_info[pick].reshape(n_seg, bps, K), f1, f2, E, 0, 1, seg_bits, True, True)
    assert np.array_equal(got, pack_msb(want))
    seg = np.full((n_seg, bps * E + 3), np.nan, np.float32)
    seg[:, :bps * E] = src_l[pick].reshape(n_seg, bps * E)
    out = gpu_dematch(om, rx0, seg, bps, K, E, 0, 1)
    assert bits_equal(out.reshape(-1, 3 * K + 12), rm.dematch(src_l, K, 0, 1)[pick])


# ------------------------------------------------------------------------------------------ the HARQ chain
def test_harq_chain_first_round_fails_second_round_decodes(om, torch):
    """payload + gCRC24A -> encode-rm rv 0 -> scramble -> modulate (64-pt QPSK) -> channel + AWGN -> demod_frames_soft ->
    descramble -> de-match -> turbo decode -> crc_check; then the rv 2 retransmission through a second channel realisation,
    de-matched with accumulate into the same buffer, decoded and checked again.  At both stages the decoded bits are the
    reference's on the GPU's own LLRs; the first stage has failing CRCs, the second none.  One block per frame over a flat
    channel, so that the copies of a bit cannot land on one subcarrier's fade together.  The noise variance
    follows from the operating point's Es/N0: a QPSK symbol carries two bits, so the per-bit Es/N0 of the host test's BPSK
    model needs a symbol Es/N0 of twice that; a data bin holds N ps / Kd of the time-domain power ps per sample against N0 =
    noise_var per bin, hence noise_var = N ps / (2 Kd 10^(esn0 / 10)).  tests/turbo_rm_cases.py says why the chain's point has
    E < K + 4 and what room its Es/N0 leaves for the receiver's channel estimate."""
    K, E, esn0 = rc.HARQ_POINTS[0]
    f1, f2 = tc.QPP[K]
    N, cp, Kd, n_sym, n = 64, 16, 40, 12, rc.HARQ_BLOCKS
    A, L, per = K - 24, N + cp, 3 * K + 12
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), "QPSK")
    rxe = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 100, 0.7)
    rxe.set_max_trials(0)
    seg_bits = txe.bits_per_frame(n_sym)
    assert om.turbo_rm_blocks(seg_bits, K, E) >= 1
    nv = None
    rng = np.random.default_rng(K)
    payload = rng.integers(0, 2, (n, A)).astype(np.uint8)
    d_cinit = dev(om, np.arange(n, dtype=np.uint32) * 2654435761 % (1 << 31))
    d_info, d_coded = om.DeviceBuffer(n * K), om.DeviceBuffer(n * seg_bits)
    txe.crc_attach_frames(dev(om, payload), n, A, om.CRC24A, d_info)
    info = d_info.download(np.uint8, n * K).reshape(n, 1, K)
    fl_tx, fl = n_sym * L, n_sym * L + cp
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = np.zeros(cp + 1, np.complex64)
    taps[0] = 1.0
    d_taps = dev(om, taps)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds * Kd * 2 == seg_bits
    d_eq, d_llr = om.DeviceBuffer(n * nds * Kd * 8), om.DeviceBuffer(n * seg_bits * 4)
    g_soft = Guarded(om, n * per * 4)
    old, wrong = None, []
    for rnd, rv in enumerate((0, 2)):
        txe.turbo_encode_rm_frames(d_info, n, 1, K, f1, f2, E, d_coded, seg_bits, rv=rv)
        coded = d_coded.download(np.uint8, n * seg_bits).reshape(n, seg_bits)
        assert np.array_equal(coded, rm.encode_rm_segments(info, f1, f2, E, 0, rv, seg_bits))
        txe.scramble_frames(d_coded, n, seg_bits, d_cinit, d_coded)
        txe.modulate_frames(d_coded, n, n_sym, d_tx)
        if nv is None:
            pw = (np.abs(d_tx.download(np.complex64, n * fl_tx).reshape(n, n_sym, L)) ** 2).mean(axis=(0, 2))
            ps = float(pw[np.arange(n_sym) % 4 != 0].mean())                    # the data symbols of the (1, 3) pattern
            nv = N * ps / (2.0 * Kd * 10.0 ** (esn0 / 10.0))
            print("HARQ chain: power per symbol %s, data ps = %.4g, noise_var = %.4g" % (np.round(pw, 4), ps, nv))
        txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx, fl, fl, noise_var=nv, seed=21 + rnd)
        assert rxe.demod_frames_soft(d_rx, n, fl, fl, d_eq, d_llr=d_llr) == nds
        rxe.descramble_llr_frames(d_llr, n, seg_bits, seg_bits, d_cinit, d_llr)
        llr = d_llr.download(np.float32, n * seg_bits).reshape(n, seg_bits)
        ber = ((llr[:, :E] < 0) != (coded[:, :E] != 0)).mean(axis=1)
        print("HARQ chain rv %d: raw BER %.4f, per frame %s" % (rv, float(ber.mean()), np.round(ber, 3)))
        rxe.turbo_rate_dematch_frames(d_llr, n, seg_bits, 1, K, E, g_soft.addr, per, rv=rv, accumulate=rnd > 0)
        soft = g_soft.read(np.float32).reshape(n, 1, per)
        want_soft = rm.dematch_segments(llr, 1, K, E, 0, rv, old=old)
        assert bits_equal(soft, want_soft)
        old = want_soft
        g_bits, g_ok = Guarded(om, n * K), Guarded(om, n)
        rxe.turbo_decode_frames(g_soft.addr, n, per, 1, K, f1, f2, rc.HARQ_ITERS, d_bits=g_bits.addr)
        rxe.crc_check_frames(g_bits.addr, n, A, om.CRC24A, d_ok=g_ok.addr)
        bits, ok = g_bits.read().reshape(n, K), g_ok.read()
        rbits, _ = tr.decode(want_soft[:, 0], f1, f2, rc.HARQ_ITERS)
        assert np.array_equal(bits, rbits)
        bad = np.any(rbits != info[:, 0], axis=1)
        assert np.array_equal(ok == 0, bad)
        wrong.append(int(bad.sum()))
    print("HARQ chain K=%d E=%d Es/N0=%+g dB: %d -> %d of %d CRCs fail" % (K, E, esn0, wrong[0], wrong[1], n))
    assert wrong[0] > 0 and wrong[1] == 0


# ------------------------------------------------------------------------------------------ capture, errors
def test_both_calls_are_capturable_after_reserve(om, torch, tx0, rx0):
    K, E, n_seg, bps, rv = 64, 2 * 64 + 3, 3, 5, 2
    f1, f2 = tc.QPP[K]
    per = 3 * K + 12
    info = rc.info_bits(K, n_seg, bps, seed=9)
    seg_bits = bps * E + 5
    l = rc.awgn_rows(n_seg, seg_bits, 9)
    old = rc.awgn_rows(n_seg, bps * per, 10)
    tx0.reserve_turbo_rm()
    rx0.reserve_turbo_rm()
    d_info, d_l = torch.from_numpy(info.copy()).cuda(), torch.from_numpy(l.copy()).cuda()
    coded = torch.zeros(n_seg * seg_bits, dtype=torch.uint8, device="cuda")
    soft = torch.from_numpy(old.copy()).cuda()
    s = torch.cuda.Stream()

    def call(stream):
        tx0.turbo_encode_rm_frames(d_info, n_seg, bps, K, f1, f2, E, coded, seg_bits, rv=rv, stream=stream)
        rx0.turbo_rate_dematch_frames(d_l, n_seg, seg_bits, bps, K, E, soft, bps * per, rv=rv, accumulate=True, stream=stream)

    want_coded = rm.encode_rm_segments(info, f1, f2, E, 0, rv, seg_bits).ravel()
    want_soft = rm.dematch_segments(l, bps, K, E, 0, rv, old=old.reshape(n_seg, bps, per)).ravel()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert not coded.any() and bits_equal(soft.cpu().numpy(), old)             # capture enqueues nothing
    for _ in range(2):
        coded.zero_()
        soft.copy_(torch.from_numpy(old))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(coded.cpu().numpy(), want_coded)
        assert bits_equal(soft.cpu().numpy().ravel(), want_soft)


def test_argument_errors_leave_poisoned_outputs_untouched(om, rx0, tx0):
    K, bps, n_seg, E = 40, 2, 3, 101
    f1, f2 = tc.QPP[K]
    per = 3 * K + 12
    d_llr = dev(om, np.ones((n_seg, bps * E), np.float32))
    g_out = Guarded(om, n_seg * bps * per * 4)

    def dem(n_seg_=n_seg, stride=bps * E, bps_=bps, K_=K, E_=E, Ncb=0, rv=0, out_stride=bps * per, acc=False):
        rx0.turbo_rate_dematch_frames(d_llr, n_seg_, stride, bps_, K_, E_, g_out.addr, out_stride, Ncb=Ncb, rv=rv, accumulate=acc)

    for kw in (dict(K_=44), dict(K_=32), dict(K_=6152), dict(E_=0), dict(E_=16 * 132 + 1), dict(E_=16 * 44 + 1, Ncb=64), dict(Ncb=63),
               dict(Ncb=193), dict(Ncb=-1), dict(rv=4), dict(rv=-1), dict(stride=bps * E - 1), dict(out_stride=bps * per - 1),
               dict(n_seg_=-1), dict(bps_=-1), dict(n_seg_=2 ** 31, bps_=2 ** 20, stride=2 ** 27, out_stride=2 ** 28), dict(stride=2 ** 41)):
        with pytest.raises(ValueError):
            dem(**kw)
    dem(n_seg_=0)                                                              # no-ops
    dem(bps_=0, acc=True)
    assert g_out.untouched()

    d_info = dev(om, np.zeros((n_seg, bps, K), np.uint8))
    seg_bits = bps * E + 6
    g_coded = Guarded(om, n_seg * seg_bits)
    U, P = om.BITS_UNPACKED, om.BITS_PACKED
    for kw in (dict(K=44), dict(f1=2), dict(f2=K), dict(E=0), dict(E=16 * 132 + 1), dict(Ncb=63), dict(Ncb=193), dict(rv=4), dict(rv=-1),
               dict(seg_bits=bps * E - 1), dict(n_seg=-1), dict(bps=-1), dict(info_mode=om.BITS_NONE), dict(coded_mode=7),
               dict(coded_mode=P, seg_bits=bps * E + 4), dict(n_seg=2 ** 31, bps=2)):
        a = dict(n_seg=n_seg, bps=bps, K=K, f1=f1, f2=f2, E=E, Ncb=0, rv=0, seg_bits=seg_bits, info_mode=U, coded_mode=U)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.turbo_encode_rm_frames(d_info, a["n_seg"], a["bps"], a["K"], a["f1"], a["f2"], a["E"], g_coded.addr, a["seg_bits"],
                                       Ncb=a["Ncb"], rv=a["rv"], info_mode=a["info_mode"], coded_mode=a["coded_mode"])
    tx0.turbo_encode_rm_frames(d_info, 0, bps, K, f1, f2, E, g_coded.addr, seg_bits)        # no-op
    assert g_coded.untouched()
