"""The LTE turbo codec of the frame-batched path on the GPU (-m gpu): ofdm_tx_turbo_encode_frames and ofdm_turbo_decode_frames
against tests/turbo_ref.py (the contract in NumPy float32).  Every comparison is array_equal -- bits and float32 LLR values --
and every output sits between poisoned guard bands.  The decoder inputs come from tests/turbo_cases.py, whose operating point
tests/test_turbo_ref_host.py asserts on the reference alone: the blocks compared here include wrongly decoded ones."""
import functools

import numpy as np
import pytest

import turbo_cases as tc
import turbo_ref as tr

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64
ENC_CASES = [(K,) + tc.QPP[K] for K in tc.ENC_KS] + [tc.IDENTITY]


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
    """any receiver handle serves the decoder (it reads LLR buffers, not the handle's numerology)"""
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


@pytest.fixture(scope="module")
def tx0(om, torch):
    return om.TxEngine(64, 16, 62, 60)


def pack_msb(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="big")


class Guarded:
    """nbytes of device memory at .addr = allocation + 64 + off, everything poisoned; read() returns the payload after asserting
    that the bytes in front of it and the 64 behind it are still poison"""

    def __init__(self, om, nbytes, off=0):
        self.nbytes, self.lo = int(nbytes), GUARD + off
        self.total = self.lo + self.nbytes + GUARD
        self.buf = om.DeviceBuffer(self.total).upload(np.full(self.total, POISON, np.uint8))
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


def gpu_encode(om, tx, info, f1, f2, seg_bits, info_packed, coded_packed, off=0):
    """info [n_seg][bps][K] -> the coded buffer's bytes [n_seg][seg_bytes], written at allocation + 64 + off"""
    n_seg, bps, K = info.shape
    src = pack_msb(info) if info_packed else info
    seg_bytes = seg_bits // 8 if coded_packed else seg_bits
    g = Guarded(om, n_seg * seg_bytes, off)
    tx.turbo_encode_frames(dev(om, src), n_seg, bps, K, f1, f2, g.addr, seg_bits, info_mode=om.BITS_PACKED if info_packed else om.BITS_UNPACKED,
                           coded_mode=om.BITS_PACKED if coded_packed else om.BITS_UNPACKED)
    return g.read().reshape(n_seg, seg_bytes)


def gpu_decode(om, rx, llr_seg, bps, K, f1, f2, n_iter, packed=False, want_bits=True, want_llr=True):
    """llr_seg [n_seg][stride] float32 -> (bits [n_seg][bps][K] or None, llr [n_seg][bps][K] or None), both from guarded buffers"""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    nb = n_seg * bps
    g_bits = Guarded(om, nb * (K // 8 if packed else K), 1)
    g_llr = Guarded(om, nb * K * 4)
    rx.turbo_decode_frames(dev(om, llr_seg), n_seg, stride, bps, K, f1, f2, n_iter, d_bits=g_bits.addr if want_bits else None,
                           bits_mode=om.BITS_PACKED if packed else om.BITS_UNPACKED, d_llr_out=g_llr.addr if want_llr else None)
    bits = out = None
    if want_bits:
        raw = g_bits.read()
        bits = (np.unpackbits(raw.reshape(nb, K // 8), axis=1, bitorder="big") if packed else raw.reshape(nb, K)).reshape(n_seg, bps, K)
    else:
        assert g_bits.untouched()
    if want_llr:
        out = g_llr.read(np.float32).reshape(n_seg, bps, K)
    else:
        assert g_llr.untouched()
    return bits, out


def check_decode(om, rx, llr, K, f1, f2, n_iter, want):
    """blocks [n][3K + 12], one per segment -> bits and llr equal to `want` = (bits, llr) of the reference"""
    bits, out = gpu_decode(om, rx, llr, 1, K, f1, f2, n_iter)
    bad = np.any(out[:, 0] != want[1], axis=1)
    assert np.array_equal(out[:, 0], want[1]), "llr differs in blocks %s: max |d| = %g" % (
        np.flatnonzero(bad)[:8], float(np.nanmax(np.abs(out[:, 0] - want[1]))))
    assert np.array_equal(bits[:, 0], want[0])


# ------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("coded_packed", (False, True), ids=("coded1", "coded8"))
@pytest.mark.parametrize("info_packed", (False, True), ids=("info1", "info8"))
@pytest.mark.parametrize("K,f1,f2", ENC_CASES, ids=lambda v: str(v))
def test_encoder_equals_reference_and_writes_the_filler(om, tx0, K, f1, f2, info_packed, coded_packed):
    """1, 7 and 9 blocks per segment (an odd count leaves half a wave idle; from 2 on, packed blocks start inside a byte), segment
    byte counts that are no multiple of 4"""
    for bps in (1, 7, 9):
        info = np.random.default_rng(K + bps).integers(0, 2, (2, bps, K)).astype(np.uint8)
        seg_bits = bps * (3 * K + 12) + ((44 if bps & 1 else 40) if coded_packed else 45)
        assert not coded_packed or seg_bits % 8 == 0
        want = tr.encode_segments(info, f1, f2, seg_bits)
        got = gpu_encode(om, tx0, info, f1, f2, seg_bits, info_packed, coded_packed)
        if coded_packed:
            want = pack_msb(want)
        assert np.array_equal(got, want), "bps=%d: %d bytes differ" % (bps, int((got != want).sum()))


@pytest.mark.parametrize("K", (40, 104, 1024))
def test_encoder_filler_only_and_unaligned_output(om, tx0, K):
    f1, f2 = tc.QPP[K]
    for packed in (False, True):                             # no block at all: the segment is filler
        got = gpu_encode(om, tx0, np.zeros((3, 0, K), np.uint8), f1, f2, 104, False, packed)
        assert got.shape == (3, 13 if packed else 104) and not got.any()
    info = np.random.default_rng(K).integers(0, 2, (3, 2, K)).astype(np.uint8)
    seg_bits = 2 * (3 * K + 12) + 5
    want = tr.encode_segments(info, f1, f2, seg_bits)
    for off in (1, 2, 3):                                    # one bit per byte at base + 1 .. 3: no whole-word store may be used
        assert np.array_equal(gpu_encode(om, tx0, info, f1, f2, seg_bits, True, False, off=off), want), off
    ones = np.full((1, 3, K), 0xFF, np.uint8)                # only bit 0 of an unpacked information byte is read
    assert np.array_equal(gpu_encode(om, tx0, ones, f1, f2, 3 * (3 * K + 12), False, False),
                          tr.encode_segments(ones & 1, f1, f2, 3 * (3 * K + 12)))


# ------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("n_iter", tc.DEC_ITERS)
@pytest.mark.parametrize("K", tc.DEC_KS)
def test_decoder_equals_reference_at_the_operating_point(om, rx0, K, n_iter):
    """17 noisy blocks per K at the recorded Es/N0, decoded as 1, 7, 8, 9 and 17 blocks (partial 8-block groups)"""
    llr, _, rbits, rout = tc.decoded(K, n_iter)
    for n in tc.DEC_COUNTS:
        check_decode(om, rx0, llr[:n], K, *tc.QPP[K], n_iter, (rbits[:n], rout[:n]))


def test_decoder_equals_reference_at_the_largest_block(om, rx0):
    K, n = tc.BIG_K, tc.BIG_BLOCKS
    llr, _, rbits, rout = tc.decoded(K, tc.BIG_ITERS, n)
    check_decode(om, rx0, llr, K, *tc.QPP[K], tc.BIG_ITERS, (rbits, rout))


@functools.lru_cache(maxsize=None)
def edge_reference(K, n_iter):
    llr = tc.edge_blocks(K)
    return (llr,) + tr.decode(llr, *tc.QPP[K], n_iter)


@pytest.mark.parametrize("n_iter", (1, 3))
@pytest.mark.parametrize("K", (40, 56, 72, 120))
def test_decoder_equals_reference_on_edge_values(om, rx0, K, n_iter):
    """NaN, +-inf, +-0 and subnormals by bit pattern, all-zero LLRs (every max ties), small integers (many exact ties)"""
    llr, rbits, rout = edge_reference(K, n_iter)
    check_decode(om, rx0, llr, K, *tc.QPP[K], n_iter, (rbits, rout))
    assert not rbits[2].any() and not rbits[6].any() and not rout[2].any()


def test_identity_interleaver(om, rx0):
    K, f1, f2 = tc.IDENTITY
    rng = np.random.default_rng(11)
    c = rng.integers(0, 2, (9, K)).astype(np.uint8)
    llr = tr.awgn_llrs(tr.encode(c, f1, f2), -3.0, rng)
    check_decode(om, rx0, llr, K, f1, f2, 2, tr.decode(llr, f1, f2, 2))


@pytest.mark.parametrize("K", (40, 120, 520))
def test_a_block_alone_in_a_batch_at_a_stride_and_on_a_repeated_call(om, rx0, K):
    f1, f2 = tc.QPP[K]
    llr, _, rbits, rout = tc.decoded(K, 2)
    n, per = 12, 3 * K + 12
    llr = llr[:n]
    alone = [gpu_decode(om, rx0, llr[i:i + 1], 1, K, f1, f2, 2) for i in range(n)]
    b1, o1 = gpu_decode(om, rx0, llr.reshape(1, n * per), n, K, f1, f2, 2)                        # one segment of 12 blocks
    wide = np.full((4, 3 * per + 37), np.nan, np.float32)                                         # 4 segments of 3, poisoned gaps
    wide[:, :3 * per] = llr.reshape(4, 3 * per)
    b2, o2 = gpu_decode(om, rx0, wide, 3, K, f1, f2, 2)
    b3, o3 = gpu_decode(om, rx0, wide, 3, K, f1, f2, 2)                                           # repeated call
    assert b1.tobytes() == b2.tobytes() == b3.tobytes() and o1.tobytes() == o2.tobytes() == o3.tobytes()
    for i in range(n):
        assert alone[i][0].tobytes() == b1[0, i].tobytes() and alone[i][1].tobytes() == o1[0, i].tobytes(), i
    assert np.array_equal(o1[0], rout[:n]) and np.array_equal(b1[0], rbits[:n])


@pytest.mark.parametrize("K", (40, 512))
def test_each_output_alone_packed_and_unpacked(om, rx0, K):
    f1, f2 = tc.QPP[K]
    llr, _, rbits, rout = tc.decoded(K, 2)
    seg = np.full((3, 5 * (3 * K + 12) + 7), np.nan, np.float32)
    seg[:, :5 * (3 * K + 12)] = llr[:15].reshape(3, -1)
    want_b, want_o = rbits[:15].reshape(3, 5, K), rout[:15].reshape(3, 5, K)
    for packed in (False, True):
        b, o = gpu_decode(om, rx0, seg, 5, K, f1, f2, 2, packed=packed)
        assert np.array_equal(b, want_b) and np.array_equal(o, want_o)
        b, o = gpu_decode(om, rx0, seg, 5, K, f1, f2, 2, packed=packed, want_llr=False)
        assert np.array_equal(b, want_b) and o is None
    b, o = gpu_decode(om, rx0, seg, 5, K, f1, f2, 2, want_bits=False)
    assert b is None and np.array_equal(o, want_o)
    gpu_decode(om, rx0, seg, 5, K, f1, f2, 2, want_bits=False, want_llr=False)                    # no pointer at all: a no-op


def test_grid_of_twenty_thousand_blocks(om, rx0):
    """20 000 blocks of K = 40 at n_iter = 1 (2 500 waves), block n of the batch = source block n mod 16, each equal to the
    reference"""
    K, f1, f2 = tc.GRID_K, *tc.QPP[tc.GRID_K]
    src = tc.grid_source()
    rbits, rout = tr.decode(src, f1, f2, 1)
    pick = np.arange(tc.GRID_BLOCKS) % tc.GRID_SRC
    bps = 10
    seg = np.full((tc.GRID_BLOCKS // bps, bps * (3 * K + 12) + 5), np.nan, np.float32)
    seg[:, :bps * (3 * K + 12)] = src[pick].reshape(tc.GRID_BLOCKS // bps, -1)
    bits, out = gpu_decode(om, rx0, seg, bps, K, f1, f2, 1)
    assert np.array_equal(out.reshape(-1, K), rout[pick]) and np.array_equal(bits.reshape(-1, K), rbits[pick])


# ------------------------------------------------------------------------------------------ the whole chain
def test_crc_encode_scramble_modulate_channel_demod_descramble_decode_check(om, torch):
    """payload + gCRC24A -> turbo encode -> scramble -> modulate (2048-pt 16-QAM) -> channel + AWGN -> demod_frames_soft ->
    descramble -> turbo decode -> crc_check: the decoded bits are the reference decoder's on that call's LLRs, and the CRC flags
    exactly the blocks the reference decodes wrongly."""
    from oracle import ofdm_oracle as orc
    N, cp, Kd, mod, n_sym, n, K, n_iter, nv = 2048, 144, 1200, "16QAM", 16, 2, 512, 2, 0.1
    f1, f2 = tc.QPP[K]
    A, L = K - 24, N + cp
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    rxe = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 100, 0.7, modulation=mod)
    rxe.set_max_trials(0)
    seg_bits = txe.bits_per_frame(n_sym)
    bps = om.turbo_blocks(seg_bits, K)
    assert bps == seg_bits // (3 * K + 12) and bps >= 12
    rng = np.random.default_rng(N)
    payload = rng.integers(0, 2, (n * bps, A)).astype(np.uint8)
    cinit = np.array([0x1234567, 0x7654321], np.uint32)
    d_cinit = dev(om, cinit)
    d_info, d_coded = om.DeviceBuffer(n * bps * K), om.DeviceBuffer(n * seg_bits)
    txe.crc_attach_frames(dev(om, payload), n * bps, A, om.CRC24A, d_info)
    info = d_info.download(np.uint8, n * bps * K).reshape(n, bps, K)
    assert np.array_equal(info[:, :, :A].reshape(-1, A), payload)
    txe.turbo_encode_frames(d_info, n, bps, K, f1, f2, d_coded, seg_bits)
    assert np.array_equal(d_coded.download(np.uint8, n * seg_bits).reshape(n, seg_bits), tr.encode_segments(info, f1, f2, seg_bits))
    txe.scramble_frames(d_coded, n, seg_bits, d_cinit, d_coded)
    fl_tx, fl = n_sym * L, n_sym * L + cp
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = np.zeros(cp + 1, np.complex64)
    taps[:5] = orc.REF_TAPS / np.linalg.norm(orc.REF_TAPS)
    txe.modulate_frames(d_coded, n, n_sym, d_tx)
    txe.channel(d_tx, n, fl_tx, fl_tx, dev(om, taps), len(taps), d_rx, fl, fl, noise_var=nv, seed=11)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds * Kd * 4 == seg_bits
    d_eq, d_llr = om.DeviceBuffer(n * nds * Kd * 8), om.DeviceBuffer(n * seg_bits * 4)
    assert rxe.demod_frames_soft(d_rx, n, fl, fl, d_eq, d_llr=d_llr) == nds
    rxe.descramble_llr_frames(d_llr, n, seg_bits, seg_bits, d_cinit, d_llr)
    llr = d_llr.download(np.float32, n * seg_bits).reshape(n, seg_bits)
    g_bits, g_ok = Guarded(om, n * bps * K), Guarded(om, n * bps)
    rxe.turbo_decode_frames(d_llr, n, seg_bits, bps, K, f1, f2, n_iter, d_bits=g_bits.addr)
    rxe.crc_check_frames(g_bits.addr, n * bps, A, om.CRC24A, d_ok=g_ok.addr)
    bits, ok = g_bits.read().reshape(n, bps, K), g_ok.read().reshape(n, bps)
    rbits, _ = tr.decode_segments(llr, bps, K, f1, f2, n_iter)
    wrong = np.any(rbits != info, axis=2)
    print("chain K=%d nv=%g n_iter=%d: %d of %d blocks decoded wrongly by the reference" % (K, nv, n_iter, int(wrong.sum()), n * bps))
    assert np.array_equal(bits, rbits)
    assert np.array_equal(ok == 0, wrong)


# ------------------------------------------------------------------------------------------ capture, errors
def test_decode_is_capturable_after_reserve(om, torch, rx0):
    K, n_seg, bps, n_iter = 120, 3, 5, 2
    f1, f2 = tc.QPP[K]
    llr, _, rbits, rout = tc.decoded(K, n_iter)
    llr = llr[:n_seg * bps].reshape(n_seg, bps * (3 * K + 12))
    rx0.reserve_turbo(n_seg * bps, K)
    d_llr = torch.from_numpy(llr.copy()).cuda()
    outs = dict(bits=torch.zeros(n_seg * bps * K // 8, dtype=torch.uint8, device="cuda"),
                llr=torch.zeros(n_seg * bps * K, dtype=torch.float32, device="cuda"))
    s = torch.cuda.Stream()

    def call(stream):
        rx0.turbo_decode_frames(d_llr, n_seg, bps * (3 * K + 12), bps, K, f1, f2, n_iter, d_bits=outs["bits"], bits_mode=om.BITS_PACKED,
                                d_llr_out=outs["llr"], stream=stream)

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert np.array_equal(eager["bits"].cpu().numpy(), pack_msb(rbits[:n_seg * bps]).ravel())
    assert np.array_equal(eager["llr"].cpu().numpy(), rout[:n_seg * bps].ravel())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert not outs["llr"].any()                                            # capture enqueues nothing
    for _ in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], eager[k]), k


def test_argument_errors_leave_poisoned_outputs_untouched(om, rx0, tx0):
    import ctypes as C
    from ofdm_mi355x import _lib
    K, bps, n_seg = 40, 2, 3
    f1, f2 = tc.QPP[K]
    per = 3 * K + 12
    d_llr = dev(om, np.ones((n_seg, bps * per), np.float32))
    g_bits, g_llr = Guarded(om, n_seg * bps * K), Guarded(om, n_seg * bps * K * 4)

    def dec(n_seg_=n_seg, stride=bps * per, bps_=bps, K_=K, f1_=f1, f2_=f2, n_iter=2, mode=om.BITS_UNPACKED):
        rx0.turbo_decode_frames(d_llr, n_seg_, stride, bps_, K_, f1_, f2_, n_iter, d_bits=g_bits.addr, bits_mode=mode, d_llr_out=g_llr.addr)

    for kw in (dict(K_=44), dict(K_=32), dict(K_=6152), dict(f1_=2), dict(f1_=K), dict(f2_=-1), dict(n_iter=0), dict(n_iter=17),
               dict(stride=bps * per - 1), dict(n_seg_=-1), dict(bps_=-1), dict(n_seg_=2 ** 31, bps_=2), dict(stride=2 ** 41),
               dict(mode=om.BITS_NONE)):
        with pytest.raises(ValueError):
            dec(**kw)
    out = _lib.TurboOut(g_bits.addr, om.BITS_UNPACKED, g_llr.addr)
    assert om.load().ofdm_turbo_decode_frames(None, d_llr.data_ptr(), n_seg, bps * per, bps, K, f1, f2, 2, C.byref(out), None) != 0
    for bad in ((4, 20), (-1, 40), (4, 6152)):
        with pytest.raises(ValueError):
            rx0.reserve_turbo(*bad)
    dec(n_seg_=0)                                                           # no-ops
    dec(bps_=0)
    rx0.turbo_decode_frames(d_llr, n_seg, bps * per, bps, K, f1, f2, 2)
    assert g_bits.untouched() and g_llr.untouched()

    d_info = dev(om, np.zeros((n_seg, bps, K), np.uint8))
    seg_bits = bps * per + 8
    g_coded = Guarded(om, n_seg * seg_bits)
    U, P = om.BITS_UNPACKED, om.BITS_PACKED
    for kw in (dict(K=44), dict(f1=2), dict(f2=K), dict(seg_bits=bps * per - 1), dict(n_seg=-1), dict(bps=-1), dict(info_mode=om.BITS_NONE),
               dict(coded_mode=7), dict(coded_mode=P, seg_bits=bps * per + 4), dict(n_seg=2 ** 31, bps=2)):
        a = dict(n_seg=n_seg, bps=bps, K=K, f1=f1, f2=f2, seg_bits=seg_bits, info_mode=U, coded_mode=U)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.turbo_encode_frames(d_info, a["n_seg"], a["bps"], a["K"], a["f1"], a["f2"], g_coded.addr, a["seg_bits"],
                                    info_mode=a["info_mode"], coded_mode=a["coded_mode"])
    tx0.turbo_encode_frames(d_info, 0, bps, K, f1, f2, g_coded.addr, seg_bits)      # no-op
    assert g_coded.untouched()
