"""The rate-matching kernels of csrc/tbcc.hip on the GPU (-m gpu): ofdm_tx_tbcc_encode_rm_frames, ofdm_tbcc_rate_dematch_frames
and ofdm_tbcc_decode_rm_frames against tests/tbcc_rm_ref.py (the contract in NumPy float32).  The contract fixes float32 and the
order of every operation, so every comparison is array_equal -- de-matched LLRs and metrics by their bit patterns.

The inputs come from tests/tbcc_rm_cases.py; tests/test_tbcc_rm_ref_host.py shows on the reference alone that they hold the
overflowing sums, the -0.0, the wrong blocks and the failed tail-biting they are here for.  Every output of every call lies
between two bands of at least 64 poisoned bytes (Guarded, as in tests/test_gpu_tbcc_edges.py), which are checked after the call."""
import numpy as np
import pytest

import tbcc_ref
import tbcc_rm_cases as rc
import tbcc_rm_ref as rm
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 0xA5


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
    that the bytes in front of it and the 64 behind it are still poison."""

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


# ------------------------------------------------------------------------------------------ encoder
def gpu_encode(om, tx, info, n_seg, bps, K, E, seg_bits, info_packed, coded_packed, off=0):
    """info [n_seg][bps][K] (None with bps = 0) -> the coded bytes [n_seg][seg_bytes] written at a guarded buffer + off"""
    d_info = None
    if info is not None:
        src = pack_msb(info) if info_packed else np.ascontiguousarray(info, np.uint8)
        d_info = om.DeviceBuffer(src.nbytes).upload(src)
    seg_bytes = seg_bits // 8 if coded_packed else seg_bits
    g = Guarded(om, n_seg * seg_bytes, off)
    tx.tbcc_encode_rm_frames(d_info, n_seg, bps, K, E, g.addr, seg_bits, info_mode=om.BITS_PACKED if info_packed else om.BITS_UNPACKED,
                             coded_mode=om.BITS_PACKED if coded_packed else om.BITS_UNPACKED)
    return g.read().reshape(n_seg, seg_bytes)


def test_encoder_equals_reference_at_every_interleaver_shape_in_all_four_layouts(om, tx0):
    """K = every multiple of 8 in 24 .. 256 (R = 1 .. 8, ND = 0, 8, 16, 24) and 1992 .. 2048, E = 2K + 3 (punctured), 3K, 4K + 1
    (repeated), 2 segments of 3 blocks and filler.  With E odd the packed blocks start inside a byte."""
    bad = []
    for K in rc.K_SWEEP:
        info = rc.enc_info(K)
        for E in rc.enc_es(K):
            for coded_packed in (False, True):
                seg_bits = rc.enc_seg_bits(K, E, coded_packed)
                want = rm.rm_encode_segments(info, E, seg_bits)
                want = pack_msb(want) if coded_packed else want
                for info_packed in (False, True):
                    got = gpu_encode(om, tx0, info, rc.ENC_SEGS, rc.ENC_BPS, K, E, seg_bits, info_packed, coded_packed)
                    if not np.array_equal(got, want):
                        bad.append("K=%d E=%d info%d coded%d: %d bytes differ, the first at %s" % (
                            K, E, 8 if info_packed else 1, 8 if coded_packed else 1, int((got != want).sum()),
                            tuple(int(v[0]) for v in np.nonzero(got != want))))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


def test_encoder_unpacked_output_off_the_word_grid(om, tx0):
    """coded bits one per byte at base + 1, + 2 and + 3: the bytes of the aligned call (which equal the reference)"""
    bad = []
    for K in rc.K_SWEEP[::3] + (2048,):
        info = rc.enc_info(K)
        for E in rc.enc_es(K):
            seg_bits = rc.enc_seg_bits(K, E, False)
            want = rm.rm_encode_segments(info, E, seg_bits)
            for off in (1, 2, 3):
                got = gpu_encode(om, tx0, info, rc.ENC_SEGS, rc.ENC_BPS, K, E, seg_bits, False, False, off=off)
                if not np.array_equal(got, want):
                    bad.append("K=%d E=%d base + %d: %d bytes differ" % (K, E, off, int((got != want).sum())))
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("coded_packed", (False, True), ids=("coded1", "coded8"))
def test_encoder_without_blocks_writes_the_filler_and_nothing_else(om, tx0, coded_packed):
    for off in (0, 1):
        got = gpu_encode(om, tx0, None, 3, 0, 40, 72, 72, False, coded_packed, off=off)
        assert got.shape == (3, 9 if coded_packed else 72) and not got.any()


# ------------------------------------------------------------------------------------------ de-matching
def gpu_dematch(om, rx, llr_seg, bps, K, E, out_pad=0):
    """llr_seg [n_seg][stride] -> de-matched [n_seg][bps * 3K + out_pad] float32 (the padding asserted untouched)"""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    out_stride = bps * 3 * K + out_pad
    d_llr = om.DeviceBuffer(llr_seg.nbytes).upload(llr_seg)
    g = Guarded(om, n_seg * out_stride * 4)
    rx.tbcc_rate_dematch_frames(d_llr, n_seg, stride, bps, K, E, g.addr, out_stride)
    out = g.read(np.float32).reshape(n_seg, out_stride)
    assert np.all(out[:, bps * 3 * K:].view(np.uint8) == POISON), "the padding between two segments' outputs was written"
    return out


def test_dematch_equals_reference_bit_for_bit(om, rx0):
    """every K of the sweep with E = K + 1, 3K - 1, 3K, 3K + 1, 6K + 5 (and 48K for K = 24, 40, 2048), 2 segments of 4 blocks at
    strides of 4E + 5 and 12K + 3 floats: noisy code words, NaN and +-inf, 3e38 sums that overflow, -0.0"""
    bad = []
    for K in rc.K_SWEEP:
        for E, (llr, _, dem, _) in rc.dm_reference(K).items():
            got = gpu_dematch(om, rx0, rc.dm_segments(llr, rc.DM_SEGS, rc.DM_BPS, rc.DM_PAD), rc.DM_BPS, K, E, out_pad=3)
            got = got[:, :rc.DM_BPS * 3 * K].reshape(8, 3 * K)
            if not np.array_equal(got.view(np.uint32), dem.view(np.uint32)):
                rows = np.flatnonzero(np.any(got.view(np.uint32) != dem.view(np.uint32), axis=1))
                x = int(np.argmax(got[rows[0]].view(np.uint32) != dem[rows[0]].view(np.uint32)))
                bad.append("K=%d E=%d: blocks %s, the first at [3i+j] = %d: %r against %r" % (
                    K, E, rows.tolist(), x, got[rows[0], x], dem[rows[0], x]))
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


# ------------------------------------------------------------------------------------------ fused decode
def gpu_decode_rm(om, rx, llr_seg, bps, K, E, packed=False, want=("bits", "metric", "ok"), off=0):
    """llr_seg [n_seg][stride] -> dict(bits = the raw bit bytes, metric, ok), flat over the n_seg * bps blocks; an output that is
    not in `want` is not passed, its (poisoned) buffer is asserted untouched and its entry is None"""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    nb = n_seg * bps
    d_llr = om.DeviceBuffer(llr_seg.nbytes).upload(llr_seg)
    g = dict(bits=Guarded(om, nb * (K // 8 if packed else K), off), metric=Guarded(om, nb * 4), ok=Guarded(om, nb * 4))
    rx.tbcc_decode_rm_frames(d_llr, n_seg, stride, bps, K, E, d_bits=g["bits"].addr if "bits" in want else None,
                             bits_mode=om.BITS_PACKED if packed else om.BITS_UNPACKED,
                             d_metric=g["metric"].addr if "metric" in want else None, d_tb_ok=g["ok"].addr if "ok" in want else None)
    out = {}
    for name, dtype in (("bits", np.uint8), ("metric", np.float32), ("ok", np.int32)):
        if name in want:
            out[name] = g[name].read(dtype)
        else:
            assert g[name].untouched(), "%s was not passed and was written" % name
            out[name] = None
    return out


def gpu_dematch_then_decode(om, rx, llr_seg, bps, K, E, packed):
    """the two-launch path: ofdm_tbcc_rate_dematch_frames into a device buffer, ofdm_tbcc_decode_frames on it"""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    nb = n_seg * bps
    d_llr = om.DeviceBuffer(llr_seg.nbytes).upload(llr_seg)
    d_mid = om.DeviceBuffer(nb * 3 * K * 4)
    g = dict(bits=Guarded(om, nb * (K // 8 if packed else K)), metric=Guarded(om, nb * 4), ok=Guarded(om, nb * 4))
    rx.tbcc_rate_dematch_frames(d_llr, n_seg, stride, bps, K, E, d_mid, bps * 3 * K)
    rx.tbcc_decode_frames(d_mid, n_seg, bps * 3 * K, bps, K, d_bits=g["bits"].addr, bits_mode=om.BITS_PACKED if packed else om.BITS_UNPACKED,
                          d_metric=g["metric"].addr, d_tb_ok=g["ok"].addr)
    return dict(bits=g["bits"].read(), metric=g["metric"].read(np.float32), ok=g["ok"].read(np.int32))


def as_bits(raw, nb, K, packed):
    return np.unpackbits(raw.reshape(nb, K // 8), axis=1, bitorder="big") if packed else raw.reshape(nb, K)


def differences(out, ref, K, packed):
    rb, rmet, rok = ref
    nb = len(rok)
    bad = []
    bits = as_bits(out["bits"], nb, K, packed)
    if not np.array_equal(bits, rb):
        rows = np.flatnonzero(np.any(bits != rb, axis=1))
        bad.append("bits of blocks %s (first at bit %d)" % (rows.tolist()[:8], int(np.argmax(bits[rows[0]] != rb[rows[0]]))))
    if not np.array_equal(out["ok"], rok):
        bad.append("tb_ok of blocks %s" % np.flatnonzero(out["ok"] != rok).tolist()[:8])
    if not np.array_equal(out["metric"].view(np.uint32), rmet.view(np.uint32)):
        rows = np.flatnonzero(out["metric"].view(np.uint32) != rmet.view(np.uint32))
        bad.append("metric of blocks %s (%r against %r)" % (rows.tolist()[:8], out["metric"][rows[0]], rmet[rows[0]]))
    return bad


def test_fused_decode_equals_dematch_plus_plain_decode_equals_reference(om, rx0):
    """the de-matching inputs' rows 0 .. 5 (noise, NaN / inf, sums that overflow to inf, -0.0) as 2 segments of 3 blocks at a
    stride of 3E + 5 floats: bits in both layouts, the float32 metric and tb_ok of the fused call and of the two-launch path"""
    bad = []
    for K in rc.K_SWEEP:
        for E, (llr, _, _, ref) in rc.dm_reference(K).items():
            seg = rc.dm_segments(llr[:rc.DM_DECODED], 2, 3, rc.DM_PAD)
            for packed in (False, True):
                bad += ["K=%d E=%d fused %s: %s" % (K, E, "packed" if packed else "unpacked", b)
                        for b in differences(gpu_decode_rm(om, rx0, seg, 3, K, E, packed), ref, K, packed)]
            bad += ["K=%d E=%d de-match + decode: %s" % (K, E, b)
                    for b in differences(gpu_dematch_then_decode(om, rx0, seg, 3, K, E, False), ref, K, False)]
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


@pytest.mark.parametrize("K", (24, 40, 2048))
def test_each_fused_output_alone_and_bits_off_the_word_grid(om, rx0, K):
    E = 6 * K + 5
    llr, _, _, (rb, rmet, rok) = rc.dm_reference(K)[E]
    seg = rc.dm_segments(llr[:rc.DM_DECODED], 2, 3, rc.DM_PAD)
    full = {p: gpu_decode_rm(om, rx0, seg, 3, K, E, packed=p) for p in (False, True)}
    for p in (False, True):
        assert not differences(full[p], (rb, rmet, rok), K, p)
        alone = gpu_decode_rm(om, rx0, seg, 3, K, E, packed=p, want=("bits",))
        assert alone["bits"].tobytes() == full[p]["bits"].tobytes(), "bits alone (%s)" % ("packed" if p else "unpacked")
    assert gpu_decode_rm(om, rx0, seg, 3, K, E, want=("metric",))["metric"].tobytes() == full[False]["metric"].tobytes()
    assert gpu_decode_rm(om, rx0, seg, 3, K, E, want=("ok",))["ok"].tobytes() == full[False]["ok"].tobytes()
    for off in (1, 2, 3):
        moved = gpu_decode_rm(om, rx0, seg, 3, K, E, off=off)
        assert moved["bits"].tobytes() == full[False]["bits"].tobytes(), "unpacked bits at base + %d" % off
    moved = gpu_decode_rm(om, rx0, seg, 3, K, E, packed=True, off=1)
    assert moved["bits"].tobytes() == full[True]["bits"].tobytes(), "packed bits at base + 1"


@pytest.mark.parametrize("K,E", ((40, 72), (40, 1920), (256, 400), (2048, 3100)))
def test_a_block_alone_in_a_batch_at_a_stride_and_on_a_repeated_call(om, rx0, K, E):
    rng = np.random.default_rng(5 + K + E)
    n = 12
    c = rng.integers(0, 2, (n, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(rm.rate_match(tbcc_ref.encode(c), E), 1.0, rng)
    ref = rm.decode_rm(llr, K)
    one = gpu_decode_rm(om, rx0, llr.reshape(1, n * E), n, K, E)                                 # one segment of 12 blocks
    assert not differences(one, ref, K, False)
    wide = rc.dm_segments(llr, 4, 3, 37)                                                         # 4 segments of 3, larger stride
    two, three = gpu_decode_rm(om, rx0, wide, 3, K, E), gpu_decode_rm(om, rx0, wide, 3, K, E)    # and the repeated call
    for name in ("bits", "metric", "ok"):
        assert one[name].tobytes() == two[name].tobytes() == three[name].tobytes(), name
    for i in range(n):
        alone = gpu_decode_rm(om, rx0, llr[i:i + 1], 1, K, E)
        assert alone["bits"].tobytes() == one["bits"][i * K:(i + 1) * K].tobytes(), i
        assert alone["metric"].tobytes() == one["metric"][i:i + 1].tobytes() and alone["ok"][0] == one["ok"][i]


@pytest.mark.parametrize("K,E", rc.PUNCTURED)
def test_fused_decode_equals_reference_where_puncturing_fails_tail_biting(om, rx0, K, E):
    """rate 8/9 and 7/9 at 3 dB, 64 blocks: wrong decisions, and tb_ok = 0 for (64, 72) (tests/test_tbcc_rm_ref_host.py)"""
    llr, c = rc.punctured_blocks(K, E)
    ref = rm.decode_rm(llr, K)
    assert np.any(ref[0] != c)
    for packed in (False, True):
        assert not differences(gpu_decode_rm(om, rx0, llr, 1, K, E, packed), ref, K, packed)
    assert not differences(gpu_dematch_then_decode(om, rx0, llr, 1, K, E, False), ref, K, False)


def test_grids_beyond_65535_blocks(om, rx0):
    """70 000 blocks of (K, E) = (24, 40) (7 000 segments of 10 at a stride of 403 floats), block n a copy of source block n mod
    16: the fused decoder's 70 000 workgroups and the de-matching kernel's 19 688 against the 16 source blocks' reference"""
    K, E, n = rc.GRID_K, rc.GRID_E, rc.GRID_SEGS * rc.GRID_BPS
    src = rc.grid_source()
    rb, rmet, rok = rm.decode_rm(src, K)
    seg = rc.grid_segments(src)
    pick = np.arange(n) % rc.GRID_SRC
    big = gpu_decode_rm(om, rx0, seg, rc.GRID_BPS, K, E)
    rows = np.flatnonzero(np.any(big["bits"].reshape(n, K) != rb[pick], axis=1))
    assert rows.size == 0, "%d blocks differ from their source block, the first is block %d" % (rows.size, rows[0])
    assert np.array_equal(big["metric"].view(np.uint32), rmet.view(np.uint32)[pick]) and np.array_equal(big["ok"], rok[pick])
    dem = gpu_dematch(om, rx0, seg, rc.GRID_BPS, K, E, out_pad=1)[:, :rc.GRID_BPS * 3 * K].reshape(n, 3 * K)
    assert np.array_equal(dem.view(np.uint32), rm.dematch(src, K).view(np.uint32)[pick])


# ------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("E", (72, 1920))
def test_encode_rm_modulate_channel_demod_decode_rm(om, torch, E):
    """64-pt QPSK, K = 40 into E = 72 (a PDCCH-shaped block, rate 5/9) and E = 1920 (PBCH-shaped, 16 copies), 8 frames of 32
    symbols (2880 coded bits: 40 blocks or 1 block per frame): random information bits -> encode_rm -> modulate_frames ->
    channel + AWGN -> demod_frames_soft -> decode_rm.  The plain rate-1/3 chain of tests/test_gpu_tbcc.py decodes this numerology
    without error at a noise variance of 10^-1.3 with 1.5 dB to spare.  E = 72 has 5/3 of that rate and runs 3 dB below that
    level.  E = 1920 = 16 x 120 puts all 16 copies of a coded bit on the same subcarrier (120 bits per symbol), so repetition buys
    no diversity against the bins the reference taps fade; it runs 2 dB below that level (at 10^-1.0 the reference decoded 1 of
    the 8 blocks wrongly).  That the level is low enough is asserted on the reference below."""
    N, cp, Kd, K, n_sym, n = 64, 16, 60, 40, 32, 8
    nv = 10 ** -1.6 if E == 72 else 10 ** -1.5
    L = N + cp
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), "QPSK")
    rxe = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 100, 0.7, modulation="QPSK")
    rxe.set_max_trials(0)
    seg_bits = txe.bits_per_frame(n_sym)
    nblk = om.tbcc_rm_blocks(seg_bits, K, E)
    assert nblk == seg_bits // E >= 1
    rng = np.random.default_rng(E)
    info = rng.integers(0, 2, (n, nblk, K)).astype(np.uint8)
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * seg_bits)
    txe.tbcc_encode_rm_frames(d_info, n, nblk, K, E, d_coded, seg_bits)
    coded = d_coded.download(np.uint8, n * seg_bits).reshape(n, seg_bits)
    assert np.array_equal(coded, rm.rm_encode_segments(info, E, seg_bits))
    fl_tx, fl = n_sym * L, n_sym * L + cp
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = np.zeros(cp + 1, np.complex64)
    taps[:5] = orc.REF_TAPS / np.linalg.norm(orc.REF_TAPS)
    d_t = om.DeviceBuffer(taps.nbytes).upload(taps)
    txe.modulate_frames(d_coded, n, n_sym, d_tx)
    txe.channel(d_tx, n, fl_tx, fl_tx, d_t, len(taps), d_rx, fl, fl, noise_var=nv, seed=11)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds * Kd * 2 == seg_bits
    d_eq, d_llr, d_tsr = om.DeviceBuffer(n * nds * Kd * 8), om.DeviceBuffer(n * seg_bits * 4), om.DeviceBuffer(n * 16)
    assert rxe.demod_frames_soft(d_rx, n, fl, fl, d_eq, d_llr=d_llr, d_tsr=d_tsr) == nds
    assert d_tsr.download(np.int32, n * 4).reshape(n, 4)[:, 3].all()
    llr = d_llr.download(np.float32, n * seg_bits).reshape(n, seg_bits)
    raw_ber = float(((llr[:, :nblk * E] < 0).astype(np.uint8) != coded[:, :nblk * E]).mean())
    rb, rmet, rok = rm.decode_rm_segments(llr, nblk, K, E)
    wrong_ref = int(np.any(rb != info, axis=2).sum())
    print("E=%d nv=%.3g: raw BER %.4f, %d blocks, the reference decodes %d wrongly" % (E, nv, raw_ber, n * nblk, wrong_ref))
    assert wrong_ref == 0, "the noise is to be low enough for the reference to decode the GPU's own LLRs without a block error"
    nb = n * nblk
    d_bits, d_m, d_ok = om.DeviceBuffer(nb * K), om.DeviceBuffer(nb * 4), om.DeviceBuffer(nb * 4)
    rxe.reserve_tbcc(nb, K)
    rxe.tbcc_decode_rm_frames(d_llr, n, seg_bits, nblk, K, E, d_bits=d_bits, d_metric=d_m, d_tb_ok=d_ok)
    bits = d_bits.download(np.uint8, nb * K).reshape(n, nblk, K)
    assert np.array_equal(bits, rb) and np.array_equal(bits, info)
    assert np.array_equal(d_m.download(np.float32, nb).view(np.uint32), rmet.ravel().view(np.uint32))
    assert np.array_equal(d_ok.download(np.int32, nb), rok.ravel())


# ------------------------------------------------------------------------------------------ capture, errors
def test_fused_decode_is_capturable_after_reserve(om, torch):
    """a handle of its own, so that the first ofdm_tbcc_decode_rm_frames of this process may be the captured one's warm-up"""
    K, E, n_seg, bps = 256, 400, 6, 5
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    rng = np.random.default_rng(9)
    c = rng.integers(0, 2, (n_seg * bps, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(rm.rate_match(tbcc_ref.encode(c), E), 2.0, rng)
    rx.reserve_tbcc(n_seg * bps, K)
    d_llr = torch.from_numpy(llr.reshape(n_seg, bps * E)).cuda()
    outs = dict(bits=torch.zeros(n_seg * bps * K // 8, dtype=torch.uint8, device="cuda"),
                metric=torch.zeros(n_seg * bps, dtype=torch.float32, device="cuda"),
                ok=torch.zeros(n_seg * bps, dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()

    def call(stream):
        rx.tbcc_decode_rm_frames(d_llr, n_seg, bps * E, bps, K, E, d_bits=outs["bits"], bits_mode=om.BITS_PACKED,
                                 d_metric=outs["metric"], d_tb_ok=outs["ok"], stream=stream)

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    rb, rmet, rok = rm.decode_rm(llr, K)
    assert np.array_equal(eager["bits"].cpu().numpy(), pack_msb(rb).ravel())
    assert np.array_equal(eager["metric"].cpu().numpy(), rmet) and np.array_equal(eager["ok"].cpu().numpy(), rok)
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                                     # one stream, one kernel node: no parallel branch
        call(torch.cuda.current_stream().cuda_stream)
    assert not outs["metric"].any()                                         # capture enqueues nothing
    for _ in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], eager[k]), k


def test_argument_errors_leave_poisoned_outputs_untouched(om, rx0, tx0):
    K, E, bps, n_seg = 40, 72, 2, 3
    llr = np.ones((n_seg, bps * E), np.float32)
    d_llr = om.DeviceBuffer(llr.nbytes).upload(llr)
    nb = n_seg * bps
    g = dict(bits=Guarded(om, nb * K), metric=Guarded(om, nb * 4), ok=Guarded(om, nb * 4), dem=Guarded(om, nb * 3 * K * 4))

    def dec(n_seg_, stride, bps_, K_, E_, mode=om.BITS_UNPACKED):
        rx0.tbcc_decode_rm_frames(d_llr, n_seg_, stride, bps_, K_, E_, d_bits=g["bits"].addr, bits_mode=mode, d_metric=g["metric"].addr,
                                  d_tb_ok=g["ok"].addr)

    def dem(n_seg_, stride, bps_, K_, E_, out_stride=bps * 3 * K):
        rx0.tbcc_rate_dematch_frames(d_llr, n_seg_, stride, bps_, K_, E_, g["dem"].addr, out_stride)

    geometry = ((n_seg, bps * E, bps, 44, E), (n_seg, bps * E, bps, 16, E), (n_seg, bps * E, bps, 2056, E), (n_seg, bps * E, bps, K, 0),
                (n_seg, bps * E, bps, K, 48 * K + 1), (n_seg, bps * E, bps, K, -3), (n_seg, bps * E - 1, bps, K, E),
                (-1, bps * E, bps, K, E), (n_seg, bps * E, -1, K, E), (2 ** 31, bps * E, 2, K, E), (n_seg, 2 ** 41, bps, K, E))
    for args in geometry:
        with pytest.raises(ValueError):
            dec(*args)
        with pytest.raises(ValueError):
            dem(*args)
    with pytest.raises(ValueError):
        dec(n_seg, bps * E, bps, K, E, om.BITS_NONE)
    with pytest.raises(ValueError):
        dem(n_seg, bps * E, bps, K, E, out_stride=bps * 3 * K - 1)
    with pytest.raises(ValueError):
        dem(n_seg, bps * E, bps, K, E, out_stride=2 ** 41)
    dec(0, bps * E, bps, K, E)                                              # no-ops
    dec(n_seg, bps * E, 0, K, E)
    dem(0, bps * E, bps, K, E)
    dem(n_seg, bps * E, 0, K, E)
    rx0.tbcc_decode_rm_frames(d_llr, n_seg, bps * E, bps, K, E)
    assert all(v.untouched() for v in g.values())

    info = np.zeros((n_seg, bps, K), np.uint8)
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    seg_bits = bps * E + 8
    coded = Guarded(om, n_seg * seg_bits)
    U, P = om.BITS_UNPACKED, om.BITS_PACKED
    for kw in (dict(K=44), dict(E=0), dict(E=48 * K + 1), dict(seg_bits=bps * E - 1), dict(n_seg=-1), dict(bps=-1),
               dict(info_mode=om.BITS_NONE), dict(coded_mode=7), dict(coded_mode=P, seg_bits=bps * E + 4), dict(n_seg=2 ** 31, bps=2)):
        a = dict(n_seg=n_seg, bps=bps, K=K, E=E, seg_bits=seg_bits, info_mode=U, coded_mode=U)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.tbcc_encode_rm_frames(d_info, a["n_seg"], a["bps"], a["K"], a["E"], coded.addr, a["seg_bits"], info_mode=a["info_mode"],
                                      coded_mode=a["coded_mode"])
    tx0.tbcc_encode_rm_frames(d_info, 0, bps, K, E, coded.addr, seg_bits)   # no-op
    assert coded.untouched()
