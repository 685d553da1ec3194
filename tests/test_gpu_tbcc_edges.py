"""The TBCC kernels (csrc/tbcc.hip) at the places tests/test_gpu_tbcc.py does not reach (-m gpu): every shape of the decoder's last
64-step tile, exact ties and failed tail-biting, float32 subnormals and large exponents, every output on its own and off the
4-byte grid, a grid beyond 65 535 workgroups, and the encoder at the same block lengths, at its window wrap and with filler only.

The inputs come from tests/tbcc_cases.py; tests/test_tbcc_ref_host.py shows on the reference alone that they hold the ties, the
tb_ok = 0 blocks, the wrong decisions and the subnormals they are here for.  The contract (include/ofdm_mi355x.h) fixes float32
and the order of every operation, so every comparison is array_equal: bits, tb_ok and the metric's bit pattern.

Every output of every call lies between two bands of at least 64 poisoned bytes, which are checked after the call."""
import numpy as np
import pytest

import tbcc_cases as tc
import tbcc_ref

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


def gpu_decode(om, rx, llr_seg, bps, K, packed=False, want=("bits", "metric", "ok"), off=0):
    """llr_seg [n_seg][stride] -> dict(bits = the raw bit bytes, metric, ok), flat over the n_seg * bps blocks; an output that is
    not in `want` is not passed, its (poisoned) buffer is asserted untouched and its entry is None.  off moves the bit output."""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    nb = n_seg * bps
    d_llr = om.DeviceBuffer(llr_seg.nbytes).upload(llr_seg)
    g = dict(bits=Guarded(om, nb * (K // 8 if packed else K), off), metric=Guarded(om, nb * 4), ok=Guarded(om, nb * 4))
    rx.tbcc_decode_frames(d_llr, n_seg, stride, bps, K, d_bits=g["bits"].addr if "bits" in want else None,
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


def as_bits(raw, nb, K, packed):
    return np.unpackbits(raw.reshape(nb, K // 8), axis=1, bitorder="big") if packed else raw.reshape(nb, K)


def differences(om, rx, llr, K, ref, packed):
    """blocks [n][3K], one segment each, against ref = (bits, metric, tb_ok) -> list of what differs (empty: exact)"""
    rb, rm, rok = ref
    out = gpu_decode(om, rx, llr, 1, K, packed)
    bits = as_bits(out["bits"], len(llr), K, packed)
    bad = []
    if not np.array_equal(bits, rb):
        rows = np.flatnonzero(np.any(bits != rb, axis=1))
        bad.append("bits of blocks %s (first at bit %d)" % (rows.tolist()[:8], int(np.argmax(bits[rows[0]] != rb[rows[0]]))))
    if not np.array_equal(out["ok"], rok):
        bad.append("tb_ok of blocks %s" % np.flatnonzero(out["ok"] != rok).tolist()[:8])
    if out["metric"].tobytes() != rm.tobytes():
        rows = np.flatnonzero(out["metric"].view(np.uint32) != rm.view(np.uint32))
        bad.append("metric of blocks %s (%r against %r)" % (rows.tolist()[:8], out["metric"][rows[0]], rm[rows[0]]))
    return bad


def assert_exact(om, rx, llr, K, ref=None):
    ref = tbcc_ref.decode(llr) if ref is None else ref
    for packed in (False, True):
        bad = differences(om, rx, llr, K, ref, packed)
        assert not bad, "%s bits: %s" % ("packed" if packed else "unpacked", "; ".join(bad))
    return ref


# ------------------------------------------------------------------------------------------ decoder
def test_decoder_equals_reference_at_every_tile_remainder(om, rx0):
    """K = every multiple of 8 in 24..256 and 1992..2048 (T mod 64 = 0, 8 .. 56, and every K < 96), 8 blocks each: AWGN at -4 dB
    (wrong decisions among them), small integers (ties), noiseless."""
    bad = []
    for K in tc.K_SWEEP:
        llr, _, ref = tc.sweep_reference(K)
        for packed in (False, True):
            bad += ["K=%d %s: %s" % (K, "packed" if packed else "unpacked", b) for b in differences(om, rx0, llr, K, ref, packed)]
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


@pytest.mark.parametrize("lo,hi", tc.TIE_RANGES, ids=("pm1", "pm2"))
@pytest.mark.parametrize("K", tc.TIE_KS)
def test_decoder_equals_reference_on_ties_and_failed_tail_biting(om, rx0, K, lo, hi):
    """64 blocks of small integers: 1e5 steps with cand0 == cand1 (the rule: cand0), >= 20 tied end states that state 0 does not
    win (the rule: lowest index) and >= 3 blocks with tb_ok = 0 per case (tests/test_tbcc_ref_host.py)."""
    _, _, rok = assert_exact(om, rx0, tc.tie_blocks(K, lo, hi), K)
    assert (rok == 0).any()


@pytest.mark.parametrize("e", tc.SCALE_EXPONENTS)
def test_decoder_equals_reference_on_llrs_scaled_by_a_power_of_two(om, rx0, e):
    """2^-140: every LLR and every metric a float32 subnormal (flushed, the block would decode to zeros with metric 0);
    2^-126: normal and subnormal values side by side; 2^100: metrics near 2^110."""
    llr, _ = tc.scale_blocks()
    rb, rm, _ = assert_exact(om, rx0, tc.scaled(llr, e), tc.SCALE_K)
    assert rb.any() and np.all(rm != 0)


@pytest.mark.parametrize("K", tc.OUTPUT_KS)
def test_each_decoder_output_alone_and_bits_off_the_word_grid(om, rx0, K):
    """2 segments of 5 blocks at a stride of 15K + 7 floats.  Each output on its own equals the call with all three and leaves
    the buffers that were not passed alone; unpacked bits 1, 2 and 3 bytes off the 4-byte grid (the byte-wise store) and packed
    bits 1 byte off give the bytes of the aligned call."""
    seg = tc.output_segments(K)
    bps, nb = tc.OUTPUT_BPS, tc.OUTPUT_SEGS * tc.OUTPUT_BPS
    rb, rm, rok = tbcc_ref.decode_segments(seg, bps, K)
    full = {p: gpu_decode(om, rx0, seg, bps, K, packed=p) for p in (False, True)}
    for p in (False, True):
        assert np.array_equal(as_bits(full[p]["bits"], nb, K, p), rb.reshape(nb, K)), "packed" if p else "unpacked"
        assert full[p]["metric"].tobytes() == rm.tobytes() and np.array_equal(full[p]["ok"], rok.ravel())
        alone = gpu_decode(om, rx0, seg, bps, K, packed=p, want=("bits",))
        assert alone["bits"].tobytes() == full[p]["bits"].tobytes(), "bits alone (%s)" % ("packed" if p else "unpacked")
    alone = gpu_decode(om, rx0, seg, bps, K, want=("metric",))
    assert alone["metric"].tobytes() == full[False]["metric"].tobytes(), "metric alone"
    alone = gpu_decode(om, rx0, seg, bps, K, want=("ok",))
    assert alone["ok"].tobytes() == full[False]["ok"].tobytes(), "tb_ok alone"
    for off in (1, 2, 3):
        moved = gpu_decode(om, rx0, seg, bps, K, off=off)
        assert moved["bits"].tobytes() == full[False]["bits"].tobytes(), "unpacked bits at base + %d" % off
        assert moved["metric"].tobytes() == full[False]["metric"].tobytes() and moved["ok"].tobytes() == full[False]["ok"].tobytes()
    moved = gpu_decode(om, rx0, seg, bps, K, packed=True, off=1)
    assert moved["bits"].tobytes() == full[True]["bits"].tobytes(), "packed bits at base + 1"


def test_decoder_grid_beyond_65535_blocks(om, rx0):
    """70 000 blocks of K = 24 (7 000 segments of 10 at a stride of 725 floats), block n a copy of source block n mod 16; the 16
    source blocks are held against the reference in a call of their own."""
    K, n = tc.GRID_K, tc.GRID_SEGS * tc.GRID_BPS
    src = tc.grid_source()
    ref = assert_exact(om, rx0, src, K)
    small = gpu_decode(om, rx0, src, 1, K)
    big = gpu_decode(om, rx0, tc.grid_segments(src), tc.GRID_BPS, K)
    pick = np.arange(n) % tc.GRID_SRC
    assert np.array_equal(small["ok"], ref[2]) and 0 < int(ref[2].sum()) < tc.GRID_SRC
    got = big["bits"].reshape(n, K)
    rows = np.flatnonzero(np.any(got != small["bits"].reshape(tc.GRID_SRC, K)[pick], axis=1))
    assert rows.size == 0, "%d blocks differ from their source block, the first is block %d" % (rows.size, rows[0])
    assert np.array_equal(big["metric"].view(np.uint32), small["metric"].view(np.uint32)[pick])
    assert np.array_equal(big["ok"], small["ok"][pick])


# ------------------------------------------------------------------------------------------ encoder
def gpu_encode(om, tx, info, n_seg, bps, K, seg_bits, info_packed, coded_packed, off=0):
    """info [n_seg][bps][K] (None with bps = 0) -> the coded bytes [n_seg][seg_bytes] written at a guarded buffer + off"""
    d_info = None
    if info is not None:
        src = pack_msb(info) if info_packed else np.ascontiguousarray(info, np.uint8)
        d_info = om.DeviceBuffer(src.nbytes).upload(src)
    seg_bytes = seg_bits // 8 if coded_packed else seg_bits
    g = Guarded(om, n_seg * seg_bytes, off)
    tx.tbcc_encode_frames(d_info, n_seg, bps, K, g.addr, seg_bits, info_mode=om.BITS_PACKED if info_packed else om.BITS_UNPACKED,
                          coded_mode=om.BITS_PACKED if coded_packed else om.BITS_UNPACKED)
    return g.read().reshape(n_seg, seg_bytes)


def encoder_differences(om, tx, info, K, what):
    bad = []
    n_seg, bps = info.shape[:2]
    for coded_packed in (False, True):
        seg_bits = bps * 3 * K + tc.ENC_FILLER[coded_packed]
        want = tbcc_ref.encode_segments(info, seg_bits)
        want = pack_msb(want) if coded_packed else want
        for info_packed in (False, True):
            got = gpu_encode(om, tx, info, n_seg, bps, K, seg_bits, info_packed, coded_packed)
            if not np.array_equal(got, want):
                bad.append("K=%d %s info%d coded%d: %d bytes differ, the first at %s" % (
                    K, what, 8 if info_packed else 1, 8 if coded_packed else 1, int((got != want).sum()),
                    tuple(int(v[0]) for v in np.nonzero(got != want))))
    return bad


def test_encoder_equals_reference_at_every_k_in_all_four_layouts(om, tx0):
    """the decoder sweep's 38 K, 2 segments of 3 random blocks, 45 (unpacked) or 40 (packed) filler bits: segment byte counts
    that are no multiple of 4, so every second segment starts off the word grid"""
    bad = []
    for K in tc.K_SWEEP:
        bad += encoder_differences(om, tx0, tc.encoder_info(K), K, "random")
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


def test_encoder_impulses_at_the_window_wrap(om, tx0):
    """a single 1 at k in {0, 1, 5, 6, K-6, K-1}: its 15 coded ones sit where the 7-bit window wraps around the block's end"""
    bad = []
    for K in tc.K_SWEEP:
        info = tc.impulse_info(K)
        assert np.all(tbcc_ref.encode(info).sum(axis=2) == 15)
        bad += encoder_differences(om, tx0, info, K, "impulses")
    assert not bad, "%d differences:\n%s" % (len(bad), "\n".join(bad[:40]))


@pytest.mark.parametrize("coded_packed", (False, True), ids=("coded1", "coded8"))
def test_encoder_without_blocks_writes_the_filler_and_nothing_else(om, tx0, coded_packed):
    """blocks_per_seg = 0, seg_bits = 72: 72 zero bits per segment (9 packed bytes: partial words), no information buffer"""
    for off in (0, 1):
        got = gpu_encode(om, tx0, None, 3, 0, 40, 72, False, coded_packed, off=off)
        assert got.shape == (3, 9 if coded_packed else 72) and not got.any()


def test_encoder_unpacked_output_off_the_word_grid(om, tx0):
    """coded bits one per byte at base + 1, + 2 and + 3 (whole words land on other bytes, the rest goes byte by byte): the bytes
    of the aligned call"""
    bad = []
    for K in tc.K_SWEEP:
        info = tc.encoder_info(K)
        seg_bits = tc.ENC_BPS * 3 * K + tc.ENC_FILLER[False]
        want = tbcc_ref.encode_segments(info, seg_bits)
        aligned = gpu_encode(om, tx0, info, tc.ENC_SEGS, tc.ENC_BPS, K, seg_bits, False, False)
        assert np.array_equal(aligned, want), K
        for off in (1, 2, 3):
            got = gpu_encode(om, tx0, info, tc.ENC_SEGS, tc.ENC_BPS, K, seg_bits, False, False, off=off)
            if got.tobytes() != aligned.tobytes():
                bad.append("K=%d base + %d: %d bytes differ" % (K, off, int((got != aligned).sum())))
    assert not bad, "\n".join(bad[:40])
