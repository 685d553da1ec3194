"""The kernels of csrc/bitproc.hip on the GPU (-m gpu): ofdm_tx_scramble_frames, ofdm_descramble_llr_frames,
ofdm_tx_crc_attach_frames and ofdm_crc_check_frames against tests/lte_bits_ref.py (bit-serial CRC, Gold sequence stepped from 0),
and the coded chain they close.  Everything here is exact: every comparison is array_equal, floats by their bit patterns.
Every output of every call lies between two bands of at least 64 poisoned bytes (Guarded, as in tests/test_gpu_tbcc_rm.py),
which are checked after the call.  tests/test_lte_bits_ref_host.py pins the reference and shows on it alone that the noisy
chain case holds the wrong blocks it is here for."""
import functools

import numpy as np
import pytest

import lte_bits_ref as lb
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 0xA5
CH, SPAN = 1024, 65536                                       # GOLD_CH, GOLD_SPAN of csrc/ofdm_launch.hpp
CINITS = np.array([0, 0x12345, 0xFFFFFFFF], np.uint32)       # the last one: bit 31 is ignored
SEG_BITS = (1, 7, 8, 31, 32, 33, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, SPAN - 1, SPAN, SPAN + 1, 100003)
KINDS = (lb.CRC24A, lb.CRC24B, lb.CRC16, lb.CRC8)


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
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


@pytest.fixture(scope="module")
def tx0(om, torch):
    return om.TxEngine(64, 16, 62, 60)


def pack_msb(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="big")


class Guarded:
    """nbytes of device memory at .addr = allocation + 64 + off, everything poisoned; read() returns the payload after asserting
    that the bytes in front of it and the 64 behind it are still poison.  fill() puts an input there (in-place calls)."""

    def __init__(self, om, nbytes, off=0):
        self.om = om
        self.nbytes, self.lo = int(nbytes), GUARD + off
        self.total = self.lo + self.nbytes + GUARD
        self.buf = om.DeviceBuffer(self.total).upload(np.full(self.total, POISON, np.uint8))
        self.addr = self.buf.data_ptr() + self.lo

    def fill(self, arr):
        raw = np.full(self.total, POISON, np.uint8)
        src = np.ascontiguousarray(arr).view(np.uint8).ravel()
        assert src.size == self.nbytes
        raw[self.lo:self.lo + self.nbytes] = src
        self.buf.upload(raw)
        return self

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


# ------------------------------------------------------------------------------------------ scrambling of bits
def seg_input(seg_bits, salt=0):
    """[3][seg_bits] bytes whose bit 0 is the data and whose other bits are set at random: only bit 0 may be read"""
    rng = np.random.default_rng(10 * seg_bits + salt)
    return rng.integers(0, 256, (len(CINITS), seg_bits)).astype(np.uint8)


def gpu_scramble(om, tx, src, seg_bits, packed, off=0, in_place=False, cinit=CINITS):
    """src [n_seg][seg_bytes] bytes as the call reads them -> what it writes, [n_seg][seg_bytes]"""
    n_seg, seg_bytes = src.shape
    d_c = dev(om, cinit)
    g = Guarded(om, src.size, off)
    if in_place:
        g.fill(src)
        d_in = g.addr
    else:
        d_src = dev(om, src)
        d_in = d_src
    tx.scramble_frames(d_in, n_seg, seg_bits, d_c, g.addr, mode=om.BITS_PACKED if packed else om.BITS_UNPACKED)
    return g.read().reshape(n_seg, seg_bytes)


def test_scramble_unpacked_at_every_path_length(om, tx0):
    """tails of 0 .. 3 bytes, one lane / one chunk / one span and one more, two spans; bytes with junk above bit 0"""
    bad = []
    for n in SEG_BITS:
        src = seg_input(n)
        want = lb.scramble(src & 1, CINITS)
        for in_place in (False, True):
            got = gpu_scramble(om, tx0, src, n, False, in_place=in_place)
            if not np.array_equal(got, want):
                bad.append("seg_bits=%d in_place=%d: %d bytes differ, the first at %s" % (
                    n, in_place, int((got != want).sum()), tuple(int(v[0]) for v in np.nonzero(got != want))))
    assert not bad, "\n".join(bad)


def test_scramble_unpacked_off_the_word_grid(om, tx0):
    bad = []
    for n in (1, 7, 33, 257, CH + 1, SPAN + 1):
        src = seg_input(n, 1)
        want = lb.scramble(src & 1, CINITS)
        for off in (1, 2, 3):
            for in_place in (False, True):
                got = gpu_scramble(om, tx0, src, n, False, off=off, in_place=in_place)
                if not np.array_equal(got, want):
                    bad.append("seg_bits=%d base + %d in_place=%d: %d bytes differ" % (n, off, in_place, int((got != want).sum())))
    assert not bad, "\n".join(bad)


def test_scramble_packed_at_every_path_length(om, tx0):
    """the multiples of 8 of the list (and 40, 72: segments of 5 and 9 bytes put the later segments off the word grid)"""
    bad = []
    for n in tuple(v for v in SEG_BITS if v % 8 == 0) + (40, 72, SPAN + 8, 100000):
        bits = seg_input(n, 2) & 1
        want = pack_msb(lb.scramble(bits, CINITS))
        for off, in_place in ((0, False), (0, True), (1, False), (3, True)):
            got = gpu_scramble(om, tx0, pack_msb(bits), n, True, off=off, in_place=in_place)
            if not np.array_equal(got, want):
                bad.append("seg_bits=%d base + %d in_place=%d: %d bytes differ" % (n, off, in_place, int((got != want).sum())))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------ descrambling of LLRs
SPECIALS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF,
                     0x00800000, 0x7F7FFFFF], np.uint32)     # NaNs with payloads, +-inf, +-0, subnormals, the normal extremes


def llr_input(seg_bits, stride, salt=0):
    """uint32 patterns [3][stride]: random words with the specials spread over them; the gap behind seg_bits is POISON"""
    rng = np.random.default_rng(7 * seg_bits + salt)
    x = rng.integers(0, 1 << 32, (len(CINITS), stride), dtype=np.uint64).astype(np.uint32)
    pos = rng.integers(0, seg_bits, (len(CINITS), 2 * len(SPECIALS)))
    for s in range(len(CINITS)):
        x[s, pos[s]] = np.tile(SPECIALS, 2)
    return x


def gpu_descramble(om, rx, x, seg_bits, out_stride, off=0, in_place=False, cinit=CINITS):
    """x uint32 [n_seg][stride] -> the output rows uint32 [n_seg][out_stride] (gaps included, as they are after the call)"""
    n_seg, stride = x.shape
    d_c = dev(om, cinit)
    if in_place:
        assert out_stride == stride
        g = Guarded(om, x.nbytes, off).fill(x)
        d_in = g.addr
    else:
        g = Guarded(om, n_seg * out_stride * 4, off)
        src = Guarded(om, x.nbytes, off).fill(x)               # the input at the same offset from its allocation
        d_in = src.addr
    rx.descramble_llr_frames(d_in, n_seg, stride, seg_bits, d_c, g.addr, out_stride)
    if not in_place:
        assert np.array_equal(src.read(np.uint32).reshape(x.shape), x), "the input was written"
    return g.read(np.uint32).reshape(n_seg, out_stride)


def check_descramble(got, x, seg_bits, in_place):
    want = lb.descramble_llr(x.view(np.float32), CINITS, seg_bits).view(np.uint32)
    bad = []
    if not np.array_equal(got[:, :seg_bits], want[:, :seg_bits]):
        d = got[:, :seg_bits] != want[:, :seg_bits]
        bad.append("%d floats differ, the first at %s" % (int(d.sum()), tuple(int(v[0]) for v in np.nonzero(d))))
    gap = got[:, seg_bits:]
    if in_place:
        if not np.array_equal(gap, x[:, seg_bits:seg_bits + gap.shape[1]]):
            bad.append("floats behind seg_bits were touched")
    elif not np.all(gap.view(np.uint8) == POISON):
        bad.append("the gap between two segments' outputs was written")
    return bad


def test_descramble_at_every_path_length_with_strides_and_specials(om, rx0):
    """input stride seg_bits + 5 (odd lengths put the later segments off the 16-byte grid), output stride seg_bits + 9 with the
    gap left poisoned; NaN payloads, +-inf, +-0, subnormals keep every bit but the sign"""
    bad = []
    for n in SEG_BITS:
        x = llr_input(n, n + 5)
        bad += ["seg_bits=%d: %s" % (n, b) for b in check_descramble(gpu_descramble(om, rx0, x, n, n + 9), x, n, False)]
        bad += ["seg_bits=%d in place: %s" % (n, b) for b in check_descramble(gpu_descramble(om, rx0, x, n, n + 5, in_place=True), x, n, True)]
        x = llr_input(n, n, 1)                                 # dense rows: the vector path where n % 4 == 0
        bad += ["seg_bits=%d dense: %s" % (n, b) for b in check_descramble(gpu_descramble(om, rx0, x, n, n), x, n, False)]
    assert not bad, "\n".join(bad)


def test_descramble_at_base_plus_4_bytes_and_twice_is_the_identity(om, rx0):
    bad = []
    for n in (1, 8, 33, 256, 257, CH, SPAN + 1):
        x = llr_input(n, n + 4, 2)
        for in_place in (False, True):
            once = gpu_descramble(om, rx0, x, n, n + 4, off=4, in_place=in_place)
            bad += ["seg_bits=%d base + 4 in_place=%d: %s" % (n, in_place, b) for b in check_descramble(once, x, n, in_place)]
        twice = gpu_descramble(om, rx0, once, n, n + 4, in_place=True)
        if not np.array_equal(twice, x):
            bad.append("seg_bits=%d: descrambling twice is not the identity" % n)
    assert not bad, "\n".join(bad)


def test_one_long_segment_reaches_every_jump_level_below_2_to_the_21(om, tx0, rx0):
    n = 2 ** 21 + 17
    cinit = np.array([0x2468ACE1], np.uint32)
    c = lb.gold(int(cinit[0]), n + 7)
    rng = np.random.default_rng(21)
    x = rng.integers(0, 1 << 32, (1, n), dtype=np.uint64).astype(np.uint32)
    got = gpu_descramble(om, rx0, x, n, n, cinit=cinit)
    assert np.array_equal(got[0], x[0] ^ (c[:n].astype(np.uint32) << np.uint32(31)))
    bits = rng.integers(0, 2, (1, n + 7)).astype(np.uint8)
    assert np.array_equal(gpu_scramble(om, tx0, bits[:, :n], n, False, cinit=cinit)[0], bits[0, :n] ^ c[:n])
    assert np.array_equal(gpu_scramble(om, tx0, pack_msb(bits), n + 7, True, cinit=cinit)[0], pack_msb(bits[0] ^ c))


# ------------------------------------------------------------------------------------------ CRC
CRC_BLOCKS = 67


def crc_as(kind):
    top = lb.CRC_K_MAX - lb.CRC_BITS[kind]
    return tuple(range(8, 129, 8)) + (top - 16, top - 8, top)


@functools.lru_cache(maxsize=None)
def crc_case(kind, A):
    """-> payload [67][A], masks [67] (L bits), info [67][K] per-block masks, info0 [67][K] the scalar mask SCALAR[kind]"""
    rng = np.random.default_rng(100 * A + kind)
    L = lb.CRC_BITS[kind]
    payload = rng.integers(0, 2, (CRC_BLOCKS, A)).astype(np.uint8)
    masks = rng.integers(0, 1 << L, CRC_BLOCKS).astype(np.uint32)
    masks[:2] = (0, (1 << L) - 1)
    plain = lb.crc_attach(payload, kind, 0)
    info = plain.copy()
    info[:, A:] ^= np.array([lb.int_bits(m, L) for m in masks], np.uint8)
    info0 = plain.copy()
    info0[:, A:] ^= lb.int_bits(scalar_mask(kind), L)
    for a in (payload, masks, info, info0):
        a.setflags(write=False)
    return payload, masks, info, info0


def scalar_mask(kind):
    return 0xA5C3F1 & ((1 << lb.CRC_BITS[kind]) - 1)


def gpu_attach(om, tx, payload, kind, mask, pay_packed, info_packed, off=0):
    n, A = payload.shape
    K = A + lb.CRC_BITS[kind]
    src = pack_msb(payload) if pay_packed else (payload | 0xA4)          # junk above bit 0 of the unpacked input
    d_p = dev(om, src)
    d_m = None if np.isscalar(mask) else dev(om, np.asarray(mask, np.uint32) | np.uint32(0xFF000000))
    g = Guarded(om, n * (K // 8 if info_packed else K), off)
    tx.crc_attach_frames(d_p, n, A, kind, g.addr, mask=int(mask) if d_m is None else 0, d_mask=d_m,
                         payload_mode=om.BITS_PACKED if pay_packed else om.BITS_UNPACKED,
                         info_mode=om.BITS_PACKED if info_packed else om.BITS_UNPACKED)
    raw = g.read().reshape(n, -1)
    return np.unpackbits(raw, axis=1, bitorder="big") if info_packed else raw


def gpu_check(om, rx, info, kind, mask, info_packed, pay_packed=False, want=("ok", "syn", "pay"), off=0, in_off=0):
    """-> dict(ok, syn, pay as bits [n][A]); an output that is not in `want` is not passed and asserted untouched"""
    n, K = info.shape
    A = K - lb.CRC_BITS[kind]
    src = Guarded(om, n * (K // 8 if info_packed else K), in_off).fill(pack_msb(info) if info_packed else info | 0xA4)
    d_m = None if np.isscalar(mask) else dev(om, np.asarray(mask, np.uint32) | np.uint32(0xFF000000))
    g = dict(ok=Guarded(om, n), syn=Guarded(om, 4 * n), pay=Guarded(om, n * (A // 8 if pay_packed else A), off))
    rx.crc_check_frames(src.addr, n, A, kind, mask=int(mask) if d_m is None else 0, d_mask=d_m,
                        info_mode=om.BITS_PACKED if info_packed else om.BITS_UNPACKED,
                        d_ok=g["ok"].addr if "ok" in want else None, d_syndrome=g["syn"].addr if "syn" in want else None,
                        d_payload=g["pay"].addr if "pay" in want else None,
                        payload_mode=om.BITS_PACKED if pay_packed else om.BITS_UNPACKED)
    out = {}
    for name, dtype in (("ok", np.uint8), ("syn", np.uint32), ("pay", np.uint8)):
        if name in want:
            out[name] = g[name].read(dtype)
        else:
            assert g[name].untouched(), "%s was not passed and was written" % name
            out[name] = None
    if out["pay"] is not None:
        out["pay"] = out["pay"].reshape(n, -1)
        if pay_packed:
            out["pay"] = np.unpackbits(out["pay"], axis=1, bitorder="big")
    return out


@pytest.mark.parametrize("kind", KINDS, ids=("crc24a", "crc24b", "crc16", "crc8"))
def test_attach_equals_reference_in_every_layout_with_scalar_and_per_block_masks(om, tx0, kind):
    """the 8 high bits set in every device mask are ignored (L <= 24)"""
    bad = []
    for A in crc_as(kind):
        payload, masks, info, info0 = crc_case(kind, A)
        for pay_packed in (False, True):
            for info_packed in (False, True):
                if not np.array_equal(gpu_attach(om, tx0, payload, kind, masks, pay_packed, info_packed), info):
                    bad.append("A=%d payload%d info%d per-block masks" % (A, 8 if pay_packed else 1, 8 if info_packed else 1))
            if not np.array_equal(gpu_attach(om, tx0, payload, kind, scalar_mask(kind), pay_packed, not pay_packed), info0):
                bad.append("A=%d payload%d scalar mask" % (A, 8 if pay_packed else 1))
        if not np.array_equal(gpu_attach(om, tx0, payload, kind, masks, False, False, off=1), info):
            bad.append("A=%d at base + 1" % A)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", KINDS, ids=("crc24a", "crc24b", "crc16", "crc8"))
def test_check_equals_reference_on_clean_and_flipped_blocks(om, rx0, kind):
    """the attached blocks, then the same with ONE bit flipped in every block, at 0, A-1, A and K-1: ok = 0 and the reference's
    syndrome; payload compacted in both layouts"""
    bad = []
    L = lb.CRC_BITS[kind]
    for A in crc_as(kind):
        payload, masks, info, info0 = crc_case(kind, A)
        for info_packed in (False, True):
            out = gpu_check(om, rx0, info, kind, masks, info_packed, pay_packed=info_packed)
            if not (out["ok"].all() and np.array_equal(out["syn"], masks) and np.array_equal(out["pay"], payload)):
                bad.append("A=%d info%d clean" % (A, 8 if info_packed else 1))
            out = gpu_check(om, rx0, info0, kind, scalar_mask(kind), info_packed, pay_packed=not info_packed)
            if not (out["ok"].all() and np.all(out["syn"] == scalar_mask(kind)) and np.array_equal(out["pay"], payload)):
                bad.append("A=%d info%d clean, scalar mask" % (A, 8 if info_packed else 1))
        for pos in (0, A - 1, A, A + L - 1):
            hit = info.copy()
            hit[:, pos] ^= 1
            rok, rsyn, rpay = lb.crc_check(hit, kind, masks)
            assert not rok.any()
            out = gpu_check(om, rx0, hit, kind, masks, pos % 2 == 0)
            if out["ok"].any() or not np.array_equal(out["syn"], rsyn) or not np.array_equal(out["pay"], rpay):
                bad.append("A=%d bit %d flipped" % (A, pos))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind,A", ((lb.CRC16, 24), (lb.CRC24A, 40), (lb.CRC8, 2040)))
def test_each_check_output_alone_and_off_the_word_grid(om, rx0, kind, A):
    payload, masks, info, _ = crc_case(kind, A)
    hit = info.copy()
    hit[::3, 5] ^= 1
    rok, rsyn, rpay = lb.crc_check(hit, kind, masks)
    assert rok.any() and not rok.all()
    for info_packed in (False, True):
        full = gpu_check(om, rx0, hit, kind, masks, info_packed)
        assert np.array_equal(full["ok"], rok) and np.array_equal(full["syn"], rsyn) and np.array_equal(full["pay"], rpay)
        assert np.array_equal(gpu_check(om, rx0, hit, kind, masks, info_packed, want=("ok",))["ok"], rok)
        assert np.array_equal(gpu_check(om, rx0, hit, kind, masks, info_packed, want=("syn",))["syn"], rsyn)
        for pay_packed in (False, True):
            for off in (0, 1):
                alone = gpu_check(om, rx0, hit, kind, masks, info_packed, pay_packed=pay_packed, want=("pay",), off=off, in_off=off)
                assert np.array_equal(alone["pay"], rpay), (info_packed, pay_packed, off)
    rx0.crc_check_frames(dev(om, hit), CRC_BLOCKS, A, kind)                                      # no pointer at all: a no-op


def test_70000_blocks_attach_then_check_with_the_right_and_a_wrong_mask(om, tx0, rx0):
    """A = 24 with CRC16, block n = source payload n mod 16 with a mask of its own: 274 workgroups"""
    n, A, kind = 70000, 24, lb.CRC16
    rng = np.random.default_rng(70000)
    src = rng.integers(0, 2, (16, A)).astype(np.uint8)
    crc16 = np.array([lb.crc(p, kind) for p in src], np.uint32)
    pick = np.arange(n) % 16
    masks = rng.integers(0, 1 << 16, n).astype(np.uint32)
    want = np.concatenate([src[pick], ((crc16[pick] ^ masks)[:, None] >> np.arange(15, -1, -1, dtype=np.uint32)).astype(np.uint8) & 1], axis=1)
    d_info = Guarded(om, n * 40)
    tx0.crc_attach_frames(dev(om, src[pick]), n, A, kind, d_info.addr, d_mask=dev(om, masks))
    assert np.array_equal(d_info.read().reshape(n, 40), want)
    g = dict(ok=Guarded(om, n), syn=Guarded(om, 4 * n))
    rx0.crc_check_frames(d_info.addr, n, A, kind, d_mask=dev(om, masks), d_ok=g["ok"].addr, d_syndrome=g["syn"].addr)
    assert g["ok"].read().all() and np.array_equal(g["syn"].read(np.uint32), masks)
    wrong = masks ^ rng.integers(1, 1 << 16, n).astype(np.uint32)
    rx0.crc_check_frames(d_info.addr, n, A, kind, d_mask=dev(om, wrong), d_ok=g["ok"].addr, d_syndrome=g["syn"].addr)
    assert not g["ok"].read().any()
    assert np.array_equal(g["syn"].read(np.uint32) ^ wrong, masks ^ wrong)


# ------------------------------------------------------------------------------------------ the chain
def gpu_receive(om, rx, llr, cinit, rnti, descramble=True):
    """llr [segs][bps*E] -> bits [n][K], tb_ok int32, crc ok uint8, syndrome: descramble -> decode_rm -> crc check"""
    segs, bps, K, E, A = lb.CHAIN_SEGS, lb.CHAIN_BPS, lb.CHAIN_K, lb.CHAIN_E, lb.CHAIN_A
    n = segs * bps
    g_llr = Guarded(om, llr.nbytes).fill(llr)
    if descramble:
        rx.descramble_llr_frames(g_llr.addr, segs, bps * E, bps * E, dev(om, cinit), g_llr.addr)
    g = dict(bits=Guarded(om, n * K), tb=Guarded(om, 4 * n), ok=Guarded(om, n), syn=Guarded(om, 4 * n))
    rx.tbcc_decode_rm_frames(g_llr.addr, segs, bps * E, bps, K, E, d_bits=g["bits"].addr, d_tb_ok=g["tb"].addr)
    rx.crc_check_frames(g["bits"].addr, n, A, lb.CHAIN_KIND, d_mask=dev(om, rnti), d_ok=g["ok"].addr, d_syndrome=g["syn"].addr)
    g_llr.read()
    return g["bits"].read().reshape(n, K), g["tb"].read(np.int32), g["ok"].read(), g["syn"].read(np.uint32)


def test_chain_crc_catches_what_tb_ok_misses(om, tx0, rx0):
    """152 blocks: payload -> CRC16 ^ RNTI -> encode_rm (K = 40, E = 144) -> scramble on the GPU equal the reference's bits;
    the reference's noisy LLRs -> descramble -> decode_rm -> CRC check equal the reference chain exactly: at least 20 wrongly
    decoded blocks with tb_ok = 1, every one of them with ok = 0.  Without the descrambling at least 140 blocks fail the CRC."""
    c = lb.chain_case()
    segs, bps, K, E, A = lb.CHAIN_SEGS, lb.CHAIN_BPS, lb.CHAIN_K, lb.CHAIN_E, lb.CHAIN_A
    n = segs * bps
    g_info, g_coded = Guarded(om, n * K), Guarded(om, segs * bps * E)
    tx0.crc_attach_frames(dev(om, c["payload"]), n, A, lb.CHAIN_KIND, g_info.addr, d_mask=dev(om, c["rnti"]))
    tx0.tbcc_encode_rm_frames(g_info.addr, segs, bps, K, E, g_coded.addr, bps * E)
    assert np.array_equal(g_coded.read().reshape(segs, bps * E), c["coded"])
    tx0.scramble_frames(g_coded.addr, segs, bps * E, dev(om, c["cinit"]), g_coded.addr)
    assert np.array_equal(g_info.read().reshape(n, K), c["info"])
    assert np.array_equal(g_coded.read().reshape(segs, bps * E), c["tx"])

    rbits, _, rtb, rok, rsyn = lb.chain_reference()
    bits, tb, ok, syn = gpu_receive(om, rx0, c["llr"], c["cinit"], c["rnti"])
    assert np.array_equal(bits, rbits) and np.array_equal(tb, rtb) and np.array_equal(ok, rok) and np.array_equal(syn, rsyn)
    wrong = np.any(bits != c["info"], axis=1)
    assert int((wrong & (tb == 1)).sum()) >= 20
    assert not np.any(ok[wrong]) and np.all(ok[~wrong]) and np.array_equal(syn[~wrong], c["rnti"][~wrong])

    pbits, _, ptb, pok, psyn = lb.chain_reference(descrambled=False)
    assert int((pok == 0).sum()) >= 140
    bits, tb, ok, syn = gpu_receive(om, rx0, c["llr"], c["cinit"], c["rnti"], descramble=False)
    assert np.array_equal(bits, pbits) and np.array_equal(tb, ptb) and np.array_equal(ok, pok) and np.array_equal(syn, psyn)
    assert int((ok == 0).sum()) >= 140


def test_modem_round_trip_every_block_passes_its_crc(om, torch):
    """64-pt QPSK, noise-free: 8 frames of 32 symbols (2880 bits: 19 blocks of E = 144 and filler, all of it scrambled) through
    modulate_frames, the reference taps and demod_frames_soft; descrambled in place, decoded, checked"""
    N, cp, Kd, n_sym = 64, 16, 60, 32
    c = lb.chain_case()
    segs, bps, K, E, A = lb.CHAIN_SEGS, lb.CHAIN_BPS, lb.CHAIN_K, lb.CHAIN_E, lb.CHAIN_A
    n, L = segs * bps, N + cp
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), "QPSK")
    rxe = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 100, 0.7, modulation="QPSK")
    rxe.set_max_trials(0)
    txe.reserve_bitproc()
    rxe.reserve_bitproc()
    seg_bits = txe.bits_per_frame(n_sym)
    assert seg_bits == 2880 and om.tbcc_rm_blocks(seg_bits, K, E) >= bps
    d_rnti, d_cinit = dev(om, c["rnti"]), dev(om, c["cinit"])
    d_info, d_coded = om.DeviceBuffer(n * K), om.DeviceBuffer(segs * seg_bits)
    txe.crc_attach_frames(dev(om, c["payload"]), n, A, lb.CHAIN_KIND, d_info, d_mask=d_rnti)
    txe.tbcc_encode_rm_frames(d_info, segs, bps, K, E, d_coded, seg_bits)
    txe.scramble_frames(d_coded, segs, seg_bits, d_cinit, d_coded)
    sent = d_coded.download(np.uint8, segs * seg_bits).reshape(segs, seg_bits)
    plain = np.zeros((segs, seg_bits), np.uint8)
    plain[:, :bps * E] = c["coded"]
    assert np.array_equal(sent, lb.scramble(plain, c["cinit"]))
    fl_tx, fl = n_sym * L, n_sym * L + cp
    d_tx, d_rx = om.DeviceBuffer(segs * fl_tx * 8), om.DeviceBuffer(segs * fl * 8)
    taps = np.zeros(cp + 1, np.complex64)
    taps[:5] = orc.REF_TAPS / np.linalg.norm(orc.REF_TAPS)
    txe.modulate_frames(d_coded, segs, n_sym, d_tx)
    txe.channel(d_tx, segs, fl_tx, fl_tx, dev(om, taps), len(taps), d_rx, fl, fl)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds * Kd * 2 == seg_bits
    d_eq, d_llr, d_tsr = om.DeviceBuffer(segs * nds * Kd * 8), om.DeviceBuffer(segs * seg_bits * 4), om.DeviceBuffer(segs * 16)
    assert rxe.demod_frames_soft(d_rx, segs, fl, fl, d_eq, d_llr=d_llr, d_tsr=d_tsr) == nds
    rxe.descramble_llr_frames(d_llr, segs, seg_bits, seg_bits, d_cinit, d_llr)
    d_bits, d_ok, d_syn, d_pay = om.DeviceBuffer(n * K), om.DeviceBuffer(n), om.DeviceBuffer(4 * n), om.DeviceBuffer(n * A // 8)
    rxe.tbcc_decode_rm_frames(d_llr, segs, seg_bits, bps, K, E, d_bits=d_bits)
    rxe.crc_check_frames(d_bits, n, A, lb.CHAIN_KIND, d_mask=d_rnti, d_ok=d_ok, d_syndrome=d_syn, d_payload=d_pay,
                         payload_mode=om.BITS_PACKED)
    assert d_ok.download(np.uint8, n).all()
    assert np.array_equal(d_syn.download(np.uint32, n), c["rnti"])
    assert np.array_equal(d_pay.download(np.uint8, n * A // 8).reshape(n, A // 8), pack_msb(c["payload"]))


# ------------------------------------------------------------------------------------------ capture, errors
def test_descramble_and_check_are_capturable_after_reserve(om, torch):
    """handles of their own; one stream, two kernel nodes in a row: no parallel branch"""
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    rx.reserve_bitproc()
    kind, A = lb.CRC24B, 48
    payload, masks, info, _ = crc_case(kind, A)
    n, seg_bits = 3, 5000
    x = llr_input(seg_bits, seg_bits, 3)
    d_x = torch.from_numpy(x.view(np.int32)).cuda()
    d_c = torch.from_numpy(CINITS.view(np.int32)).cuda()
    d_info = torch.from_numpy(info.copy()).cuda()
    d_m = torch.from_numpy(masks.view(np.int32).copy()).cuda()
    d_y = torch.zeros_like(d_x)
    d_ok = torch.zeros(CRC_BLOCKS, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st = torch.cuda.current_stream().cuda_stream
        rx.descramble_llr_frames(d_x, n, seg_bits, seg_bits, d_c, d_y, stream=st)
        rx.crc_check_frames(d_info, CRC_BLOCKS, A, kind, d_mask=d_m, d_ok=d_ok, stream=st)
    assert not d_ok.any() and not d_y.any()                                 # capture enqueues nothing
    want = lb.descramble_llr(x.view(np.float32), CINITS).view(np.int32)
    for _ in range(2):
        d_y.zero_()
        d_ok.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_y.cpu().numpy(), want) and d_ok.cpu().numpy().all()


def test_argument_errors_and_no_ops_leave_poisoned_outputs_untouched(om, rx0, tx0):
    kind, A, n = lb.CRC16, 24, 5
    K = A + 16
    src = dev(om, np.zeros(n * K * 4, np.uint8))
    g = dict(info=Guarded(om, n * K), ok=Guarded(om, n), syn=Guarded(om, 4 * n), pay=Guarded(om, n * A), bits=Guarded(om, 3 * 64),
             llr=Guarded(om, 3 * 64 * 4))
    U, P = om.BITS_UNPACKED, om.BITS_PACKED
    for kw in (dict(kind=4), dict(kind=-1), dict(A=20), dict(A=0), dict(A=2040), dict(mask=1 << 16), dict(n=-1), dict(n=2 ** 31),
               dict(pm=om.BITS_NONE), dict(im=5)):
        a = dict(kind=kind, A=A, n=n, mask=0, pm=U, im=U)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.crc_attach_frames(src, a["n"], a["A"], a["kind"], g["info"].addr, mask=a["mask"], payload_mode=a["pm"], info_mode=a["im"])
        if "im" not in kw:
            with pytest.raises(ValueError):
                rx0.crc_check_frames(src, a["n"], a["A"], a["kind"], mask=a["mask"], info_mode=a["pm"], d_ok=g["ok"].addr,
                                     d_syndrome=g["syn"].addr, d_payload=g["pay"].addr)
    with pytest.raises(ValueError):
        rx0.crc_check_frames(src, n, A, kind, d_payload=g["pay"].addr, payload_mode=om.BITS_NONE)
    tx0.crc_attach_frames(src, 0, A, kind, g["info"].addr)                                       # no-ops
    rx0.crc_check_frames(src, 0, A, kind, d_ok=g["ok"].addr, d_syndrome=g["syn"].addr, d_payload=g["pay"].addr)
    rx0.crc_check_frames(src, n, A, kind)
    tx0.crc_attach_frames(src, n, A, kind, g["info"].addr, mask=1 << 16, d_mask=src)             # the scalar is not in use: fine
    assert np.array_equal(g["info"].read().reshape(n, K), lb.crc_attach(np.zeros((n, A), np.uint8), kind, 0))
    g["info"] = Guarded(om, n * K)
    d_c = dev(om, CINITS)
    for kw in (dict(n_seg=-1), dict(seg_bits=-1), dict(seg_bits=2 ** 31 - 1600), dict(mode=P, seg_bits=60), dict(mode=om.BITS_NONE),
               dict(n_seg=2 ** 41)):
        a = dict(n_seg=3, seg_bits=64, mode=U)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.scramble_frames(src, a["n_seg"], a["seg_bits"], d_c, g["bits"].addr, mode=a["mode"])
    for kw in (dict(n_seg=-1), dict(seg_bits=-1), dict(seg_bits=2 ** 31 - 1600, stride=2 ** 31, out_stride=2 ** 31), dict(stride=63),
               dict(out_stride=63), dict(n_seg=2 ** 41)):
        a = dict(n_seg=3, seg_bits=64, stride=64, out_stride=64)
        a.update(kw)
        with pytest.raises(ValueError):
            rx0.descramble_llr_frames(src, a["n_seg"], a["stride"], a["seg_bits"], d_c, g["llr"].addr, a["out_stride"])
    with pytest.raises(ValueError):
        rx0.descramble_llr_frames(g["llr"].addr, 3, 64, 60, d_c, g["llr"].addr, 62)              # in place at another stride
    tx0.scramble_frames(src, 0, 64, d_c, g["bits"].addr)                                         # no-ops
    tx0.scramble_frames(src, 3, 0, d_c, g["bits"].addr)
    rx0.descramble_llr_frames(src, 0, 64, 64, d_c, g["llr"].addr, 64)
    rx0.descramble_llr_frames(src, 3, 64, 0, d_c, g["llr"].addr, 64)
    assert all(v.untouched() for v in g.values())
