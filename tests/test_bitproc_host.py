"""The host side of csrc/bitproc.hip without a GPU: ofdm_crc_bits, ofdm_crc_compute (the kernels' remainder routine) and
ofdm_gold_bits (the kernels' jump tables, up to the top of the index range) against tests/lte_bits_ref.py, and the argument
checks that need no device.  Needs the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import lte_bits_ref as lb

KINDS = (lb.CRC24A, lb.CRC24B, lb.CRC16, lb.CRC8)
CINITS = (0, 1, 0x12345, 0x7FFFFFFF)
CH = 1024                                                    # GOLD_CH of csrc/ofdm_launch.hpp: the bits behind one jump
TOP = 2 ** 31 - 1600


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    ofdm_mi355x.load()
    return ofdm_mi355x


def test_crc_bits_and_constants(om):
    assert (om.CRC24A, om.CRC24B, om.CRC16, om.CRC8) == KINDS
    assert [om.crc_bits(k) for k in KINDS] == [24, 24, 16, 8]
    for kind in (-1, 4, 99):
        with pytest.raises(ValueError):
            om.crc_bits(kind)


def test_crc_compute_equals_the_reference(om):
    rng = np.random.default_rng(3)
    msg = np.frombuffer(b"123456789", np.uint8)
    for kind in KINDS:
        assert om.crc_compute(kind, msg) == lb.crc(np.unpackbits(msg), kind)
        for A in (8, 24, 72, 2024):
            for _ in range(3):
                bits = rng.integers(0, 2, A).astype(np.uint8)
                assert om.crc_compute(kind, np.packbits(bits), A) == lb.crc(bits, kind), (kind, A)


def test_gold_bits_equal_the_stepped_reference(om):
    firsts = (0, 1, 31, 32, 1599, 1600, CH - 1, CH, CH + 1, 2 ** 20 + 5)
    for c_init in CINITS:
        ref = lb.gold(c_init, max(firsts) + 200)
        for first in firsts:
            assert np.array_equal(om.gold_bits(c_init, first, 200), ref[first:first + 200]), (hex(c_init), first)
    assert np.array_equal(om.gold_bits(0xFFFFFFFF, 77, 100), lb.gold(0x7FFFFFFF, 177)[77:])      # bit 31 is ignored
    assert om.gold_bits(5, 10, 0).size == 0


def _lfsr_state_at(taps, state, n):
    """state of the LFSR x(m + 31) = XOR of x(m + t), t in taps, after n steps, by square-and-multiply on the 31 x 31 step
    matrix over GF(2) kept as Python integers (row r = the mask of the state bits that make new bit r): nothing of the library's"""
    rows = [1 << (r + 1) for r in range(30)] + [sum(1 << t for t in taps)]

    def mul(a, b):                                           # (a b) v = a (b v)
        out = []
        for r in range(31):
            acc = 0
            for k in range(31):
                if (a[r] >> k) & 1:
                    acc ^= b[k]
            out.append(acc)
        return out

    result = [1 << r for r in range(31)]
    while n:
        if n & 1:
            result = mul(rows, result)
        rows = mul(rows, rows)
        n >>= 1
    return sum((bin(result[r] & state).count("1") & 1) << r for r in range(31))


def _gold_from(first, c_init, n):
    s1 = _lfsr_state_at((0, 3), 1, first + 1600)
    s2 = _lfsr_state_at((0, 1, 2, 3), c_init & 0x7FFFFFFF, first + 1600)
    out = np.empty(n, np.uint8)
    for i in range(n):
        out[i] = (s1 ^ s2) & 1
        s1 = (s1 >> 1) | (((s1 ^ (s1 >> 3)) & 1) << 30)
        s2 = (s2 >> 1) | (((s2 ^ (s2 >> 1) ^ (s2 >> 2) ^ (s2 >> 3)) & 1) << 30)
    return out


def test_gold_bits_at_the_top_of_the_index_range(om):
    assert np.array_equal(_gold_from(12345, 0x12345, 300), lb.gold(0x12345, 12645)[12345:])      # the helper itself
    for c_init in CINITS:
        for first in (TOP - 200, TOP - 200 - CH - 3, 2 ** 30 + 2 ** 29 - 100):
            assert np.array_equal(om.gold_bits(c_init, first, 200), _gold_from(first, c_init, 200)), (hex(c_init), first)


def test_gold_bits_across_a_split(om):
    for c_init in CINITS:
        for first, n in ((0, 200), (CH - 50, 100), (64 * CH - 33, 67), (2 ** 20 + 5, 2 * CH + 9), (TOP - 300, 300)):
            whole = om.gold_bits(c_init, first, n)
            h = n // 2
            assert np.array_equal(whole, np.concatenate([om.gold_bits(c_init, first, h), om.gold_bits(c_init, first + h, n - h)]))


def test_argument_errors(om):
    lib = om.load()
    INVALID = -1
    buf = np.zeros(256, np.uint8)
    crc = C.c_uint32(0)
    p = C.c_void_p(buf.ctypes.data)
    for kind, A in ((-1, 24), (4, 24), (lb.CRC16, 12), (lb.CRC16, 0), (lb.CRC16, -8), (lb.CRC16, 2040), (lb.CRC24A, 2032),
                    (lb.CRC8, 2048)):
        assert lib.ofdm_crc_compute(kind, p, A, C.byref(crc)) == INVALID, (kind, A)
    assert lib.ofdm_crc_compute(lb.CRC8, p, 2040, C.byref(crc)) == 0                             # K = 2048 exactly
    assert lib.ofdm_crc_compute(lb.CRC16, None, 24, C.byref(crc)) == INVALID
    assert lib.ofdm_crc_bits(7) == INVALID
    out = np.zeros(16, np.uint8)
    po = C.c_void_p(out.ctypes.data)
    for first, n in ((-1, 4), (0, -1), (TOP, 1), (TOP - 3, 4), (2 ** 40, 1), (0, 2 ** 40)):
        assert lib.ofdm_gold_bits(1, first, n, po) == INVALID, (first, n)
    assert lib.ofdm_gold_bits(1, TOP - 4, 4, po) == 0
    assert lib.ofdm_gold_bits(1, 0, 4, None) == INVALID
    # the device calls check their arguments before they look at the handle, so the texts can be read without a device
    def attach(kind=lb.CRC16, A=24, n=4, mask=0, pm=om.BITS_UNPACKED, im=om.BITS_UNPACKED):
        rc = lib.ofdm_tx_crc_attach_frames(None, p, pm, n, A, kind, mask, None, p, im, None)
        return rc, lib.ofdm_last_error().decode()

    def check(kind=lb.CRC16, A=24, n=4, mask=0):
        rc = lib.ofdm_crc_check_frames(None, p, om.BITS_UNPACKED, n, A, kind, mask, None, None, None)
        return rc, lib.ofdm_last_error().decode()

    for call in (attach, check):
        for kw, text in ((dict(kind=9), "kind"), (dict(A=20), "multiple of 8"), (dict(A=2040), "2048"), (dict(mask=1 << 16), "mask"),
                         (dict(kind=lb.CRC8, mask=0x100), "mask"), (dict(n=-1), "negative"), (dict(), "null handle")):
            rc, msg = call(**kw)
            assert rc == INVALID and text in msg, (call.__name__, kw, msg)
    assert attach(pm=om.BITS_NONE)[0] == INVALID and "bit modes" in attach(pm=om.BITS_NONE)[1]
    for kw, text in ((dict(n_seg=-1), "negative"), (dict(seg_bits=-1), "negative"), (dict(seg_bits=TOP), "2^31"),
                     (dict(mode=om.BITS_PACKED, seg_bits=12), "% 8"), (dict(mode=om.BITS_NONE), "mode"), (dict(), "null handle")):
        a = dict(n_seg=2, seg_bits=64, mode=om.BITS_UNPACKED)
        a.update(kw)
        assert lib.ofdm_tx_scramble_frames(None, p, a["mode"], a["n_seg"], a["seg_bits"], p, p, None) == INVALID
        assert text in lib.ofdm_last_error().decode(), kw
    for kw, text in ((dict(n_seg=-1), "negative"), (dict(seg_bits=TOP, stride=TOP), "2^31"), (dict(stride=63), "stride"),
                     (dict(out_stride=63), "stride"), (dict(out_stride=65), "in place"), (dict(), "null handle")):
        a = dict(n_seg=2, seg_bits=64, stride=64, out_stride=64)
        a.update(kw)
        assert lib.ofdm_descramble_llr_frames(None, p, a["n_seg"], a["stride"], a["seg_bits"], p, p, a["out_stride"], None) == INVALID
        assert text in lib.ofdm_last_error().decode(), kw
