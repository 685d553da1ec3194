"""Host side of the transport-block calls (no GPU): the symbols and their Python wrappers exist, ofdm_tb_geometry and
ofdm_turbo_k_next equal tests/tb_ref.py, ofdm_crc_compute_long -- the kernels' chunk-and-combine routine on the host -- equals
bit-serial long division for every length, and the argument errors that are decided before a handle is looked at."""
import ctypes as C

import numpy as np
import pytest

import lte_bits_ref as lb
import ofdm_mi355x as om
import tb_cases as tc
import tb_ref
from ofdm_mi355x import _lib

NEW = ("ofdm_turbo_k_next", "ofdm_tb_geometry", "ofdm_crc_compute_long", "ofdm_tx_tb_encode_frames", "ofdm_tb_decode_frames",
       "ofdm_tx_reserve_tb", "ofdm_rx_reserve_tb")
INVALID = _lib.OFDM_ERR_INVALID
SEG_FIELDS = ("A", "Z", "B", "L", "C", "K_plus", "K_minus", "C_plus", "C_minus", "F", "soft_floats")
RM_FIELDS = ("G", "q", "gamma", "E0", "E1")


@pytest.fixture(scope="module")
def lib():
    return om.load()


def same(got, want):
    """a tb_geometry dict against tb_ref.geometry's"""
    assert all(got[k] == want[k] for k in SEG_FIELDS), (got, want)
    assert got["n_groups"] == len(want["groups"]) and got["groups"] == want["groups"], (got["groups"], want["groups"])
    if "G" in want:
        assert all(got[k] == want[k] for k in RM_FIELDS), (got, want)
        ncb = dict(zip(want["Ks"], want["Ncbs"]))
        assert got["Ncb_plus"] == ncb[want["K_plus"]]
        assert got["Ncb_minus"] == (ncb[want["K_minus"]] if want["C_minus"] else 0)
    else:
        assert all(got[k] == 0 for k in RM_FIELDS + ("Ncb_minus", "Ncb_plus"))


def test_symbols_prototypes_and_wrappers_exist(lib):
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    for name in ("tb_geometry", "turbo_k_next", "crc_compute_long"):
        assert callable(getattr(om, name))
    for cls, name in ((om.TxEngine, "tb_encode_frames"), (om.TxEngine, "reserve_tb"), (om.RxEngine, "tb_decode_frames"),
                      (om.RxEngine, "reserve_tb")):
        assert callable(getattr(cls, name)), name
    assert C.sizeof(_lib.TbGeom) == 18 * 4 + 3 * 32 + 8 and C.sizeof(_lib.TbOut) == 40


def test_k_next_for_every_argument(lib):
    for bits in range(1, 6201):
        want = tb_ref.k_next(bits)
        assert lib.ofdm_turbo_k_next(bits) == (INVALID if want is None else want), bits
    assert lib.ofdm_turbo_k_next(0) == 40 and lib.ofdm_turbo_k_next(-5) == 40
    assert om.turbo_k_next(6144) == 6144
    with pytest.raises(ValueError):
        om.turbo_k_next(6145)


def test_segmentation_equals_the_reference_over_the_sweep(lib):
    g = _lib.TbGeom()
    for Z in tc.SWEEP_ZS:
        for A in tc.SWEEP_AS:
            same(om.tb_geometry(A, Z), tb_ref.geometry(A, Z))
    for (A, Z) in tc.HAND:
        same(om.tb_geometry(A, Z), tb_ref.geometry(A, Z))
    same(om.tb_geometry(496, 0), tb_ref.geometry(496, 6144))
    same(om.tb_geometry((1 << 20) - 24), tb_ref.geometry((1 << 20) - 24))
    for Z in (40, 48, 56):                                   # small Z: where a K- below 40 would be needed the call refuses
        for A in range(8, 400, 8):
            want = tb_ref.geometry(A, Z)
            if want is None:
                assert lib.ofdm_tb_geometry(A, Z, 0, 1, 0, C.byref(g)) == INVALID, (A, Z)
            else:
                same(om.tb_geometry(A, Z), want)


def test_rate_matching_sizes_equal_the_reference(lib):
    g = _lib.TbGeom()
    for (A, Z) in ((80, 64), (72, 64), (88, 64), (48, 64), (976, 528), (496, 528), (6128, 6144), (75376, 6144)):
        Cn = tb_ref.segmentation(A, Z)["C"]
        for q in tc.QS:
            for Gp in tc.g_sweep(Cn):
                for N_IR in (0, Cn * 3 * 6176, Cn * 2 * 544 + 1, Cn * 2 * 64 + 1, Cn * 3 * 96):
                    want = tb_ref.geometry(A, Z, Gp * q, q, N_IR)
                    if want is None:
                        assert lib.ofdm_tb_geometry(A, Z, Gp * q, q, N_IR, C.byref(g)) == INVALID, (A, Z, Gp, q, N_IR)
                    else:
                        same(om.tb_geometry(A, Z, Gp * q, q, N_IR), want)
    assert om.tb_geometry(80, 64, 602, 1)["n_groups"] == 3


def test_geometry_errors(lib):
    g = _lib.TbGeom()
    for A, Z, G, q, N_IR in ((80, 60, 0, 1, 0), (80, 520, 0, 1, 0), (80, -8, 0, 1, 0), (84, 64, 0, 1, 0), (0, 64, 0, 1, 0), (-8, 64, 0, 1, 0),
                             ((1 << 20) - 16, 0, 0, 1, 0), (32, 40, 0, 1, 0), (80, 64, 2, 1, 0), (80, 64, 600, 7, 0), (80, 64, 600, 0, 0),
                             (80, 64, 600, -1, 0), (80, 64, -600, 1, 0), (80, 64, 1 << 31, 1, 0), (80, 64, 600, 1, -1),
                             (80, 64, 600, 1, 3 * 96 - 1), (80, 64, 16 * 3 * 180 + 3, 1, 0)):
        assert tb_ref.geometry(A, Z, G, q, N_IR) is None
        assert lib.ofdm_tb_geometry(A, Z, G, q, N_IR, C.byref(g)) == INVALID, (A, Z, G, q, N_IR)
        assert b"ofdm_tb_geometry" in lib.ofdm_last_error()
    assert lib.ofdm_tb_geometry(80, 64, 0, 1, 0, None) == INVALID
    assert lib.ofdm_tb_geometry(80, 64, 16 * 3 * 180, 1, 0, C.byref(g)) == 0
    with pytest.raises(ValueError):
        om.tb_geometry(84, 64)


def test_long_crc_equals_long_division_for_every_length(lib):
    """every multiple of 8 in 8 .. 4096 bits for both 24-bit generators: 1 .. 512 bytes over the routine's 256 runs, so runs of
    one and two bytes, empty runs, and a last run that is shorter than the others; the other generators on a few lengths"""
    rng = np.random.default_rng(24)
    bits = rng.integers(0, 2, 4096).astype(np.uint8)
    packed = np.packbits(bits)
    for kind in (lb.CRC24A, lb.CRC24B):
        g, L = lb.CRC_POLY[kind], 24
        reg, want = 0, {}
        for i, b in enumerate(bits):                         # long division, the running remainder of the first i + 1 bits
            reg = (reg << 1) | int(b)
            if reg >> L:
                reg ^= g
            if (i + 1) % 8 == 0:
                tail = reg
                for _ in range(L):                           # times D^L
                    tail <<= 1
                    if tail >> L:
                        tail ^= g
                want[i + 1] = tail
        assert want[4096] == lb.crc(bits, kind) and want[8] == lb.crc(bits[:8], kind)
        for n in range(8, 4097, 8):
            assert om.crc_compute_long(kind, packed, n) == want[n], (kind, n)
    for kind in (lb.CRC16, lb.CRC8):
        for n in (8, 16, 2040, 2048, 2056, 4096):
            assert om.crc_compute_long(kind, packed, n) == lb.crc(bits[:n], kind), (kind, n)
    for n in (8, 24, 2024):                                  # and the short routine where both are defined
        assert om.crc_compute_long(lb.CRC24A, packed, n) == om.crc_compute(lb.CRC24A, packed, n)


def test_long_crc_at_the_largest_transport_block(lib):
    n = (1 << 20) - 24
    bits = np.random.default_rng(25).integers(0, 2, n).astype(np.uint8)
    assert om.crc_compute_long(lb.CRC24A, np.packbits(bits)) == lb.crc(bits, lb.CRC24A)


def test_long_crc_errors(lib):
    crc = C.c_uint32()
    buf = np.zeros(16, np.uint8)
    for kind, n in ((4, 8), (-1, 8), (0, 0), (0, 12), (0, -8), (0, (1 << 30) + 8)):
        assert lib.ofdm_crc_compute_long(kind, _lib.ptr(buf), n, C.byref(crc)) == INVALID, (kind, n)
        assert b"ofdm_crc_compute_long" in lib.ofdm_last_error()
    assert lib.ofdm_crc_compute_long(0, None, 8, C.byref(crc)) == INVALID and lib.ofdm_crc_compute_long(0, _lib.ptr(buf), 8, None) == INVALID
    with pytest.raises(ValueError):
        om.crc_compute_long(0, buf, 136)


def test_null_handles_are_argument_errors(lib):
    U = om.BITS_UNPACKED
    assert lib.ofdm_tx_tb_encode_frames(None, None, U, 1, 80, 64, 600, 1, 0, 19, 42, 7, 16, 0, None, None, U, 600, None) == INVALID
    assert b"ofdm_tx_tb_encode_frames" in lib.ofdm_last_error()
    out = _lib.TbOut()
    assert lib.ofdm_tb_decode_frames(None, None, 1, 600, 80, 64, 600, 1, 0, 19, 42, 7, 16, 0, None, 2, 0, None, 564, C.byref(out), None) == INVALID
    assert b"ofdm_tb_decode_frames" in lib.ofdm_last_error()
    assert lib.ofdm_tx_reserve_tb(None, 1, 80, 64, 600, 1) == INVALID and lib.ofdm_rx_reserve_tb(None, 1, 80, 64) == INVALID
