"""Host side of the turbo rate-matching calls (no GPU): the symbols and their Python wrappers exist, ofdm_turbo_rm_info and
ofdm_turbo_rm_blocks equal tests/turbo_rm_ref.py for every valid K x rv x three Ncb, and the argument errors that are decided
before a handle or the device is looked at."""
import ctypes as C

import pytest

import ofdm_mi355x as om
import turbo_ref as tr
import turbo_rm_cases as rc
import turbo_rm_ref as rm
from ofdm_mi355x import _lib

NEW = ("ofdm_turbo_rm_blocks", "ofdm_turbo_rm_info", "ofdm_tx_turbo_encode_rm_frames", "ofdm_turbo_rate_dematch_frames",
       "ofdm_tx_reserve_turbo_rm", "ofdm_rx_reserve_turbo_rm")
INVALID = _lib.OFDM_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    return om.load()


def test_symbols_prototypes_and_wrappers_exist(lib):
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    for name in ("turbo_rm_blocks", "turbo_rm_info"):
        assert callable(getattr(om, name))
    for cls, name in ((om.TxEngine, "turbo_encode_rm_frames"), (om.TxEngine, "reserve_turbo_rm"), (om.RxEngine, "turbo_rate_dematch_frames"),
                      (om.RxEngine, "reserve_turbo_rm")):
        assert callable(getattr(cls, name)), name


def test_info_equals_the_reference_for_every_k_rv_and_three_ncb(lib):
    k0, na = C.c_int32(), C.c_int32()
    for K in range(tr.K_MIN, tr.K_MAX + 1, 8):
        for Ncb in rc.ncbs(K) + (0,):
            want_na = rm.n_avail(K, Ncb)
            for rv in range(4):
                assert lib.ofdm_turbo_rm_info(K, Ncb, rv, C.byref(k0), C.byref(na)) == 0
                assert (k0.value, na.value) == (rm.k0(K, Ncb, rv), want_na), (K, Ncb, rv)
    assert om.turbo_rm_info(40) == (4, 132) and om.turbo_rm_info(6144, 0, 3) == (14282, 18444)
    assert lib.ofdm_turbo_rm_info(40, 0, 1, None, None) == 0


def test_info_errors(lib):
    k0, na = C.c_int32(), C.c_int32()
    for K, Ncb, rv in ((44, 0, 0), (32, 0, 0), (6152, 0, 0), (40, 63, 0), (40, 193, 0), (40, -1, 0), (40, 0, 4), (40, 0, -1)):
        assert lib.ofdm_turbo_rm_info(K, Ncb, rv, C.byref(k0), C.byref(na)) == INVALID, (K, Ncb, rv)
        assert b"ofdm_turbo_rm_info" in lib.ofdm_last_error()
    with pytest.raises(ValueError):
        om.turbo_rm_info(40, 63)


def test_blocks(lib):
    for K in (40, 64, 1024, 6144):
        for E in (1, K + 1, 3 * K + 12, 16 * (3 * K + 12)):
            for seg_bits in (0, E - 1, E, 10 * E + 3, 10 ** 6):
                assert lib.ofdm_turbo_rm_blocks(seg_bits, K, E) == seg_bits // E == rm.rm_blocks(seg_bits, K, E) == om.turbo_rm_blocks(seg_bits, K, E)
    for K, E in ((44, 100), (40, 0), (40, -3), (40, 16 * 132 + 1)):
        assert lib.ofdm_turbo_rm_blocks(10 ** 6, K, E) == INVALID, (K, E)
    assert lib.ofdm_turbo_rm_blocks(-1, 40, 100) == INVALID
    with pytest.raises(ValueError):
        om.turbo_rm_blocks(1000, 40, 0)


def test_null_handles_are_argument_errors(lib):
    U = om.BITS_UNPACKED
    assert lib.ofdm_tx_turbo_encode_rm_frames(None, None, U, 1, 1, 40, 3, 10, 100, 0, 0, None, None, U, 100, None) == INVALID
    assert b"ofdm_tx_turbo_encode_rm_frames" in lib.ofdm_last_error()
    assert lib.ofdm_turbo_rate_dematch_frames(None, None, 1, 100, 1, 40, 100, 0, 0, None, 0, None, 132, None) == INVALID
    assert b"ofdm_turbo_rate_dematch_frames" in lib.ofdm_last_error()
    assert lib.ofdm_tx_reserve_turbo_rm(None) == INVALID and lib.ofdm_rx_reserve_turbo_rm(None) == INVALID
