"""The turbo codec's C ABI without a GPU: the library exports the new calls, the two host-only calls equal the Python rules of
tests/turbo_ref.py over a sweep, and the compute calls fail loudly (no CPU path)."""
import ctypes as C
import os

import pytest

import turbo_cases as tc
import turbo_ref as tr

NEW = ("ofdm_turbo_blocks", "ofdm_turbo_qpp_check", "ofdm_tx_turbo_encode_frames", "ofdm_rx_reserve_turbo", "ofdm_turbo_decode_frames")


@pytest.fixture(scope="module")
def lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_library_and_package_export_the_turbo_calls(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    for name in ("turbo_blocks", "turbo_qpp_check"):
        assert callable(getattr(om, name))
    for cls, name in ((om.TxEngine, "turbo_encode_frames"), (om.RxEngine, "reserve_turbo"), (om.RxEngine, "turbo_decode_frames")):
        assert callable(getattr(cls, name))
    assert [f[0] for f in _lib.TurboOut._fields_] == ["bits", "bits_mode", "llr"]


def test_block_count_equals_the_python_rule(lib):
    import ofdm_mi355x as om
    for K in (40, 48, 1024, 6144):
        for seg_bits in (0, 1, 3 * K + 11, 3 * K + 12, 3 * K + 13, 7 * (3 * K + 12) - 1, 7 * (3 * K + 12), 10 ** 12):
            assert lib.ofdm_turbo_blocks(seg_bits, K) == tr.blocks(seg_bits, K) == om.turbo_blocks(seg_bits, K)
    for K in (32, 44, 36, 6152, 0, -8):
        assert lib.ofdm_turbo_blocks(1000, K) < 0
        with pytest.raises(ValueError):
            om.turbo_blocks(1000, K)
    assert lib.ofdm_turbo_blocks(-1, 40) < 0


def test_qpp_check_equals_the_python_rule(lib):
    import ofdm_mi355x as om
    for K, (f1, f2) in tc.QPP.items():
        assert lib.ofdm_turbo_qpp_check(K, f1, f2) == 0 and om.turbo_qpp_check(K, f1, f2)
    assert lib.ofdm_turbo_qpp_check(*tc.IDENTITY) == 0
    for bad in ((40, 2, 10), (44, 3, 10), (32, 3, 8), (6152, 3, 10), (40, 40, 0), (40, 3, 40), (40, -1, 0), (40, 3, -1), (40, 0, 0)):
        assert lib.ofdm_turbo_qpp_check(*bad) != 0 and not tr.qpp_check(*bad), bad
        assert not om.turbo_qpp_check(*bad)
    for K in (40, 48, 72, 120):                              # every pair at a few K: the C rule is the Python rule
        for f1 in range(K):
            for f2 in range(0, K, 1 if K <= 48 else 5):
                assert (lib.ofdm_turbo_qpp_check(K, f1, f2) == 0) == tr.qpp_check(K, f1, f2), (K, f1, f2)
    for f1, f2 in ((263, 480), (1, 0), (2, 0), (6143, 6143), (3, 96), (5, 3072)):
        assert (lib.ofdm_turbo_qpp_check(6144, f1, f2) == 0) == tr.qpp_check(6144, f1, f2), (f1, f2)


def test_compute_calls_fail_loudly_without_a_handle(lib):
    """No device is needed to get here: a NULL handle is refused before anything else, with a text that names the call."""
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    out = _lib.TurboOut(None, om.BITS_UNPACKED, None)
    assert lib.ofdm_tx_turbo_encode_frames(None, None, om.BITS_UNPACKED, 1, 1, 40, 3, 10, None, om.BITS_UNPACKED, 132, None) != 0
    assert b"ofdm_tx_turbo_encode_frames" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_turbo(None, 8, 40) != 0
    assert b"ofdm_rx_reserve_turbo" in lib.ofdm_last_error()
    assert lib.ofdm_turbo_decode_frames(None, None, 1, 132, 1, 40, 3, 10, 1, C.byref(out), None) != 0
    assert b"ofdm_turbo_decode_frames" in lib.ofdm_last_error()


def test_no_engine_without_a_device():
    import torch
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(om.OfdmError):
        om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100).reserve_turbo(8, 40)
