"""tests/tbcc_ref.py -- the NumPy restatement of the TBCC contract the GPU is held against -- pinned by means that do not share
its code, and the host side of the new entry points (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tbcc_ref
from conftest import ROOT

KS = (24, 40, 96, 256, 1024, 2048)
NEW = ("ofdm_tbcc_blocks", "ofdm_tx_tbcc_encode_frames", "ofdm_rx_reserve_tbcc", "ofdm_tbcc_decode_frames")


def _poly_encode(c):
    """Second formulation: dj = c (*) gj, a circular polynomial product mod 2, written as a K x K circulant matrix product."""
    K = c.shape[-1]
    out = np.zeros(c.shape[:-1] + (K, 3), np.uint8)
    for j, taps in enumerate(((0, 2, 3, 5, 6), (0, 1, 2, 3, 6), (0, 1, 2, 4, 6))):
        g = np.zeros(K, np.int64)
        g[list(taps)] = 1
        idx = (np.arange(K)[:, None] - np.arange(K)[None, :]) % K             # full[k] = sum_m c[m] g[(k - m) mod K]
        out[..., j] = (c.astype(np.int64) @ g[idx].T) & 1
    return out.reshape(c.shape[:-1] + (3 * K,))


# ------------------------------------------------------------------------------------------ encoder, noiseless decoding
@pytest.mark.parametrize("K", KS)
def test_encoder_equals_the_circular_polynomial_product(K):
    rng = np.random.default_rng(K)
    c = rng.integers(0, 2, (5, K)).astype(np.uint8)
    assert np.array_equal(tbcc_ref.encode(c), _poly_encode(c))


@pytest.mark.parametrize("K", (24, 40, 256))
def test_encoder_is_linear_shift_covariant_and_has_the_known_weights(K):
    rng = np.random.default_rng(7 + K)
    a = rng.integers(0, 2, (4, K)).astype(np.uint8)
    b = rng.integers(0, 2, (4, K)).astype(np.uint8)
    assert np.array_equal(tbcc_ref.encode(a ^ b), tbcc_ref.encode(a) ^ tbcc_ref.encode(b))
    assert np.array_equal(tbcc_ref.encode(np.roll(a, 1, axis=-1)), np.roll(tbcc_ref.encode(a), 3, axis=-1))
    assert not tbcc_ref.encode(np.zeros((1, K), np.uint8)).any()
    one = np.zeros((1, K), np.uint8)
    one[0, K // 3] = 1
    assert int(tbcc_ref.encode(one).sum()) == 15                              # 5 taps in each of the three generators


@pytest.mark.parametrize("K", KS)
def test_noiseless_llrs_decode_to_the_information_bits(K):
    rng = np.random.default_rng(100 + K)
    c = rng.integers(0, 2, (3, K)).astype(np.uint8)
    llr = (1.0 - 2.0 * tbcc_ref.encode(c)).astype(np.float32)
    bits, metric, ok = tbcc_ref.decode(llr)
    assert np.array_equal(bits, c)
    assert np.all(ok == 1)
    assert np.array_equal(metric, np.full(3, 3 * (K + 192), np.float32))      # 3 per step over T = K + 192 steps, exact in fp32


def test_all_zero_llrs_decode_to_all_zero_bits_by_the_tie_rules():
    bits, metric, ok = tbcc_ref.decode(np.zeros((2, 3 * 40), np.float32))
    assert not bits.any() and np.all(metric == 0) and np.all(ok == 1)
    bad = np.full((1, 3 * 40), np.nan, np.float32)
    bad[0, ::2] = np.inf
    bad[0, 1::4] = -np.inf
    bits, metric, ok = tbcc_ref.decode(bad)                                   # not finite counts as 0
    assert not bits.any() and np.all(metric == 0) and np.all(ok == 1)


# ------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("K,n_blocks", ((40, 400), (256, 200), (1024, 50)))
def test_awgn_blocks_decode_without_error_at_2_db_and_at_0_db(K, n_blocks):
    """Seed 1, Es/N0 of the coded BPSK symbols.  Measured with this file's reference: raw BER 3.6-3.9 % at 2 dB, 0 block errors
    at 2 dB and at 0 dB for all three K."""
    for esn0 in (2.0, 0.0):
        rng = np.random.default_rng(1)
        c = rng.integers(0, 2, (n_blocks, K)).astype(np.uint8)
        e = tbcc_ref.encode(c)
        llr = tbcc_ref.awgn_llrs(e, esn0, rng)
        raw = float(np.mean((llr < 0).astype(np.uint8) != e))
        bits, _, _ = tbcc_ref.decode(llr)
        wrong = int(np.sum(np.any(bits != c, axis=1)))
        print("K=%d Es/N0=%.1f dB: raw BER %.4f, block errors %d / %d" % (K, esn0, raw, wrong, n_blocks))
        if esn0 == 2.0:
            assert raw >= 0.03
        assert wrong == 0


# ------------------------------------------------------------------------------------------ host side of the entry points
def _lib_or_skip():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_header_prototypes_and_engines_carry_the_new_entry_points():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    txt = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES, name
    assert "ofdm_tbcc_out" in code and "5.1.4.2" in txt
    assert [f[0] for f in _lib.TbccOut._fields_] == ["bits", "bits_mode", "metric", "tb_ok"]
    assert callable(ofdm_mi355x.TxEngine.tbcc_encode_frames)
    assert callable(ofdm_mi355x.RxEngine.reserve_tbcc)
    assert callable(ofdm_mi355x.RxEngine.tbcc_decode_frames)
    assert callable(ofdm_mi355x.tbcc_blocks)


def test_new_calls_reject_a_null_handle_and_a_bad_k_without_a_device():
    from ofdm_mi355x import _lib
    lib = _lib_or_skip()
    out = _lib.TbccOut(None, _lib.BITS_UNPACKED, None, None)
    assert lib.ofdm_tx_tbcc_encode_frames(None, None, 2, 1, 1, 40, None, 2, 120, None) == _lib.OFDM_ERR_INVALID
    assert lib.ofdm_rx_reserve_tbcc(None, 1, 40) == _lib.OFDM_ERR_INVALID
    assert lib.ofdm_tbcc_decode_frames(None, None, 1, 120, 1, 40, C.byref(out), None) == _lib.OFDM_ERR_INVALID
    assert b"null handle" in lib.ofdm_last_error()
    for K in (0, 16, 25, 44, 2056, -8):
        assert lib.ofdm_tbcc_blocks(10000, K) == _lib.OFDM_ERR_INVALID
    assert lib.ofdm_tbcc_blocks(-1, 40) == _lib.OFDM_ERR_INVALID


def test_c_block_count_equals_the_python_rule():
    import ofdm_mi355x
    lib = _lib_or_skip()
    for K in (24, 40, 96, 256, 1024, 2048):
        for seg_bits in (0, 1, 3 * K - 1, 3 * K, 3 * K + 1, 115200, 1200 * 4 * 180, 2 ** 33 + 5):
            assert lib.ofdm_tbcc_blocks(seg_bits, K) == seg_bits // (3 * K) == tbcc_ref.blocks(seg_bits, K)
            assert ofdm_mi355x.tbcc_blocks(seg_bits, K) == seg_bits // (3 * K)
    with pytest.raises(ValueError):
        ofdm_mi355x.tbcc_blocks(1000, 20)
