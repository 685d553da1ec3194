"""tests/tbcc_ref.py -- the NumPy restatement of the TBCC contract the GPU is held against -- pinned by means that do not share
its code, and the host side of the new entry points (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tbcc_cases as tc
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


# ------------------------------------------------------------------------------------------ inputs of the GPU edge tests
# tests/test_gpu_tbcc_edges.py compares the kernels with tbcc_ref on the arrays of tests/tbcc_cases.py.  These tests show, on the
# reference alone, that those arrays reach the paths they are there for, so that the comparison cannot pass without them.
def test_edge_sweep_covers_every_tile_remainder_and_has_marginal_decisions():
    assert len(tc.K_SWEEP) == 38 and all(tbcc_ref.valid_k(K) for K in tc.K_SWEEP)
    assert {K % 64 for K in tc.K_SWEEP if K <= 256} == {K % 64 for K in tc.K_SWEEP if K >= 1992} == set(range(0, 64, 8))
    assert set(range(24, 96, 8)) <= set(tc.K_SWEEP)                           # every K whose warm-up wraps more than once
    wrong_total = 0
    for K in tc.K_SWEEP:
        llr, c, (bits, metric, ok) = tc.sweep_reference(K)
        assert llr.shape == (8, 3 * K) and llr.dtype == np.float32
        assert np.all(llr[4:7] == np.round(llr[4:7])) and np.abs(llr[4:6]).max() == 1 and np.abs(llr[6]).max() == 2
        assert np.array_equal(bits[7], c[7]) and ok[7] == 1 and metric[7] == np.float32(3 * (K + 192))
        wrong_total += int(np.any(bits[tc.SWEEP_AWGN] != c[tc.SWEEP_AWGN], axis=1).sum())
    print("AWGN blocks of the sweep that decode wrongly: %d of %d" % (wrong_total, 4 * len(tc.K_SWEEP)))
    assert wrong_total >= 1


@pytest.mark.parametrize("lo,hi", tc.TIE_RANGES, ids=("pm1", "pm2"))
@pytest.mark.parametrize("K", tc.TIE_KS)
def test_edge_tie_inputs_hold_ties_failed_tail_biting_and_end_states_other_than_0(K, lo, hi):
    llr = tc.tie_blocks(K, lo, hi)
    assert llr.shape == (64, 3 * K) and llr.min() == lo and llr.max() == hi - 1
    _, metric, ok = tbcc_ref.decode(llr)
    st = tc.forward_stats(llr)
    assert np.array_equal(st["metric"], metric)                               # the recount is the reference's recursion
    n_fail = int((ok == 0).sum())
    n_end = int((st["end_tied"] & (st["end_state"] != 0)).sum())
    n_ties = int(st["ties"].sum())
    print("K=%d [%d, %d): tb_ok = 0 in %d blocks, tied end states %d (%d not won by state 0), decision ties %d" % (
        K, lo, hi, n_fail, int(st["end_tied"].sum()), n_end, n_ties))
    assert n_fail >= 3
    assert n_end >= 20
    assert n_ties >= 10000


def test_edge_scale_inputs_keep_bits_and_scale_the_metric_down_to_subnormals():
    llr, _ = tc.scale_blocks()
    assert llr.shape == (16, 360)
    b0, m0, ok0 = tbcc_ref.decode(llr)
    tiny = np.finfo(np.float32).tiny
    for e in tc.SCALE_EXPONENTS:
        x = tc.scaled(llr, e)
        assert x.dtype == np.float32 and np.all(np.isfinite(x))
        b, m, ok = tbcc_ref.decode(x)
        assert np.array_equal(b, b0) and np.array_equal(ok, ok0), e
        if e == -140:
            # |llr| < 2^5 puts every product below 2^-126; the few with |llr| < 2^-10 round to 0 (P(|4y| < 2^-10) ~ 1e-4)
            assert np.all(np.abs(x) < tiny) and np.count_nonzero(x) >= 0.99 * x.size, "every input is to be subnormal"
            assert np.all(m != 0) and np.all(np.abs(m) < tiny)
        else:
            assert np.array_equal(m, np.ldexp(m0, e).astype(np.float32)) and np.all(np.isfinite(m)), e
    x = tc.scaled(llr, -126)                                                  # normal and subnormal inputs side by side
    assert 0 < int((np.abs(x) < tiny).sum()) < x.size


def test_edge_output_grid_and_encoder_inputs_have_the_stated_shapes():
    for K in tc.OUTPUT_KS:
        seg = tc.output_segments(K)
        assert seg.shape == (2, 5 * 3 * K + 7) and np.isnan(seg[:, 5 * 3 * K:]).all() and np.isfinite(seg[:, :5 * 3 * K]).all()
        assert seg.shape[1] % 2 == 1                                          # a stride that moves every second segment off 8 bytes
    src = tc.grid_source()
    _, _, ok = tbcc_ref.decode(src)
    assert 0 < int(ok.sum()) < 16, "the tiled blocks are to hold both values of tb_ok"
    seg = tc.grid_segments(src)
    assert seg.shape == (7000, 725) and 7000 * 10 > 65535
    flat = seg[:, :720].reshape(70000, 72)
    assert np.array_equal(flat[16 * 4000 + 5], src[5]) and np.array_equal(flat[69999], src[69999 % 16])
    for K in (24, 2048):
        imp = tc.impulse_info(K)
        assert imp.shape == (2, 3, K) and np.all(imp.sum(axis=2) == 1)
        assert [int(np.argmax(r)) for r in imp.reshape(6, K)] == [0, 1, 5, 6, K - 6, K - 1]
        assert np.all(tbcc_ref.encode(imp).sum(axis=2) == 15)


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
