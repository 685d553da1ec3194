"""tests/tbcc_rm_ref.py -- the NumPy restatement of the rate-matching contract the GPU is held against -- pinned by means that do
not share its code, the inputs of tests/test_gpu_tbcc_rm.py shown to hold what they are there for, and the host side of the
new entry points (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tbcc_ref
import tbcc_rm_cases as rc
import tbcc_rm_ref as rm
from conftest import ROOT

NEW = ("ofdm_tbcc_rm_blocks", "ofdm_tx_tbcc_encode_rm_frames", "ofdm_tbcc_rate_dematch_frames", "ofdm_tbcc_decode_rm_frames")
NULL = -1


def literal_order(K):
    """TS 36.212 5.1.4.2.1 / 5.1.4.2.2 word for word on index labels: stream j as <NULL> * ND + [3 i + j], written row by row into
    R x 32, columns permuted, read column by column, the three streams concatenated, NULLs skipped -> the label at every rank."""
    R = -(-K // 32)
    ND = 32 * R - K
    w = []
    for j in range(3):
        y = [NULL] * ND + [3 * i + j for i in range(K)]
        mat = [y[32 * r:32 * r + 32] for r in range(R)]
        permuted = [[mat[r][rm.P[c]] for c in range(32)] for r in range(R)]
        w += [permuted[r][c] for c in range(32) for r in range(R)]
    assert len(w) == 96 * R
    return [x for x in w if x != NULL]


def literal_rate_match(e, E):
    """the circular walk itself on one block's coded bits e [3K] (tbcc_ref.encode's order)"""
    K = len(e) // 3
    R = -(-K // 32)
    ND = 32 * R - K
    w = []
    for j in range(3):
        y = [None] * ND + [int(e[3 * i + j]) for i in range(K)]
        w += [y[32 * r + rm.P[c]] for c in range(32) for r in range(R)]
    out, k = [], 0
    while len(out) < E:
        if w[k % len(w)] is not None:
            out.append(w[k % len(w)])
        k += 1
    return np.array(out, np.uint8)


# ------------------------------------------------------------------------------------------ the closed form
def test_closed_form_equals_the_literal_construction_for_every_valid_k():
    assert len(rc.ALL_K) == 254 and all(tbcc_ref.valid_k(K) for K in rc.ALL_K)
    for K in rc.ALL_K:
        lit = np.array(literal_order(K))
        assert lit.shape == (3 * K,)
        i, j = lit // 3, lit % 3
        assert np.array_equal(rm.rank(K, j, i), np.arange(3 * K)), K
        assert np.array_equal(rm.order(K), lit), K


def test_permutation_is_the_bit_reversal_of_c_plus_16():
    for c in range(32):
        x = (c + 16) % 32
        assert rm.P[c] == int("{:05b}".format(x)[::-1], 2)
    assert sorted(rm.P) == list(range(32)) and all(rm.P[rm.P_INV[x]] == x for x in range(32))


def test_e_equal_3k_is_a_bijection_and_the_inverse_round_trips():
    for K in rc.ALL_K:
        q = np.arange(3 * K)
        assert np.array_equal(np.sort(rm.order(K)), q), K
        j, i = rm.inverse(K, q)
        assert j.min() == 0 and j.max() == 2 and i.min() == 0 and i.max() == K - 1
        assert np.array_equal(rm.rank(K, j, i), q), K
        assert np.array_equal(3 * i + j, rm.order(K)), K


@pytest.mark.parametrize("K,E", ((24, 40), (40, 72), (40, 1920), (56, 72), (72, 144), (120, 363), (2048, 3100)))
def test_rate_match_equals_the_circular_walk_that_skips_nulls(K, E):
    rng = np.random.default_rng(K + E)
    c = rng.integers(0, 2, (2, K)).astype(np.uint8)
    e = tbcc_ref.encode(c)
    got = rm.rate_match(e, E)
    for n in range(2):
        assert np.array_equal(got[n], literal_rate_match(e[n], E))
    seg = rm.rm_encode_segments(c.reshape(1, 2, K), E, 2 * E + 9)
    assert np.array_equal(seg[0, :2 * E], got.ravel()) and not seg[0, 2 * E:].any()


def test_dematch_sums_copies_in_increasing_index_in_float32():
    """an independent scalar loop over one block with ten or eleven copies per coded bit: Gaussian values, whose float32 sum
    depends on the order of the additions"""
    K, E = 24, 10 * 72 + 5
    rng = np.random.default_rng(3)
    l = rng.standard_normal(E).astype(np.float32)
    l[5], l[5 + 72], l[7] = np.nan, np.inf, -0.0
    want = np.zeros(3 * K, np.float32)
    order = literal_order(K)
    differs = 0
    for q in range(3 * K):
        acc = None
        back = np.float32(0)
        for idx in range(q, E, 3 * K):
            x = l[idx] if np.isfinite(l[idx]) else np.float32(0)
            acc = x if acc is None else np.float32(acc + x)
        for idx in reversed(range(q, E, 3 * K)):
            back = np.float32(back + (l[idx] if np.isfinite(l[idx]) else np.float32(0)))
        differs += int(acc != back)
        want[order[q]] = acc
    got = rm.dematch(l[None], K)[0]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert differs >= 3, "the order of the additions is to be visible in this input"
    # puncturing: +0 beyond E; a single -0 stays -0
    short = rm.dematch(l[None, :30], K)[0]
    assert np.array_equal(short[order[30:]].view(np.uint32), np.zeros(42, np.uint32))
    assert short[order[7]].view(np.uint32) == np.float32(-0.0).view(np.uint32)


# ------------------------------------------------------------------------------------------ decoding
@pytest.mark.parametrize("K,E,n", rc.NOISELESS, ids=lambda v: str(v))
def test_noiseless_rate_matched_llrs_decode_to_the_information_bits(K, E, n):
    rng = np.random.default_rng(100 + K + E)
    c = rng.integers(0, 2, (n, K)).astype(np.uint8)
    llr = (1.0 - 2.0 * rm.rate_match(tbcc_ref.encode(c), E)).astype(np.float32)
    bits, _, _ = rm.decode_rm(llr, K)
    assert int(np.any(bits != c, axis=1).sum()) == 0


@pytest.mark.parametrize("K,E", rc.PUNCTURED)
def test_punctured_inputs_hold_wrong_blocks_and_failed_tail_biting(K, E):
    llr, c = rc.punctured_blocks(K, E)
    bits, _, ok = rm.decode_rm(llr, K)
    wrong = int(np.any(bits != c, axis=1).sum())
    print("K=%d E=%d at %.1f dB: %d of %d blocks wrong, tb_ok = 0 in %d" % (K, E, rc.PUNCTURED_ESN0_DB, wrong, len(c), int((ok == 0).sum())))
    assert wrong >= 1
    if (K, E) == (64, 72):                                                    # rate 8/9: tail-biting fails as well
        assert int((ok == 0).sum()) >= 4


def test_dematch_inputs_hold_what_they_are_there_for():
    assert {(-(-K // 32), 32 * -(-K // 32) - K) for K in rc.K_SWEEP if K <= 256} == \
        {(R, nd) for R in range(1, 9) for nd in (0, 8, 16, 24) if 32 * R - nd >= 24}
    for K in (24, 40, 136, 2048):
        ref = rc.dm_reference(K)
        assert set(ref) == set(rc.dm_es(K)) and (48 * K in ref) == (K in rc.FULL_KS)
        for E, (llr, c, dem, (bits, metric, ok)) in ref.items():
            assert llr.shape == (8, E) and dem.shape == (8, 3 * K) and bits.shape == (6, K)
            assert np.isnan(llr[3]).any() and np.isinf(llr[3]).any()
            assert np.all(np.isfinite(dem[:4])) and np.all(np.isfinite(metric))
            if E > 3 * K:
                assert np.isinf(dem[4]).any(), "sums that overflow, which the decoder is to take as 0"
                assert np.isinf(dem[6]).any()
            if E == 6 * K + 5:
                assert (dem[6] == 0).any(), "two or three copies: sums that cancel beside sums that overflow"
            if E <= 3 * K:
                assert (dem[5].view(np.uint32) == 0x80000000).any(), "a single -0.0 is to stay -0.0"
                assert (dem[5].view(np.uint32) == 0).sum() == 3 * K - E, "punctured bits are +0"
            if E >= 3 * K - 1:
                assert np.array_equal(bits[:3], c[:3]), (K, E)


# ------------------------------------------------------------------------------------------ host side of the entry points
def _lib_or_skip():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_header_prototypes_and_engines_carry_the_rate_matched_entry_points():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    txt = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.PROTOTYPES, name
    assert callable(ofdm_mi355x.TxEngine.tbcc_encode_rm_frames)
    assert callable(ofdm_mi355x.RxEngine.tbcc_rate_dematch_frames)
    assert callable(ofdm_mi355x.RxEngine.tbcc_decode_rm_frames)
    assert callable(ofdm_mi355x.tbcc_rm_blocks)


def test_library_exports_the_rate_matched_entry_points():
    lib = _lib_or_skip()
    for name in NEW:
        assert hasattr(lib, name), name


def test_rate_matched_calls_reject_a_null_handle_a_bad_k_and_a_bad_e_without_a_device():
    from ofdm_mi355x import _lib
    lib = _lib_or_skip()
    out = _lib.TbccOut(None, _lib.BITS_UNPACKED, None, None)
    assert lib.ofdm_tx_tbcc_encode_rm_frames(None, None, 2, 1, 1, 40, 72, None, 2, 72, None) == _lib.OFDM_ERR_INVALID
    assert b"null handle" in lib.ofdm_last_error()
    assert lib.ofdm_tbcc_rate_dematch_frames(None, None, 1, 72, 1, 40, 72, None, 120, None) == _lib.OFDM_ERR_INVALID
    assert b"null handle" in lib.ofdm_last_error()
    assert lib.ofdm_tbcc_decode_rm_frames(None, None, 1, 72, 1, 40, 72, C.byref(out), None) == _lib.OFDM_ERR_INVALID
    assert b"null handle" in lib.ofdm_last_error()
    for K, E in ((44, 72), (16, 72), (2056, 72), (40, 0), (40, 48 * 40 + 1), (40, -1)):     # the check all four calls share
        assert lib.ofdm_tbcc_rm_blocks(10 ** 6, K, E) == _lib.OFDM_ERR_INVALID, (K, E)
        assert (b"E must lie" if K == 40 else b"K must be") in lib.ofdm_last_error()
    assert lib.ofdm_tbcc_rm_blocks(-1, 40, 72) == _lib.OFDM_ERR_INVALID
    assert lib.ofdm_tbcc_rm_blocks(10 ** 6, 40, 48 * 40) == 10 ** 6 // 1920


def test_c_rate_matched_block_count_equals_the_python_rule():
    import ofdm_mi355x
    lib = _lib_or_skip()
    for K in (24, 40, 256, 2048):
        for E in (1, K + 1, 3 * K, 72, 1920, 48 * K):
            if not rm.valid_e(K, E):
                continue
            for seg_bits in (0, 1, E - 1, E, E + 1, 115200, 2 ** 33 + 5):
                assert lib.ofdm_tbcc_rm_blocks(seg_bits, K, E) == seg_bits // E == rm.rm_blocks(seg_bits, K, E)
                assert ofdm_mi355x.tbcc_rm_blocks(seg_bits, K, E) == seg_bits // E
    with pytest.raises(ValueError):
        ofdm_mi355x.tbcc_rm_blocks(1000, 40, 0)
    with pytest.raises(ValueError):
        ofdm_mi355x.tbcc_rm_blocks(1000, 40, 1921)
