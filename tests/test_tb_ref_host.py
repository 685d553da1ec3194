"""Pins tests/tb_ref.py (the yardstick of the transport-block kernels) by means that do not share its code (no GPU): segmentations
derived by hand, divisibility of every block by its generator in Python-integer polynomial arithmetic, the counting identities of
TS 36.212 5.1.2 and 5.1.4.1.2, the linearity identity the kernels' chunk-and-combine CRC rests on, noiseless round trips, and
the operating point of the device HARQ chain."""
import numpy as np
import pytest

import lte_bits_ref as lb
import tb_cases as tc
import tb_ref

G24A, G24B = 0x1864CFB, 0x1800063


def gf2_mod(n, g):
    """remainder of the polynomial n (a Python integer, bit i = the coefficient of x^i) divided by g"""
    lg = g.bit_length()
    while n.bit_length() >= lg:
        n ^= g << (n.bit_length() - lg)
    return n


def as_int(bits):
    return int.from_bytes(np.packbits(np.concatenate([np.zeros((-len(bits)) % 8, np.uint8), np.asarray(bits, np.uint8)])).tobytes(), "big")


def test_valid_k_list_and_k_next():
    assert len(tb_ref.LTE_KS) == 188 and tb_ref.LTE_KS[0] == 40 and tb_ref.LTE_KS[-1] == 6144
    assert all(K % 8 == 0 for K in tb_ref.LTE_KS) and list(tb_ref.LTE_KS) == sorted(set(tb_ref.LTE_KS))
    assert [tb_ref.k_next(b) for b in (1, 40, 41, 512, 513, 1024, 1025, 2048, 2049, 6144, 6145)] == \
        [40, 40, 48, 512, 528, 1024, 1056, 2048, 2112, 6144, None]


@pytest.mark.parametrize("A,Z", sorted(tc.HAND))
def test_hand_derived_segmentations(A, Z):
    g = tb_ref.segmentation(A, Z)
    got = (g["C"], g["K_minus"], g["C_minus"], g["K_plus"], g["C_plus"], g["F"], g["L"])
    assert got == tc.HAND[(A, Z)]
    assert g["Ks"] == [g["K_minus"]] * g["C_minus"] + [g["K_plus"]] * g["C_plus"]


def test_refused_geometries():
    assert tb_ref.segmentation(80, 60) is None and tb_ref.segmentation(80, 520) is None          # Z is no valid K
    assert tb_ref.segmentation(84, 64) is None and tb_ref.segmentation(0, 64) is None
    assert tb_ref.segmentation((1 << 20) - 16, 0) is None and tb_ref.segmentation((1 << 20) - 24, 0) is not None
    # Z = 40: K+ = 40 for every A; B' = 40 C exactly only when B is a multiple of 16, otherwise a K- below 40 would be needed
    assert tb_ref.segmentation(24, 40)["C_minus"] == 0 and tb_ref.segmentation(32, 40) is None
    g = tb_ref.geometry(80, 64, 3 * 200, 1)
    assert g["Es"] == [200, 200, 200]
    assert tb_ref.geometry(80, 64, 2, 1) is None                                                  # E0 = 0
    assert tb_ref.geometry(80, 64, 600, 7) is None and tb_ref.geometry(80, 64, 600, 0) is None
    assert tb_ref.geometry(80, 64, 600, 1, N_IR=3 * 96 - 1) is None                              # Ncb < Kpi = 96 of K = 64
    assert tb_ref.geometry(80, 64, 600, 1, N_IR=3 * 96)["Ncbs"] == [96, 96, 96]                  # Kw = 192, 192, 288 without it
    assert tb_ref.geometry(80, 64, 600, 1)["Ncbs"] == [192, 192, 288]
    assert tb_ref.geometry(80, 64, 16 * 3 * 180, 1) is not None and tb_ref.geometry(80, 64, 16 * 3 * 180 + 3, 1) is None


@pytest.mark.parametrize("Z", tc.SWEEP_ZS)
def test_every_block_is_divisible_by_its_generator(Z):
    """every A in 8 .. 4096: sizes add up, F >= 0 and below the K step, each block (payload + CRC24B) and the re-joined
    transport block (payload + CRC24A) leave remainder 0 in integer polynomial arithmetic"""
    rng = np.random.default_rng(Z)
    for A in tc.SWEEP_AS:
        p = rng.integers(0, 2, A).astype(np.uint8)
        blocks, g = tb_ref.segment(p, Z)
        assert [len(b) for b in blocks] == g["Ks"] and all(K in tb_ref.LTE_KS and K <= Z for K in g["Ks"])
        assert sum(K - g["L"] for K in g["Ks"]) == g["B"] + g["F"] and 0 <= g["F"] < 64 * g["C"]
        assert (g["L"], g["C"]) == ((0, 1) if A + 24 <= Z else (24, g["C"])) and g["C"] == len(blocks)
        assert not blocks[0][:g["F"]].any()
        if g["L"]:
            assert all(gf2_mod(as_int(b), G24B) == 0 for b in blocks)
        joined = np.concatenate([b[:len(b) - g["L"]] for b in blocks])[g["F"]:]
        assert np.array_equal(joined[:A], p) and gf2_mod(as_int(joined), G24A) == 0
        pay, tb_ok, cb_ok, syn = tb_ref.desegment(blocks, A, Z)
        assert np.array_equal(pay, p) and tb_ok == 1 and cb_ok.all() and syn == 0


def test_flipped_bits_are_seen_by_the_right_crc():
    A, Z = 88, 64
    p = tc.payloads(A, 1)[0]
    blocks, g = tb_ref.segment(p, Z)
    for r in range(g["C"]):
        for pos in (0, g["Ks"][r] - 25, g["Ks"][r] - 1):
            bad = [b.copy() for b in blocks]
            bad[r][pos] ^= 1
            _, tb_ok, cb_ok, _ = tb_ref.desegment(bad, A, Z)
            assert list(cb_ok) == [int(i != r) for i in range(g["C"])]
            assert tb_ok == (1 if pos == g["Ks"][r] - 1 else 0)              # a flip inside a CRC24B never reaches the B sequence


def test_rate_matching_sizes_and_groups():
    for (A, Z) in ((80, 64), (72, 64), (88, 64), (48, 64), (976, 528), (496, 528), (6128, 6144), (75376, 6144)):
        C = tb_ref.segmentation(A, Z)["C"]
        for q in tc.QS:
            for Gp in tc.g_sweep(C):
                g = tb_ref.geometry(A, Z, Gp * q, q)
                assert g is not None, (A, Z, Gp, q)
                assert sum(g["Es"]) == Gp * q and len(set(g["Es"])) <= 2 and all(E % q == 0 for E in g["Es"])
                assert g["Es"] == sorted(g["Es"]) and g["Es"].count(g["E1"]) in (g["gamma"], C)
                assert max(g["Es"]) - min(g["Es"]) in (0, q)
                gr = g["groups"]
                assert 1 <= len(gr) <= 3 and gr[0]["first"] == 0 and gr[-1]["first"] + gr[-1]["count"] == C
                for a, b in zip(gr, gr[1:]):
                    assert a["first"] + a["count"] == b["first"]
                    assert b["cw_bit_offset"] == a["cw_bit_offset"] + a["count"] * a["E"]
                    assert b["soft_offset"] == a["soft_offset"] + a["count"] * (3 * a["K"] + 12)
                for x in gr:
                    assert g["Ks"][x["first"]:x["first"] + x["count"]] == [x["K"]] * x["count"]
                    assert g["Es"][x["first"]:x["first"] + x["count"]] == [x["E"]] * x["count"]
    assert len(tb_ref.geometry(80, 64, 3 * 200 + 2, 1)["groups"]) == 3                           # K cut at 2, E cut at 1
    assert len(tb_ref.geometry(80, 64, 3 * 200 + 1, 1)["groups"]) == 2                           # both cuts at 2


@pytest.mark.parametrize("kind,g", ((lb.CRC24A, G24A), (lb.CRC24B, G24B)))
def test_crc_is_linear_in_the_way_chunk_and_combine_needs(kind, g):
    """crc(M1 || M2) = crc(M1) x^|M2| mod g ^ crc(M2), the right side in integer polynomial arithmetic"""
    rng = np.random.default_rng(kind)
    for n1, n2 in ((8, 8), (8, 4000), (1000, 24), (2048, 2048), (24, 8), (4096, 8)):
        m1, m2 = rng.integers(0, 2, n1).astype(np.uint8), rng.integers(0, 2, n2).astype(np.uint8)
        whole = lb.crc(np.concatenate([m1, m2]), kind)
        assert whole == gf2_mod(lb.crc(m1, kind) << n2, g) ^ lb.crc(m2, kind)
        assert whole == gf2_mod(as_int(np.concatenate([m1, m2])) << 24, g)


@pytest.mark.parametrize("A,Z,Gq,q,N_IR,rv", ((80, 64, 564, 1, 0, 0), (80, 64, 3 * 150 + 2, 2, 0, 1), (88, 64, 3 * 90 + 1, 6, 3 * 150, 2),
                                             (496, 528, 1700, 1, 0, 3), (976, 528, 1200, 2, 0, (0, 1, 2))))
def test_noiseless_round_trip(A, Z, Gq, q, N_IR, rv):
    qm, qp = tc.pairs(A, Z)
    p = tc.payloads(A, 3)
    G = Gq * q
    cw = tb_ref.encode(p, G, qm, qp, Z=Z, q=q, N_IR=N_IR, rv=rv, cw_bits=G + 5)
    assert cw.shape == (3, G + 5) and not cw[:, G:].any()
    llr = (4.0 * (1.0 - 2.0 * cw)).astype(np.float32)
    pay, tb_ok, cb_ok, syn, soft = tb_ref.decode(llr, A, G, qm, qp, 4, Z=Z, q=q, N_IR=N_IR, rv=rv)
    assert np.array_equal(pay, p) and tb_ok.all() and cb_ok.all() and not syn.any()
    assert soft.shape == (3, tb_ref.geometry(A, Z)["soft_floats"])


def test_harq_chain_condition_round_one_fails_round_two_decodes():
    """the condition of the device chain (tests/test_gpu_tb.py), on the reference alone: every transport block fails after
    the rv 0 round (E < K + 4) and every one passes once the rv 2 round is combined"""
    p, l0, l2 = tc.harq_rounds()
    qm, qp = tc.pairs(tc.HARQ_A, tc.HARQ_Z)
    kw = dict(Z=tc.HARQ_Z, q=tc.HARQ_Q)
    g = tb_ref.geometry(tc.HARQ_A, tc.HARQ_Z, tc.HARQ_G, tc.HARQ_Q)
    assert g["Es"] == [500, 500] and g["Ks"] == [528, 528] and g["F"] == 8 and all(E < K + 4 for E, K in zip(g["Es"], g["Ks"]))
    pay1, ok1, cb1, _, soft1 = tb_ref.decode(l0, tc.HARQ_A, tc.HARQ_G, qm, qp, tc.HARQ_ITERS, rv=0, **kw)
    pay2, ok2, cb2, _, _ = tb_ref.decode(l2, tc.HARQ_A, tc.HARQ_G, qm, qp, tc.HARQ_ITERS, rv=2, soft=soft1, **kw)
    assert not ok1.any() and ok2.all() and cb2.all() and np.array_equal(pay2, p)
