"""tests/lte_bits_ref.py (the NumPy yardstick of csrc/bitproc.hip) pinned by independent means, without a GPU and without the
library: catalogue check values, divisibility, linearity, sequence prefixes recomputed by a bit-serial LFSR, the recurrences
themselves -- and that the noisy chain case of tests/test_gpu_bitproc.py holds what it is there for."""
import numpy as np

import lte_bits_ref as lb
import tbcc_cases

KINDS = (lb.CRC24A, lb.CRC24B, lb.CRC16, lb.CRC8)
CHECK_123456789 = {lb.CRC24A: 0xCDE703, lb.CRC24B: 0x23EF52, lb.CRC16: 0x31C3, lb.CRC8: 0xEA}
GOLD_PREFIX = {
    0: "0000001000011010000100100111101000100101100101010000001101010110",
    1: "0000001010000011000000110111010000101011100110101111110111100010",
    0x12345: "1101011001010111011110100111101100111010100001111011001101001001",
    0x7fffffff: "1111110100001011111100111000111000101110011000000101011110001110",
}


def test_crc_catalogue_check_values():
    msg = np.unpackbits(np.frombuffer(b"123456789", np.uint8), bitorder="big")
    assert msg.size == 72
    for kind in KINDS:
        assert lb.crc(msg, kind) == CHECK_123456789[kind], kind


def test_payload_and_parity_are_divisible_by_the_generator():
    rng = np.random.default_rng(1)
    for kind in KINDS:
        for A in (8, 24, 72, 2024):
            blk = lb.crc_attach(rng.integers(0, 2, (3, A)), kind, 0)
            assert blk.shape == (3, A + lb.CRC_BITS[kind])
            assert all(lb.poly_mod(b, kind) == 0 for b in blk)
            ok, syn, pay = lb.crc_check(blk, kind, 0)
            assert ok.all() and not syn.any() and np.array_equal(pay, blk[:, :A])


def test_crc_is_linear_and_the_mask_goes_into_the_parity_msb_first():
    rng = np.random.default_rng(2)
    for kind in KINDS:
        L = lb.CRC_BITS[kind]
        a, b = rng.integers(0, 2, (2, 120)).astype(np.uint8)
        assert lb.crc(a ^ b, kind) == lb.crc(a, kind) ^ lb.crc(b, kind)
        plain = lb.crc_attach(a[None], kind, 0)[0]
        for bit in (0, 1, L - 1):
            masked = lb.crc_attach(a[None], kind, 1 << (L - 1 - bit))[0]        # mask bit on top = parity bit p0
            assert np.flatnonzero(masked != plain).tolist() == [120 + bit]
        mask = int(rng.integers(1, 1 << L))
        ok, syn, _ = lb.crc_check(lb.crc_attach(a[None], kind, mask), kind, mask)
        assert ok[0] == 1 and syn[0] == mask                                    # the syndrome IS the mask: an RNTI is read from it
        ok, syn, _ = lb.crc_check(lb.crc_attach(a[None], kind, mask), kind, mask ^ 1)
        assert ok[0] == 0 and syn[0] == mask


def test_gold_prefixes_and_recurrences():
    for c_init, text in GOLD_PREFIX.items():
        assert "".join(map(str, lb.gold(c_init, 64))) == text, hex(c_init)
    assert np.array_equal(lb.gold(0xFFFFFFFF, 300), lb.gold(0x7FFFFFFF, 300))   # bit 31 is ignored
    n = 4000
    c0 = lb.gold(0, n + 31).astype(np.uint8)                                    # x2 = 0: c is x1 shifted
    assert np.array_equal(c0[31:], c0[3:n + 3] ^ c0[:n])
    d = lb.gold(0x12345, n + 31) ^ lb.gold(0x6ABCDEF1, n + 31)                  # x1 cancels: x2's recurrence
    assert d.any() and np.array_equal(d[31:], d[3:n + 3] ^ d[2:n + 2] ^ d[1:n + 1] ^ d[:n])


def test_descrambling_llrs_flips_signs_only_and_twice_is_the_identity():
    llr = np.array([[1.5, -2.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-42, 3.0, -4.0]], np.float32)
    llr.view(np.uint32)[0, 6] = 0x7FC12345                                      # a NaN with a payload
    out = lb.descramble_llr(llr, [0x12345], 8)
    flips = (out.view(np.uint32) ^ llr.view(np.uint32))[0]
    assert np.array_equal(flips[:8], lb.gold(0x12345, 8).astype(np.uint32) << np.uint32(31)) and not flips[8:].any()
    assert np.array_equal(lb.descramble_llr(out, [0x12345], 8).view(np.uint32), llr.view(np.uint32))


def test_the_chain_case_holds_what_it_is_there_for():
    """152 blocks at the -4 dB operating point of tests/tbcc_cases.py: at least 20 wrongly decoded blocks that still close
    (tb_ok = 1), every wrong block caught by the CRC, and without the descrambling at least 140 blocks fail the CRC"""
    assert np.isclose(lb.CHAIN_ESN0_DB, tbcc_cases.SWEEP_ESN0_DB - 10 * np.log10(lb.CHAIN_E / (3 * lb.CHAIN_K)))
    c = lb.chain_case()
    assert c["info"].shape == (152, 40) and c["llr"].shape == (lb.CHAIN_SEGS, lb.CHAIN_BPS * lb.CHAIN_E)
    bits, _, tb_ok, ok, syn = lb.chain_reference()
    wrong = np.any(bits != c["info"], axis=1)
    assert int((wrong & (tb_ok == 1)).sum()) >= 20, "wrong blocks that tb_ok does not see"
    assert not np.any(wrong & (ok == 1)), "an undetected error: choose another seed"
    assert np.array_equal(ok == 1, ~wrong) and np.array_equal(syn[~wrong], c["rnti"][~wrong])
    _, _, _, ok_plain, _ = lb.chain_reference(descrambled=False)
    assert int((ok_plain == 0).sum()) >= 140
