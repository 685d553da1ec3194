"""tests/turbo_rm_ref.py pinned by means that do not share its code (no GPU, no library): counts, the k0 values computed
independently, the permutation property, the position of the last NULL, the closed form the kernels use against the literal
walk, noiseless round trips through turbo_ref.decode, and the HARQ operating point the GPU chain test relies on."""
import numpy as np
import pytest

import turbo_cases as tc
import turbo_ref as tr
import turbo_rm_cases as rc
import turbo_rm_ref as rm

ALL_KS = tuple(range(tr.K_MIN, tr.K_MAX + 1, 8))


def test_dims_and_null_counts_for_every_k():
    nds = set()
    for K in ALL_KS:
        D, R, Kpi, ND, Kw = rm.dims(K)
        assert D == K + 4 and Kpi == 32 * R and Kpi - 32 < D <= Kpi and ND == Kpi - D and Kw == 3 * Kpi
        nds.add(ND)
        w = rm.buffer_index(K)
        assert w.shape == (Kw,)
        assert np.array_equal(np.sort(w[w >= 0]), np.arange(3 * K + 12))        # 3K + 12 non-NULL entries, each coded bit once
        assert w[Kw - 1] == rm.NULL                                            # the third stream's wrapped entry y[0]
        assert rm.n_avail(K, 0) == rm.n_avail(K, Kw) == 3 * K + 12
        assert rm.n_avail(K, Kpi) == D                                         # v0 alone: the systematic stream
    assert nds == {4, 12, 20, 28}
    assert [rm.dims(K)[3] for K in rc.SMALL_KS] == [20, 12, 4, 28] and [rm.dims(K)[1] for K in rc.SMALL_KS] == [2, 2, 2, 3]


def test_k0_values_computed_independently():
    assert [rm.k0(40, 0, rv) for rv in range(4)] == [4, 52, 100, 148]
    assert [rm.k0(6144, 0, rv) for rv in range(4)] == [386, 5018, 9650, 14282]
    for K in (40, 64, 6144):
        _, R, Kpi, _, Kw = rm.dims(K)
        for Ncb in (Kpi, 2 * Kpi + 1, Kw):
            for rv in range(4):
                assert rm.k0(K, Ncb, rv) == R * (2 * int(np.ceil(Ncb / (8.0 * R))) * rv + 2) < Ncb


def test_the_whole_block_is_a_permutation_at_every_rv_and_rv0_sends_systematic_bits_first():
    for K in (40, 48, 56, 64, 104, 512, 6144):
        n = 3 * K + 12
        for rv in range(4):
            assert np.array_equal(np.sort(rm.selection(K, n, 0, rv)), np.arange(n))
            assert np.array_equal(rm.selection(K, 2 * n, 0, rv), np.tile(rm.selection(K, n, 0, rv), 2))
        D, R = K + 4, rm.dims(K)[1]
        sel = rm.selection(K, n, 0, 0)
        lead = D - 2 * R + int((rm.buffer_index(K)[:2 * R] == rm.NULL).sum())   # what is left of v0 behind k0 = 2R
        assert np.all(sel[:lead] % 3 == 0) and len(set(sel[:lead].tolist())) == lead
        assert np.all(rm.selection(K, D, rm.dims(K)[2], 1) % 3 == 0)            # Ncb = Kpi: nothing but d0, at any rv


# ---------------------------------------------------------------------------------------------- closed form
BREV5 = np.array([int("{:05b}".format(x)[::-1], 2) for x in range(32)])
POPC = np.array([bin(x).count("1") for x in range(1 << 16)])


def popcount32(x):
    return POPC[x & 0xFFFF] + POPC[(x >> 16) & 0xFFFF]


def closed_form(K, Ncb, rv):
    """The kernels' arithmetic on integer arrays: -> (k0, n_avail, n0 [3K + 12]) with n0 = the index of a coded bit's first
    transmission in e (at E = infinity), -1 for a bit whose place in w is at or behind Ncb"""
    D = K + 4
    R = (D + 31) // 32
    Kpi = 32 * R
    ND = Kpi - D
    Ncb = Ncb or 3 * Kpi
    m01 = int(sum(1 << c for c in range(32) if BREV5[c] < ND))
    m2 = int(sum(1 << c for c in range(32) if BREV5[c] < ND - 1))

    def stream_cr(mask, c, r):                               # non-NULL entries in front of (column c, row r) of a stream
        return c * R + r - popcount32(mask & ((1 << c) - 1)) - ((r > 0) & ((mask >> c) & 1))

    def stream(mask, k):                                     # non-NULL entries among the first k of a stream
        return D if k >= Kpi else int(stream_cr(mask, np.int64(k // R), np.int64(k % R)))

    def count(p):                                            # non-NULL entries of w[0 .. p)
        if p <= Kpi:
            return stream(m01, p)
        q = p - Kpi
        return D + stream(m01, (q + 1) >> 1) + stream(m2, q >> 1)

    start = R * (2 * ((Ncb + 8 * R - 1) // (8 * R)) * rv + 2)
    navail, rank0 = count(Ncb), count(start)
    n0 = np.full(3 * K + 12, -1, np.int64)
    i = np.arange(D, dtype=np.int64)
    for j in range(3):
        y = ND + i - (1 if j == 2 else 0)
        c, r = BREV5[y & 31].astype(np.int64), y >> 5
        kv = c * R + r
        pos = kv if j == 0 else Kpi + 2 * kv + (j - 1)
        rank = stream_cr(m01, c, r)
        if j:
            rank = rank + D + stream_cr(m2, c, r)
        if j == 2:
            rank = rank + 1 - ((r == 0) & ((m01 >> c) & 1))   # v1[kv] in front of v2[kv], unless it is a NULL
        n0[3 * i + j] = np.where(pos < Ncb, (rank - rank0) % navail, -1)
    return start, navail, n0


@pytest.mark.parametrize("part", range(8))
def test_closed_form_equals_the_literal_walk_for_every_k_rv_and_three_ncb(part):
    for K in ALL_KS[part::8]:
        for Ncb in rc.ncbs(K):
            navail = rm.n_avail(K, Ncb)
            for rv in range(4):
                start, na, n0 = closed_form(K, Ncb, rv)
                assert (start, na) == (rm.k0(K, Ncb, rv), navail)
                sel = rm.selection(K, navail, Ncb, rv)                          # one turn of the buffer
                want = np.full(3 * K + 12, -1, np.int64)
                want[sel] = np.arange(navail)
                assert np.array_equal(n0, want), (K, Ncb, rv)


# ---------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("K,E,Ncb,rv", [(40, 132, 0, 0), (40, 132, 0, 3), (64, 204, 0, 1), (104, 250, 0, 0), (104, 400, 200, 2),
                                         (120, 1000, 0, 3), (512, 1000, 1200, 0)])
def test_noiseless_round_trip_through_the_decoder(K, E, Ncb, rv):
    f1, f2 = tc.QPP[K]
    c = np.random.default_rng(K + E).integers(0, 2, (5, K)).astype(np.uint8)
    e = rm.rate_match(tr.encode(c, f1, f2), E, Ncb, rv)
    llr = rm.dematch((1.0 - 2.0 * e).astype(np.float32), K, Ncb, rv)
    sel = rm.selection(K, E, Ncb, rv)
    counts = np.bincount(sel, minlength=3 * K + 12)
    assert np.array_equal(np.abs(llr[0]), counts.astype(np.float32))          # every copy of +-1 added; unsent bits are 0
    assert np.array_equal(tr.decode(llr, f1, f2, 4)[0], c)


def test_noiseless_round_trip_below_the_systematic_length_needs_a_second_round():
    """E < K + 4: rv 0 alone leaves information bits unsent; rv 0 and rv 2 combined decode"""
    K, E = 104, 100
    f1, f2 = tc.QPP[K]
    c = np.random.default_rng(3).integers(0, 2, (5, K)).astype(np.uint8)
    e = tr.encode(c, f1, f2)
    acc = rm.dematch((1.0 - 2.0 * rm.rate_match(e, E, 0, 0)).astype(np.float32), K, 0, 0)
    assert int((acc[:, 0:3 * K:3] == 0).sum()) > 0
    for rv in (2, 1, 3):
        acc = rm.dematch((1.0 - 2.0 * rm.rate_match(e, E, 0, rv)).astype(np.float32), K, 0, rv, old=acc)
    assert np.array_equal(tr.decode(acc, f1, f2, 6)[0], c)


def test_dematch_adds_in_scalar_order_and_keeps_a_single_negative_zero():
    K, Ncb, rv = 40, 0, 0
    n = 3 * K + 12
    E = 3 * n
    sel = rm.selection(K, E, Ncb, rv)
    l = np.zeros((1, E), np.float32)
    x = int(sel[5])
    l[0, [5, 5 + n, 5 + 2 * n]] = (3e38, 3e38, -3e38)                          # (3e38 + 3e38) - 3e38 = inf in this order
    assert rm.dematch(l, K, Ncb, rv)[0, x] == np.inf
    l[0, [5, 5 + n, 5 + 2 * n]] = (3e38, -3e38, 3e38)
    assert rm.dematch(l, K, Ncb, rv)[0, x] == np.float32(3e38)
    one = np.full((1, n), -0.0, np.float32)
    out = rm.dematch(one, K, Ncb, rv)
    assert np.all(np.signbit(out))                                              # a single -0 stays -0
    two = rm.dematch(np.full((1, n + 1), -0.0, np.float32), K, Ncb, rv)
    assert np.all(np.signbit(two)) and not two.any()                            # -0 + -0 = -0 as well
    short = rm.dematch(np.full((1, 10), -0.0, np.float32), K, Ncb, rv)
    unsent = np.setdiff1d(np.arange(n), rm.selection(K, 10, Ncb, rv))
    assert not np.any(np.signbit(short[0, unsent])) and not short[0, unsent].any()   # never sent: +0
    nan = rm.dematch(np.full((1, n), np.nan, np.float32), K, Ncb, rv)
    assert not nan.any() and not np.any(np.signbit(nan))                        # not finite counts as +0


# ---------------------------------------------------------------------------------------------- HARQ operating point
@pytest.mark.parametrize("K,E,esn0", rc.HARQ_NOISE_POINTS + rc.HARQ_POINTS)
def test_harq_operating_point(K, E, esn0):
    """rv 0 alone: at least half of the blocks decoded wrongly; rv 0 + rv 2 combined: none"""
    f1, f2 = tc.QPP[K]
    c, l0, l2 = rc.harq_rounds(K, E, esn0)
    first = rm.dematch(l0, K, 0, 0)
    wrong1 = int(np.any(tr.decode(first, f1, f2, rc.HARQ_ITERS)[0] != c, axis=1).sum())
    both = rm.dematch(l2, K, 0, 2, old=first)
    wrong2 = int(np.any(tr.decode(both, f1, f2, rc.HARQ_ITERS)[0] != c, axis=1).sum())
    print("HARQ K=%d E=%d Es/N0=%+g dB: %d -> %d of %d blocks wrong" % (K, E, esn0, wrong1, wrong2, rc.HARQ_BLOCKS))
    assert 2 * wrong1 >= rc.HARQ_BLOCKS and wrong2 == 0
