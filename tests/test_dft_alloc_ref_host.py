"""tests/dft_alloc_ref.py pinned without a GPU: the restatement of the multi-user allocation contract is the single-transform
restatement per allocation, two users through different channels come back from one call each with the gain and weight of its
own columns, a user's outputs do not depend on another user's data or channel, and the loopback case of test_gpu_dft_alloc.py
(S1 on the 64-pt numerology, flat unit channel, no noise) is error-free on the oracle's receiver with the restated stage."""
import numpy as np

import dft_alloc_ref as aref
import dft_spread_ref as ref
from oracle import ofdm_oracle as orc

S1 = [(0, 12, 2), (12, 24, 4), (36, 24, 6)]
NAME = {2: "QPSK", 4: "16QAM", 6: "64QAM"}


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def test_one_allocation_over_the_row_is_the_single_transform():
    rng = np.random.default_rng(1)
    rows, M = 3, 60
    z = crandn(rng, rows, M)
    a = rng.uniform(0.05, 2.0, M).astype(np.float32)
    (u, wt, er), = aref.despread_alloc_segment(z, a, [(0, M, 4)], 0.03, 0.01)
    u1, wt1, er1 = ref.despread_segment(z, a, 0.03, 0.01)
    assert np.array_equal(u, u1) and wt == wt1 and np.array_equal(er, er1)
    assert np.array_equal(aref.spread_alloc(z, [(0, M)]), ref.spread(z))
    (p, wp, _), = aref.despread_alloc_segment(z, None, [(0, M, 4)], 0.0, 0.0)
    assert wp["beta32"] == 1 and np.allclose(p, ref.inverse(z))


def two_users(rng, h2=(1.0, 0.05), rho=0.03, sigma2=0.0):
    """S1's first and last allocation as two users, each through its own flat channel with |H|^2 = h2: the equalised row and
    the channel powers a receiver would hold, the symbols sent"""
    allocs = [S1[0], S1[2]]
    rows, row_len = 4, 60
    sent = {}
    z = crandn(rng, rows, row_len)                           # the gap holds anything
    a = np.full(row_len, 0.5, np.float32)
    for (s, M, bps), p in zip(allocs, h2):
        x = orc.map_bits(rng.integers(0, 2, rows * M * bps), NAME[bps]).reshape(rows, M)
        sent[s] = x
        z[:, s:s + M] = (p / (p + rho)) * ref.spread(x)      # the MMSE equaliser's bias on a flat channel
        a[s:s + M] = p
    return allocs, z, a, sent


def test_two_users_through_different_channels_get_their_own_gain_and_weight():
    rho, sigma2 = 0.03, 0.01
    allocs, z, a, sent = two_users(np.random.default_rng(2), rho=rho)
    out = aref.despread_alloc_segment(z, a, allocs, rho, sigma2)
    for (s, M, bps), (u, wt, er), p in zip(allocs, out, (1.0, 0.05)):
        p = float(np.float32(p))
        rho32 = float(np.float32(rho))
        beta = p / (p + rho32)
        assert wt["usable"] and not er.any()
        assert abs(wt["beta"] - beta) < 1e-12
        nu = sigma2 * p / (p + rho32) ** 2                   # flat inside the allocation: no spread of the b_k
        assert abs(wt["w"] - beta * beta / nu) < 1e-6 * wt["w"]
        assert np.abs(u - sent[s]).max() < 1e-6              # unbiased by the user's own beta
        llr, hard = ref.outputs_from(u.astype(np.complex64), wt["weight32"], bps)
        assert np.array_equal(hard, orc.demap_hard(sent[s].astype(np.complex64).ravel(), NAME[bps]))
    assert out[0][1]["beta"] > 0.97 and out[1][1]["beta"] < 0.63      # 1/(1.03) and 0.05/0.08
    assert out[0][1]["w"] > 10 * out[1][1]["w"]


def test_a_user_does_not_see_another_users_data_or_channel():
    allocs, z, a, _ = two_users(np.random.default_rng(3))
    base = aref.despread_alloc_segment(z, a, allocs, 0.03, 0.01)
    z2, a2 = z.copy(), a.copy()
    s, M, _ = allocs[1]
    z2[:, s:s + M] = crandn(np.random.default_rng(4), z.shape[0], M)
    z2[:, 12:36] = np.nan                                    # the gap as well
    a2[s:s + M] = 7.0
    a2[12:36] = np.nan
    other = aref.despread_alloc_segment(z2, a2, allocs, 0.03, 0.01)
    assert np.array_equal(base[0][0], other[0][0]) and base[0][1] == other[0][1]
    assert not np.array_equal(base[1][0], other[1][0]) and base[1][1]["beta"] != other[1][1]["beta"]


def test_set_rules_and_layout():
    assert aref.check_set(S1) is None and aref.check_set(S1, row_len=59) == "row too short"
    assert aref.check_set([(0, 12, 2), (11, 12, 2)]) == "overlap"
    assert aref.check_set([(0, 7, 2)]) == "bad M" and aref.check_set([(4085, 12, 2)]) == "start + M > 4096"
    assert aref.check_set([(0, 12, 1)]) == "bad modulation" and aref.check_set([(-1, 12, 2)]) == "start < 0"
    assert aref.check_set([(12 * k, 12, 2) for k in range(33)]) == "too many"
    so, lo, bo, tot = aref.layout(S1, 3, 2)
    assert so == [0, 72, 216] and lo == [0, 144, 720] and bo == lo and tot == (360, 1584, 1584)
    assert aref.layout(S1, 3, 2, packed=True)[2] == [0, 18, 90]


def test_loopback_case_is_error_free_on_the_reference():
    """The loopback of test_gpu_dft_alloc.py on the CPU: S1 at the handle's modulation (QPSK) and S1 without its middle
    allocation, sent through a flat unit channel without noise, received by the oracle's receiver, despread by the restatement:
    every allocation's bits come back exactly (0 errors of 6 rows x 60 and 6 rows x 36 symbols)."""
    N, cp, Ks, Kd, n_sym, mod = 64, 16, 62, 60, 8, "QPSK"
    L = N + cp
    rows = [r for r in range(n_sym) if r % 4 != 3]
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, len(rows) * Kd * 2).astype(np.uint8)
    for allocs in ([(s, M, 2) for s, M, _ in S1], [(0, 12, 2), (36, 24, 2)]):
        x = orc.map_bits(bits, mod).reshape(len(rows), Kd)
        tx = orc.tx_modulate(None, N, cp, Ks, Kd, n_sym, modulation=mod, data_symbols=aref.spread_alloc(x, allocs))
        fl = n_sym * L + L
        y = np.zeros(fl, np.complex64)
        y[5:5 + len(tx)] = tx
        o = orc.RxOracle(n_sym, N, cp, Ks, [1, 3], Kd, 30.0, 0.7, force_fp64=True)
        o.work(y, np.zeros(fl, np.complex64))
        import csi_ref
        z = o.est_data_freq[rows].astype(np.complex64)
        a = csi_ref.csi_row(o.est_chan_freq_P[0].astype(np.complex64), orc.bins_p(Kd, N))
        rho = np.float32(1.0 / 10.0 ** (30.0 / 20.0))
        want = bits.reshape(len(rows), Kd, 2)
        for (s, M, bps), (u, wt, er) in zip(allocs, aref.despread_alloc_segment(z, a, allocs, rho, float(rho))):
            assert wt["usable"] and not er.any()
            _, hard = ref.outputs_from(u.astype(np.complex64), wt["weight32"], bps)
            assert np.array_equal(hard.reshape(len(rows), M, 2), want[:, s:s + M]), (s, M)
