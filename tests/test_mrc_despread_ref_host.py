"""tests/mrc_despread_ref.py pinned without a GPU: one branch against the single-branch weights of dft_spread_ref (the two
formulas are algebraically equal), the weight rule against a Monte-Carlo variance of the unbiased despread symbol over two
branches, a row in which a branch is missing, the erasure and usability rules, and the link case on the reference alone."""
import math

import numpy as np
import pytest

import dft_spread_ref
import mrc_cases as mc
import mrc_despread_ref as ref
from oracle import ofdm_oracle as orc


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def branch_channels(M=60, N=64):
    bins = orc.bins_p(M, N)
    return [np.fft.fft(t, N)[bins] for t in mc.TAPS]


def equalised(rng, H, x_spread, sigma2, rho):
    """one branch behind the one-tap MMSE equaliser: z [rows][M] complex64, a [M] float32"""
    a = (np.abs(H) ** 2).astype(np.float32)
    y = H * x_spread + crandn(rng, *x_spread.shape) * math.sqrt(sigma2 / 2)
    z = np.conj(H) / (a.astype(np.float64) + float(np.float32(rho))) * y
    return z.astype(np.complex64), a


@pytest.mark.parametrize("rho", [0.03, 0.1, 0.004])
def test_one_branch_with_sigma2_equal_rho_has_the_single_branch_weights(rho):
    """B = 1, sigma2 = rho: A = a/rho, so b = a/(a + rho) and nu = beta eps equals step 3 of the DFT-spread contract.  The
    difference is the float32 rounding of c and t."""
    rng = np.random.default_rng(11)
    M = 60
    a = rng.uniform(0.01, 2.0, M).astype(np.float32)
    z = crandn(rng, 1, 3, M).astype(np.complex64)
    seg = ref.combine_despread_segment(z, a[None], rho, [float(np.float32(rho))])
    one = dft_spread_ref.weights(a, rho, float(np.float32(rho)))
    assert seg["usable"].all() and one["usable"]
    for wt in seg["wts"]:
        assert abs(wt["beta"] - one["beta"]) < 1e-6 * one["beta"]
        assert abs(wt["w"] - one["w"]) < 1e-6 * one["w"]
        assert abs(wt["beta"] * wt["eps"] - one["nu"]) < 1e-6 * one["nu"]
    # and the symbols: v / beta is the equalised symbol over beta
    u1, _, _ = dft_spread_ref.despread_segment(z[0], a, rho, float(np.float32(rho)))
    assert np.max(np.abs(seg["sym"] - u1)) < 1e-5 * np.max(np.abs(u1))


@pytest.mark.parametrize("s0,s1,rho", [(0.05, 0.05, 0.03), (0.2, 0.05, 0.03), (0.3, 0.3, 0.03)])
def test_weight_rule_predicts_the_error_variance(s0, s1, rho):
    """The two tap sets of mrc_cases.py, M = 60, 20 000 rows of 16-QAM, each branch through its one-tap MMSE equaliser with
    regulariser rho at its own noise variance: the error variance of the unbiased despread symbol is 1/w within 2 %."""
    M, rows = 60, 20000
    rng = np.random.default_rng(36211)
    x = orc.map_bits(rng.integers(0, 2, rows * M * 4), "16QAM").reshape(rows, M)
    xs = dft_spread_ref.spread(x)
    zs, As = zip(*[equalised(rng, H, xs, s2, rho) for H, s2 in zip(branch_channels(M), (s0, s1))])
    v, A, took = ref.combine_rows(np.stack(zs), np.stack(As), rho, [s0, s1])
    assert took.all() and np.array_equal(A, np.tile(A[0], (rows, 1)))
    wt = ref.row_weights(A[0])
    assert wt["usable"]
    u = dft_spread_ref.inverse(v.astype(np.complex128)) * float(wt["inv32"])
    measured = float(np.mean(np.abs(u - x) ** 2))
    predicted = 1.0 / wt["w"]
    print("sigma2 %.3g / %.3g rho %.3g: measured %.5f predicted %.5f ratio %.4f" % (s0, s1, rho, measured, predicted, measured / predicted))
    assert abs(measured - predicted) < 0.02 * predicted
    assert abs(wt["beta"] * wt["eps"] / wt["beta"] ** 2 - predicted) < 1e-12 * predicted


def test_a_row_without_one_branch_has_the_beta_of_the_others():
    rng = np.random.default_rng(3)
    B, rows, M = 3, 4, 12
    z = crandn(rng, B, rows, M).astype(np.complex64)
    a = rng.uniform(0.05, 2.0, (B, M)).astype(np.float32)
    s2 = [0.05, 0.08, 0.11]
    full = ref.combine_despread_segment(z, a, 0.03, s2)
    zz = z.copy()
    zz[1, 2] = 0                                             # branch 1 misses row 2
    got = ref.combine_despread_segment(zz, a, 0.03, s2)
    others = ref.combine_despread_segment(z[[0, 2]], a[[0, 2]], 0.03, [s2[0], s2[2]])
    assert got["usable"].all() and not got["took"][1, 2].any() and got["took"][1, [0, 1, 3]].all()
    for k in ("beta32", "weight32"):
        assert got[k][2] == others[k][2] and got[k][2] < full[k][2]
        assert np.array_equal(got[k][[0, 1, 3]], full[k][[0, 1, 3]])
    assert np.array_equal(got["comb"][2], others["comb"][2]) and np.array_equal(got["sym"][2], others["sym"][2])
    assert np.array_equal(got["comb"][[0, 1, 3]], full["comb"][[0, 1, 3]])


def _pz(x):
    x = np.ascontiguousarray(x)
    return not x.view(np.uint8).any()


def test_erasure_and_usability_rules():
    rng = np.random.default_rng(5)
    B, rows, M = 2, 3, 12
    z = crandn(rng, B, rows, M).astype(np.complex64)
    a = rng.uniform(0.1, 2.0, (B, M)).astype(np.float32)
    s2 = [0.05, 0.08]
    base = ref.combine_despread_segment(z, a, 0.03, s2)
    assert base["usable"].all() and (base["A"] > 0).all()
    # an entry that no branch can use: not combined, v = 0, b = 0 and e = 1 in the row sums
    aa = a.copy()
    aa[:, 4] = [0.0, np.nan]
    got = ref.combine_despread_segment(z, aa, 0.03, s2)
    assert not got["comb"][:, 4].any() and (got["A"][:, 4] == 0).all() and got["usable"].all()
    A = got["A"][0].astype(np.float64)
    assert abs(got["wts"][0]["beta"] - math.fsum(A / (A + 1)) / M) < 1e-15 and abs(got["wts"][0]["eps"] - math.fsum(1 / (A + 1)) / M) < 1e-15
    assert got["wts"][0]["beta"] < base["wts"][0]["beta"]
    # one branch unusable in an entry, or with a non-finite symbol: the other carries it
    aa = a.copy()
    aa[1, 4] = -1.0
    zz = z.copy()
    zz[0, 1, 7] = complex(np.nan, 0.5)
    got = ref.combine_despread_segment(zz, aa, 0.03, s2)
    alone0 = ref.combine_rows(z[:1], a[:1], 0.03, s2[:1])
    alone1 = ref.combine_rows(z[1:], a[1:], 0.03, s2[1:])
    assert np.array_equal(got["comb"][:, 4], alone0[0][:, 4]) and np.array_equal(got["A"][:, 4], alone0[1][:, 4])
    assert got["comb"][1, 7] == alone1[0][1, 7] and got["A"][1, 7] == alone1[1][1, 7]
    assert np.isfinite(got["sym"].view(np.float64)).all()
    # a row with nothing in any branch is an erasure: +0 everywhere, its neighbours are not touched
    zz = z.copy()
    zz[:, 1] = 0
    got = ref.combine_despread_segment(zz, a, 0.03, s2)
    assert list(got["erased"]) == [False, True, False] and list(got["usable"]) == [True, False, True]
    assert _pz(got["sym"][1]) and got["beta32"][1] == 0 and got["weight32"][1] == 0
    assert np.array_equal(got["sym"][[0, 2]], base["sym"][[0, 2]])
    llr, bits = ref.segment_llr(got, "64QAM")
    assert _pz(llr.reshape(rows, -1)[1]) and llr.reshape(rows, -1)[0].any()
    assert np.array_equal(bits.reshape(rows, -1)[1], np.tile(orc.demap_hard(np.zeros(1, np.complex64), "64QAM"), M))
    # a variance that is 0, not finite or negative takes its branch out; in every branch: every row erased
    for bad in (0.0, np.nan, np.inf, -0.1):
        got = ref.combine_despread_segment(z, a, 0.03, [bad, s2[1]])
        assert np.array_equal(got["comb"], alone1[0]) and got["usable"].all()
        got = ref.combine_despread_segment(z, a, 0.03, [bad, bad])
        assert got["erased"].all() and not got["usable"].any() and _pz(got["sym"]) and _pz(got["beta32"]) and _pz(got["weight32"])
    # a / sigma2 = 1e30: usable, beta = 1 to float32, a finite weight
    got = ref.combine_despread_segment(z, np.full((B, M), 1e10, np.float32), 0.03, [1e-20, 1e-20])
    assert got["usable"].all() and (got["beta32"] == 1).all() and np.isfinite(got["weight32"]).all() and (got["weight32"] > 1e29).all()
    # w = sum b / sum e <= max A <= the largest float32, so float(w) cannot overflow through step 6; float(1/beta) can:
    got = ref.combine_despread_segment(z, np.full((B, M), 1e-30, np.float32), 0.0, [1e10, 1e10])
    assert (got["A"] > 0).all() and not got["erased"].any()                                   # t = 1e-40, a float32 denormal
    assert not got["usable"].any() and _pz(got["sym"]) and _pz(got["beta32"]) and _pz(got["weight32"])
    big = float(np.finfo(np.float32).max)
    wt = ref.row_weights(np.full(M, big, np.float32))
    assert wt["usable"] and np.isfinite(wt["weight32"])
    # the usability rule itself on values step 6 cannot produce from float32 A
    assert not ref.row_weights(np.zeros(M, np.float32))["usable"]
    assert not ref.row_weights(np.full(M, 1.0, np.float32), erased=True)["usable"]


# ------------------------------------------------------------------------------------------ the link case, on the reference alone
def received_frames(noise_var):
    """the case's frames, transform-precoded, through the oracle's receiver branch by branch -> (z [B][frames][9][60] complex64
    equalised rows, a [B][frames][60] float32 channel powers, info bits)"""
    import channel_ref
    import csi_ref
    import mrc_despread_cases as dc
    import turbo_ref
    info = dc.info_bits()
    coded = turbo_ref.encode_segments(info, dc.F1, dc.F2, dc.SEG_BITS)
    rows = [r for r in range(dc.N_SYM) if r % 4 != 3]
    bins = orc.bins_p(dc.KD, dc.N)
    tx = []
    for f in range(dc.N_FRAMES):
        spread = dft_spread_ref.spread(orc.map_bits(coded[f], dc.MOD).reshape(dc.N_DSYM, dc.KD))
        tx.append(orc.tx_modulate(None, dc.N, dc.CP, dc.KS, dc.KD, dc.N_SYM, modulation=dc.MOD, data_symbols=spread))
    z = np.zeros((dc.N_BRANCH, dc.N_FRAMES, dc.N_DSYM, dc.KD), np.complex64)
    a = np.zeros((dc.N_BRANCH, dc.N_FRAMES, dc.KD), np.float32)
    for b in range(dc.N_BRANCH):
        noise = channel_ref.noise(dc.SEED_NOISE + b, dc.N_FRAMES, dc.FRAME_LEN, noise_var)
        for f in range(dc.N_FRAMES):
            y = np.convolve(tx[f], dc.TAPS[b])[:dc.FRAME_LEN - dc.LEAD]
            x = np.zeros(dc.FRAME_LEN, complex)
            x[dc.LEAD:dc.LEAD + len(y)] = y
            x += noise[f]
            o = orc.RxOracle(dc.N_SYM, dc.N, dc.CP, dc.KS, [1, 3], dc.KD, dc.SNR_ARG, dc.GATE, force_fp64=True)
            o.work(x.astype(np.complex64), np.zeros(dc.FRAME_LEN, np.complex64))
            z[b, f] = o.est_data_freq[rows]
            a[b, f] = csi_ref.csi_row(o.est_chan_freq_P[0].astype(np.complex64), bins)
    return z, a, info


def link_result(noise_var):
    """-> blocks lost of 64 at this noise level: {"combined", "branch 0 alone", "branch 1 alone"}.  The combined stage and the
    single-branch despreading stage (dft_spread_ref, noise given) both take noise_var as the variance of every branch."""
    import mrc_despread_cases as dc
    import turbo_ref
    rho = np.float32(1.0 / 10.0 ** (dc.SNR_ARG / 20.0))
    z, a, info = received_frames(noise_var)
    llr = {k: np.zeros((dc.N_FRAMES, dc.SEG_BITS), np.float32) for k in ("combined", "branch 0 alone", "branch 1 alone")}
    for f in range(dc.N_FRAMES):
        seg = ref.combine_despread_segment(z[:, f], a[:, f], rho, [noise_var] * dc.N_BRANCH)
        assert seg["usable"].all()
        llr["combined"][f] = ref.segment_llr(seg, dc.MOD)[0]
        for b in range(dc.N_BRANCH):
            u, wt, _ = dft_spread_ref.despread_segment(z[b, f], a[b, f], rho, noise_var)
            assert wt["usable"]
            llr["branch %d alone" % b][f] = dft_spread_ref.outputs_from(u.astype(np.complex64), wt["weight32"], dc.MOD)[0]
    lost = {}
    for k, v in llr.items():
        bits, _ = turbo_ref.decode_segments(v, 1, dc.K, dc.F1, dc.F2, dc.N_ITER)
        lost[k] = int((bits != info).any(axis=(1, 2)).sum())
    return lost


def test_link_case_on_the_reference():
    import mrc_despread_cases as dc
    assert dft_spread_ref.size_ok(dc.KD)
    res = {name: link_result(nv) for name, nv in (("level", dc.NOISE_VAR), ("1 dB up", dc.NOISE_VAR_1DB))}
    print("blocks lost of %d: %r" % (dc.N_FRAMES, res))
    assert res["level"]["combined"] == 0 and res["1 dB up"]["combined"] == 0
    assert res["level"]["branch 0 alone"] >= 1 and res["level"]["branch 1 alone"] >= 1
