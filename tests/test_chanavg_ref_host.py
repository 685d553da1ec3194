"""Pins tests/chanavg_ref.py (the fp64 restatement of the channel-estimate averaging contract, include/ofdm_mi355x.h) by means that
do not depend on it -- the oracle's own LS estimate on a noise-free frame, planted rotations, erasures, white noise of a known
variance -- and asserts the benefit the stage exists for, on the reference alone: on the link case of csi_cases.py, seen through
the oracle's receiver, the averaged estimate decodes every block at noise levels where the LS estimate loses at least 8 of 64, and
the average followed by the delay window holds where either alone does not."""
import numpy as np
import pytest

import channel_ref
import chanavg_cases as ac
import chanavg_ref
import chanwin_ref
import csi_cases as cc
import csi_ref
import turbo_ref
from oracle import ofdm_oracle as orc
from test_csi_ref_host import wrong_blocks

N, CPL, KS, KD = 64, 16, 62, 60
L = N + CPL
SNR_LS = ac.snr_lin()
RHO = 1.0 / SNR_LS
TAPS = np.array([0.8, 0.0, 0.3 - 0.4j, 0.0, 0.2j])


def clean_frame(n_pat, synch_dat=(1, 3), seed=1, lead=0):
    """a noise-free frame of n_pat patterns over TAPS -> x complex128, n_sym"""
    rng = np.random.default_rng(seed)
    S, D = synch_dat
    n_sym = (S + D) * n_pat
    bits = rng.integers(0, 2, D * n_pat * KD * 2).astype(np.uint8)
    tx = orc.tx_modulate(bits, N, CPL, KS, KD, n_sym, synch_dat=synch_dat)
    return np.concatenate((np.zeros(lead, complex), np.convolve(tx, TAPS))), n_sym


def oracle_ls(x, n_sym, synch_dat=(1, 3)):
    """the oracle's receiver on x -> (est_chan_freq_P[0], t0, lag)"""
    o = orc.RxOracle(n_sym, N, CPL, KS, list(synch_dat), KD, ac.SNR_ARG, 0.5, force_fp64=True)
    o.work(x, np.zeros(len(x), complex))
    assert o.corr_obs >= 0
    return np.asarray(o.est_chan_freq_P[0]), int(o.time_synch_ref[0]), int(o.time_synch_ref[1])


def run(x, tsr, n_avg=-1, frame_len=None, synch_dat=(1, 3), Ks=KS):
    return chanavg_ref.average_frame(x, len(x) if frame_len is None else frame_len, tsr, n_avg, N, CPL, synch_dat[0], synch_dat[1],
                                     Ks, KD, SNR_LS, RHO)


# ------------------------------------------------------------------------------------------ the contract by independent means
def test_noise_free_frame_is_the_oracles_estimate():
    x, n_sym = clean_frame(5)
    H, t0, lag = oracle_ls(x, n_sym)
    r = run(x, [t0, lag, 0, 1])
    sb = chanavg_ref.bins_p(KS, N)
    assert r["on"] and r["n_used"] == 5
    for p in range(5):
        assert np.max(np.abs(r["a"][p][sb] - H[sb])) < 1e-12, p
        assert abs(r["rot"][p] - 1.0) < 1e-12
    assert r["spread"] < 1e-20
    assert np.max(np.abs(r["H"] - r["a"][0])) < 1e-12
    assert not r["H"][np.setdiff1d(np.arange(N), sb)].any()
    db = chanavg_ref.bins_p(KD, N)
    want = np.conj(H[db]) / (np.abs(H[db]) ** 2 + RHO) * np.exp(2j * np.pi * lag * db / N)
    assert np.max(np.abs(r["gain"] - want)) < 1e-10


def test_planted_rotations():
    x, n_sym = clean_frame(6, seed=2)
    _, t0, lag = oracle_ls(x, n_sym)
    base = run(x, [t0, lag, 0, 1])
    theta = np.array([0.0, 0.4, -2.9, 1.7, 3.1, -0.01])
    y = x.copy()
    for p in range(1, 6):
        lo = t0 - CPL + L * 4 * p                                            # the pattern's span, from its sync symbol's CP on
        y[lo:lo + L * 4] *= np.exp(1j * theta[p])
    r = run(y, [t0, lag, 0, 1])
    assert np.max(np.abs(r["rot"] - np.exp(1j * theta))) < 1e-12
    assert np.max(np.abs(r["H"] - base["H"])) < 1e-12 and abs(r["spread"] - base["spread"]) < 1e-20
    assert r["n_used"] == 6


def test_n_avg_one_and_limits():
    x, n_sym = clean_frame(4, seed=3)
    x = x + 0.1 * np.random.default_rng(3).standard_normal(len(x))
    _, t0, lag = oracle_ls(x, n_sym)
    r = run(x, [t0, lag, 0, 1], n_avg=1)
    assert r["n_used"] == 1 and r["spread"] == 0.0 and not np.signbit(r["spread"]) and len(r["rot"]) == 1
    assert np.array_equal(r["H"], r["a"][0])
    assert run(x, [t0, lag, 0, 1], n_avg=2)["n_used"] == 2
    assert run(x, [t0, lag, 0, 1], n_avg=9)["n_used"] == 4 and len(run(x, [t0, lag, 0, 1], n_avg=9)["rot"]) == 4
    for bad in (0, -2):
        with pytest.raises(ValueError):
            run(x, [t0, lag, 0, 1], n_avg=bad)
    with pytest.raises(ValueError):
        run(x, [t0, lag, 0, 1], synch_dat=(2, 3))


def test_erasures():
    lead = 2 * L - N + 1                                                     # late enough for the last window to be cut alone
    x, n_sym = clean_frame(4, synch_dat=(1, 1), seed=4, lead=lead)
    x = x + 0.05 * np.random.default_rng(4).standard_normal(len(x))
    t0, lag = lead + CPL, 0
    full = run(x, [t0, lag, 0, 1], synch_dat=(1, 1))
    assert full["n_used"] == 4
    # a sync symbol of exact zeros does not take part; the others do as before
    y = x.copy()
    w2 = t0 + 2 * L * 2
    y[w2:w2 + N] = 0
    r = run(y, [t0, lag, 0, 1], synch_dat=(1, 1))
    assert r["n_used"] == 3 and r["rot"][2] == 0 and r["a"][2] is None and abs(r["rot"][1] - full["rot"][1]) < 1e-15
    # frame_len cut to w_3 + N - 1: the last pattern drops out; to w_3 + N: it takes part
    w3 = t0 + 3 * L * 2
    cut = run(x, [t0, lag, 0, 1], frame_len=w3 + N - 1, synch_dat=(1, 1))
    assert len(cut["rot"]) == 4 and cut["n_used"] == 3 and cut["rot"][3] == 0
    keep = run(x, [t0, lag, 0, 1], frame_len=w3 + N, synch_dat=(1, 1))
    assert keep["n_used"] == 4 and np.array_equal(keep["H"], full["H"])
    # a window before the frame's first sample is no candidate either; pattern 0 out = a row without a sync
    neg = run(x, [-1, lag, 0, 1], synch_dat=(1, 1))
    assert not neg["on"] and neg["n_used"] == 0 and neg["spread"] == 0.0 and not neg["rot"].any()
    nos = run(x, [t0, lag, 0, 0], synch_dat=(1, 1))
    assert not nos["on"] and nos["H"] is None and nos["gain"] is None and nos["n_used"] == 0 and not nos["rot"].any()
    assert len(nos["rot"]) == 4


def test_bin_listed_twice():
    """num_synch_bins == nfft: bin N/2 keeps its last list entry and E_p counts it twice"""
    Ks = 64
    rng = np.random.default_rng(5)
    x = rng.standard_normal(4 * L) + 1j * rng.standard_normal(4 * L)
    r = chanavg_ref.average_frame(x, len(x), [CPL, 1, 0, 1], 1, N, CPL, 1, 3, Ks, KD, SNR_LS, RHO)
    Y = np.fft.fft(x[CPL:CPL + N])
    sb = chanavg_ref.bins_p(Ks, N)
    assert sb[0] == sb[-1] == N // 2
    E = np.sum(np.abs(Y[sb]) ** 2)
    zc = chanavg_ref.zadoff_chu(Ks)
    want = np.sqrt(Ks / E) * Y[N // 2] * np.exp(2j * np.pi * 1 * (N // 2) / N) * np.conj(zc[-1]) / (1 + 1 / SNR_LS)
    assert abs(r["H"][N // 2] - want) < 1e-12 and r["H"][0] == 0
    assert np.max(np.abs(zc - orc.zadoff_chu(Ks, 23))) < 1e-12


def test_spread_is_the_planted_variance():
    """known estimates plus white noise of variance v per bin, planted behind the FFT: the mean spread over the trials lies within
    four standard deviations of the planted variance.  What the contract lets through of it: each pattern's noise has 2 Ks real
    dimensions; the normalisation by E_p removes the one along the estimate (its amplitude) and the phase alignment the one
    across it (its common phase), so the spread expects v (1 - 2 / (2 Ks)), on estimates scaled by 1 / sqrt(1 + v) (E_p = Ks (1 + v)
    on average; undone below).  One trial's spread is a chi-square of about 2 Ks (n - 1) degrees over that number: its standard
    deviation is v / sqrt(Ks (n - 1)), and v / sqrt(trials Ks (n - 1)) for the mean of the trials."""
    n, trials, v = 6, 200, 0.04
    rng = np.random.default_rng(6)
    sb = chanavg_ref.bins_p(KS, N)
    zc = chanavg_ref.zadoff_chu(KS)
    h = np.zeros(N, complex)
    h[:4] = [0.7, 0, 0.2j, 0.5]
    H0 = np.fft.fft(h)
    H0 *= np.sqrt(KS / np.sum(np.abs(H0[sb]) ** 2))                          # unit mean power on the sync bins
    spreads = []
    for _ in range(trials):
        x = np.zeros(n * 4 * L, complex)
        for p in range(n):
            Y = np.zeros(N, complex)
            Y[sb] = (H0[sb] + (rng.standard_normal(KS) + 1j * rng.standard_normal(KS)) * np.sqrt(v / 2)) * zc
            x[p * 4 * L:p * 4 * L + N] = np.fft.ifft(Y)
        # snr_ls -> infinity and E_p = Ks (1 + v) on average: a_p = (H0 + noise) / sqrt(1 + v) up to the fluctuation of E_p
        r = chanavg_ref.average_frame(x, len(x), [0, 0, 0, 1], -1, N, CPL, 1, 3, KS, KD, 1e30, RHO)
        assert r["n_used"] == n
        spreads.append(r["spread"] * (1 + v))
    sd = v / np.sqrt(trials * KS * (n - 1))
    assert abs(np.mean(spreads) - v * (1 - 1 / KS)) < 4 * sd, (np.mean(spreads), v, sd)


# ------------------------------------------------------------------------------------------ the benefit, on the reference alone
def received(noise_var):
    """the link case's frames through the oracle's receiver -> dict of z [F][rows][Kd] and |H|^2 rows per estimate
    (ls, avg, win, both), the spreads and info"""
    c = cc
    info = c.info_bits()
    coded = turbo_ref.encode_segments(info, c.F1, c.F2, c.SEG_BITS)
    rows = [r for r in range(c.N_SYM) if r % 4 != 3]
    db = orc.bins_p(c.KD, c.N)
    noise = channel_ref.noise(c.SEED_NOISE, c.N_FRAMES, c.FRAME_LEN, noise_var)
    rho = 1.0 / 10.0 ** (c.SNR_ARG / 20.0)
    kinds = ("ls", "avg", "win", "both")
    out = {k: (np.zeros((c.N_FRAMES, c.N_DSYM, c.KD), np.complex64), np.zeros((c.N_FRAMES, c.KD), np.float32)) for k in kinds}
    spread, n_used = np.zeros(c.N_FRAMES), np.zeros(c.N_FRAMES, int)
    for f in range(c.N_FRAMES):
        tx = orc.tx_modulate(coded[f], c.N, c.CP, c.KS, c.KD, c.N_SYM, modulation=c.MOD)
        x = np.zeros(c.FRAME_LEN, complex)
        y = np.convolve(tx, c.TAPS)[:c.FRAME_LEN - c.LEAD]
        x[c.LEAD:c.LEAD + len(y)] = y
        x = (x + noise[f]).astype(np.complex64)
        o = orc.RxOracle(c.N_SYM, c.N, c.CP, c.KS, [1, 3], c.KD, c.SNR_ARG, c.GATE, force_fp64=True)
        o.work(x, np.zeros(c.FRAME_LEN, np.complex64))
        assert o.corr_obs >= 0, "every frame of the case finds its sync"
        H = np.asarray(o.est_chan_freq_P[0], dtype=np.complex128)
        z = np.asarray(o.est_data_freq[rows], dtype=np.complex128)
        t0, lag = int(o.time_synch_ref[0]), int(o.time_synch_ref[1])
        g = np.conj(H[db]) / (np.abs(H[db]) ** 2 + rho) * np.exp(2j * np.pi * lag * db / c.N)   # the receiver's own gains
        r = chanavg_ref.average_frame(x, c.FRAME_LEN, [t0, lag, 0, 1], -1, c.N, c.CP, 1, 3, c.KS, c.KD, 1.0 / rho, rho)
        assert np.max(np.abs(r["a"][0] - H)) < 1e-12                         # pattern 0 is the receiver's row
        Hw, gw, _ = chanwin_ref.window_row(H, lag, *ac.LINK_WINDOW, c.KS, c.KD, rho)
        Hb, gb, _ = chanwin_ref.window_row(r["H"], lag, *ac.LINK_WINDOW, c.KS, c.KD, rho)
        for k, (He, ge) in dict(ls=(H, g), avg=(r["H"], r["gain"]), win=(Hw, gw), both=(Hb, gb)).items():
            out[k][0][f] = z * (ge / g)[None, :]
            out[k][1][f] = csi_ref.csi_row(He.astype(np.complex64), db)
        spread[f], n_used[f] = r["spread"], r["n_used"]
    return out, spread, n_used, info


def lost(za, info):
    rho = np.float32(1.0 / 10.0 ** (cc.SNR_ARG / 20.0))
    llr = np.stack([csi_ref.demap_csi_segment(za[0][f], za[1][f], rho, cc.MOD)[0] for f in range(za[0].shape[0])])
    return wrong_blocks(llr, info)


def test_benefit_of_the_average():
    for i, nv in enumerate(ac.LEVELS):
        out, spread, n_used, info = received(nv)
        ls, avg = lost(out["ls"], info), lost(out["avg"], info)
        print("noise %.4f: LS loses %d of %d, averaged %d; mean spread %.4f" % (nv, ls, cc.N_FRAMES, avg, spread.mean()))
        assert (n_used == 3).all()
        assert ls >= ac.LS_MIN_LOST and avg == 0, (nv, ls, avg)
        if i == 0:
            assert ac.SPREAD_MEAN_BOUNDS[0] < spread.mean() < ac.SPREAD_MEAN_BOUNDS[1]


def test_average_and_window_compose():
    out, _, _, info = received(ac.LEVEL_HIGH)
    n = {k: lost(out[k], info) for k in ("avg", "win", "both")}
    print("noise %.2f, wrong blocks of %d: %r" % (ac.LEVEL_HIGH, cc.N_FRAMES, n))
    assert n["win"] >= ac.SINGLE_MIN_LOST and n["avg"] >= ac.SINGLE_MIN_LOST and n["both"] <= ac.PAIR_MAX_LOST
