"""Pins tests/chantrack_ref.py (the fp64 restatement of the channel-tracking contract, include/ofdm_mi355x.h) by means that do not
depend on it -- chanavg_ref's per-pattern estimate, chanwin_ref's window, a static channel, planted erasures -- and asserts the
benefit the stage exists for, on the reference alone: on the link case of chantrack_cases.py (two paths with Doppler) the estimate
of pattern 0 held for the whole frame loses at least 400 of the 2520 bits of patterns 0-6 and OFDM_TRACK_LINEAR loses none."""
import numpy as np
import pytest

import chanavg_ref
import chantrack_cases as tc
import chantrack_ref as tr
import chanwin_ref
from oracle import ofdm_oracle as orc

N, CPL, KS, KD = 64, 16, 62, 60
L = N + CPL
SNR = tc.snr_lin()
RHO = 1.0 / SNR
TAPS = np.array([0.8, 0.0, 0.3 - 0.4j, 0.0, 0.2j])


def clean_frame(n_pat, synch_dat=(1, 3), seed=1, lead=0):
    rng = np.random.default_rng(seed)
    S, D = synch_dat
    bits = rng.integers(0, 2, D * n_pat * KD * 2).astype(np.uint8)
    tx = orc.tx_modulate(bits, N, CPL, KS, KD, (S + D) * n_pat, synch_dat=synch_dat)
    return np.concatenate((np.zeros(lead, complex), np.convolve(tx, TAPS))), bits


def run(x, tsr, mode, synch_dat=(1, 3), frame_len=None, window=(0, 0), Ks=KS, Kd=KD):
    return tr.track_frame(x, len(x) if frame_len is None else frame_len, tsr, mode, N, CPL, synch_dat[0], synch_dat[1], Ks, Kd, SNR,
                          RHO, window)


# ------------------------------------------------------------------------------------------ the benefit, on the reference alone
@pytest.mark.parametrize("seed", tc.LINK["seeds"])
def test_link_case(seed):
    c = tc.LINK
    fr = tc.link_frame(seed)
    snr = tc.snr_lin(c["snr_arg"])
    S, D = c["synch_dat"]
    rows = 7 * D
    lost = {}
    for name, mode in (("held", tr.FIRST), ("hold", tr.HOLD), ("linear", tr.LINEAR)):
        r = tr.track_frame(fr["x"], fr["frame_len"], fr["tsr"], mode, c["N"], c["cp"], S, D, c["Ks"], c["Kd"], snr, 1.0 / snr)
        assert r["on"] and r["takes"].all() and r["demod"].all()
        lost[name] = (tc.bit_errors(r["eq"][:rows], fr["bits"]), tc.bit_errors(r["eq"][rows:], fr["bits"][tc.LINK_BITS:]))
    print("seed %d: bit errors (patterns 0-6 of %d, last pattern of 360): %r" % (seed, tc.LINK_BITS, lost))
    assert lost["held"][0] >= tc.LINK_HELD_MIN and lost["linear"][0] == tc.LINK_LINEAR_LOST, lost
    assert lost["held"][0] == tc.LINK_HELD_LOST[seed], "the figures of chantrack_cases.py and DESIGN.md are the reference's"
    assert lost["linear"][1] == lost["hold"][1], "the last pattern has no later sync symbol: LINEAR holds"


# ------------------------------------------------------------------------------------------ the contract by independent means
def test_static_channel_every_estimate_agrees():
    x, bits = clean_frame(5)
    tsr = [CPL, 0, 0, 1]
    res = [run(x, tsr, m) for m in (tr.LINEAR, tr.HOLD, tr.FIRST)]
    assert res[0]["on"] and res[0]["takes"].all()
    for r in res[1:]:
        assert np.max(np.abs(r["eq"] - res[0]["eq"])) < 1e-9 and np.max(np.abs(r["csi"] - res[0]["csi"])) < 1e-9
    assert tc.bit_errors(res[0]["eq"], bits) == 0
    # the held estimate is ofdm_rx_demod_frames' row: the oracle's receiver gives the same symbols
    o = orc.RxOracle(20, N, CPL, KS, [1, 3], KD, tc.SNR_ARG, 0.5, force_fp64=True)
    o.work(x, np.zeros(len(x), complex))
    assert (int(o.time_synch_ref[0]), int(o.time_synch_ref[1])) == (CPL, 0)
    rows = [r for r in range(20) if r % 4 != 3]
    assert np.max(np.abs(np.asarray(o.est_data_freq)[rows] - res[2]["eq"])) < 1e-9


def test_estimates_are_chanavg_refs():
    x, _ = clean_frame(4, seed=2, lead=5)
    x = x + 0.05 * np.random.default_rng(2).standard_normal(len(x))
    for lag in tc.LAGS:
        r = run(x, [5 + CPL - lag, lag, 0, 1], tr.LINEAR)
        zc = chanavg_ref.zadoff_chu(KS)
        for p in range(4):
            want = chanavg_ref.pattern_estimate(x, len(x), 5 + CPL - lag + L * 4 * p, lag, N, KS, SNR, zc)
            assert np.array_equal(r["H_pat"][p], want), (lag, p)
        assert not r["H_pat"][:, np.setdiff1d(np.arange(N), tr.bins_p(KS, N))].any()


def test_weights_and_erasures():
    x, _ = clean_frame(5, seed=3)
    x = x * np.exp(2j * np.pi * 0.004 * np.arange(len(x)) / N)               # a drift: the estimates differ
    tsr = [CPL, 0, 0, 1]
    full = run(x, tsr, tr.LINEAR)
    want = [(p * 4 + 1 + m - p * 4) / 4.0 if p < 4 else np.nan for p in range(5) for m in range(3)]
    assert np.array_equal(full["weight"], np.array(want, np.float32).astype(float), equal_nan=True)
    db = tr.bins_p(KD, N)
    for r, (p, m) in enumerate((p, m) for p in range(5) for m in range(3)):
        H = full["H_pat"][p] + want[r] * (full["H_pat"][p + 1] - full["H_pat"][p]) if p < 4 else full["H_pat"][4]
        assert np.allclose(full["csi"][r], np.abs(H[db]) ** 2, rtol=1e-12, atol=0), r
    # a pattern in the middle that does not take part: the weights run over the doubled gap
    y = x.copy()
    y[CPL + L * 4 * 2:CPL + L * 4 * 2 + N] = 0
    mid = run(y, tsr, tr.LINEAR)
    assert list(mid["takes"]) == [1, 1, 0, 1, 1] and not mid["H_pat"][2].any()
    w = mid["weight"].reshape(5, 3)
    assert np.array_equal(w[1], np.float32([1, 2, 3]) / np.float32(8)) and np.array_equal(w[2], np.float32([5, 6, 7]) / np.float32(8))
    assert np.array_equal(w[0], full["weight"][:3]) and np.array_equal(w[3], full["weight"][9:12])
    hold = run(y, tsr, tr.HOLD)
    assert np.array_equal(hold["csi"][6], hold["csi"][3]) and np.isnan(hold["weight"]).all()
    # the last sync symbol zeroed: patterns 3 and 4 hold a_3
    z = x.copy()
    z[CPL + L * 4 * 4:CPL + L * 4 * 4 + N] = 0
    last = run(z, tsr, tr.LINEAR)
    assert list(last["takes"]) == [1, 1, 1, 1, 0] and np.isnan(last["weight"][9:]).all() and not np.isnan(last["weight"][:9]).any()
    assert np.allclose(last["csi"][9:], np.abs(last["H_pat"][3][db]) ** 2, rtol=1e-12, atol=0)
    # pattern 0 zeroed: a frame without a sync
    v = x.copy()
    v[CPL:CPL + N] = 0
    off = run(v, tsr, tr.LINEAR)
    assert not off["on"] and not off["eq"].any() and not off["csi"].any() and not off["H_pat"].any() and not off["takes"].any()
    nos = run(x, [CPL, 0, 0, 0], tr.LINEAR)
    assert not nos["on"] and not nos["eq"].any() and not nos["takes"].any()


def test_guard_and_zero_padding():
    lead = 2 * L - N + 1
    x, _ = clean_frame(3, synch_dat=(1, 1), seed=4, lead=lead)
    t0 = lead + CPL
    tsr = [t0, 0, 0, 1]
    ptr2 = t0 + L * (2 * 2 + 1)
    full = run(x, tsr, tr.LINEAR, synch_dat=(1, 1))
    assert full["demod"].all()
    cut = run(x, tsr, tr.LINEAR, synch_dat=(1, 1), frame_len=ptr2 + N - 2)    # ptr + N - 1 > frame_len: the rows are zeros
    assert list(cut["demod"]) == [True, True, False] and not cut["eq"][2].any() and cut["csi"][2].any()
    edge = run(x, tsr, tr.LINEAR, synch_dat=(1, 1), frame_len=ptr2 + N - 1)   # the guard holds; the last sample is padding
    assert edge["demod"].all()
    seg = np.array(x[ptr2:ptr2 + N])
    seg[-1] = 0
    Y = np.fft.fft(seg)[tr.bins_p(KD, N)]
    H = edge["H_pat"][2][tr.bins_p(KD, N)]
    want = Y * np.sqrt(KD / np.sum(np.abs(Y) ** 2)) * np.conj(H) / (np.abs(H) ** 2 + RHO)
    assert np.max(np.abs(edge["eq"][2] - want)) < 1e-12


def test_window_is_chanwin_refs_row_by_row():
    x, _ = clean_frame(4, seed=5)
    x = x + 0.05 * np.random.default_rng(5).standard_normal(len(x))
    tsr = [CPL - 3, 3, 0, 1]
    x[tsr[0] + L * 4:tsr[0] + L * 4 + N] = 0                                 # pattern 1 does not take part
    plain, win = run(x, tsr, tr.LINEAR), run(x, tsr, tr.LINEAR, window=tc.WINDOW)
    assert list(win["takes"]) == [1, 0, 1, 1]
    for p in range(4):
        if p == 1:
            assert not win["H_pat"][1].any()
            continue
        want, _, _ = chanwin_ref.window_row(plain["H_pat"][p], 3, *tc.WINDOW, KS, KD, RHO)
        assert np.max(np.abs(win["H_pat"][p] - want)) < 1e-14, p
    assert np.max(np.abs(win["eq"] - plain["eq"])) > 1e-4
    with pytest.raises(ValueError):
        run(x, tsr, tr.LINEAR, window=(-1, 4))
    with pytest.raises(ValueError):
        run(x, tsr, 7)
    with pytest.raises(ValueError):
        run(x, tsr, tr.LINEAR, synch_dat=(2, 3))


def test_bins_listed_twice():
    """num_synch_bins == num_data_bins == nfft: P_s counts bin N/2 twice and both list entries of the row hold its value"""
    rng = np.random.default_rng(6)
    x = rng.standard_normal(8 * L) + 1j * rng.standard_normal(8 * L)
    r = run(x, [CPL, 1, 0, 1], tr.LINEAR, Ks=64, Kd=64)
    db = tr.bins_p(64, N)
    assert db[0] == db[-1] == N // 2
    assert np.array_equal(r["eq"][:, 0], r["eq"][:, -1]) and r["eq"][:, 0].all()
    Y = np.fft.fft(x[CPL + L:CPL + L + N])
    P = np.sum(np.abs(Y[db]) ** 2)
    H = r["H_pat"][0] + 0.25 * (r["H_pat"][1] - r["H_pat"][0])
    k = N // 2
    want = Y[k] * np.sqrt(64 / P) * np.conj(H[k]) / (abs(H[k]) ** 2 + RHO) * np.exp(2j * np.pi * k / N)
    assert abs(r["eq"][0, 0] - want) < 1e-12
