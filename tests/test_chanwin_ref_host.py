"""Pins tests/chanwin_ref.py (the fp64 restatement of the delay-window denoising contract, include/ofdm_mi355x.h) by means that do
not depend on it -- planted single taps whose outcome is known in closed form, the identity window -- and asserts the benefit the
stage exists for, on the reference alone: on the link cases of csi_cases.py and mrc_cases.py, seen through the oracle's receiver,
the windowed estimate decodes every block at noise levels where the LS estimate loses at least 8 of 64, and the tail power serves
as the per-unit noise variance of the combiner."""
import numpy as np
import pytest

import channel_ref
import chanwin_cases as wc
import chanwin_ref
import csi_cases as cc
import csi_ref
import mrc_cases as mc
import mrc_ref
import turbo_ref
from oracle import ofdm_oracle as orc
from test_csi_ref_host import wrong_blocks

RHO = 0.03


# ------------------------------------------------------------------------------------------ the contract in closed form
@pytest.mark.parametrize("N,Ks,Kd", [(64, 62, 60), (64, 52, 48), (64, 64, 64), (128, 126, 100), (1024, 1022, 600)])
def test_planted_single_taps(N, Ks, Kd):
    """a tap inside the window comes back unchanged on the sync bins with tail 0; a tap outside gives H' = 0 and
    tail = N/M |tap|^2; the gain follows the equaliser's expression with the lag de-rotation"""
    amp = complex(0.8, -0.5)
    sb, db = chanwin_ref.bins_p(Ks, N), chanwin_ref.bins_p(Kd, N)
    for pre, post in [(wc.CP[N] // 4, 3 * wc.CP[N] // 4), (0, 1), (0, 5), (N - 1, 1), (3, N - 4)]:
        M = N - pre - post
        taps = wc.planted_taps(N, pre, post)
        assert any(k for _, k in taps) and (M == 0 or any(not k for _, k in taps))
        assert {n for n, _ in taps} >= {0, post - 1, post, N - 1}
        for n0, kept in taps:
            assert kept == (n0 < post or n0 >= N - pre)
            H = wc.planted_row(N, n0, amp)
            for lag in wc.LAGS:
                Hw, g, tail = chanwin_ref.window_row(H, lag, pre, post, Ks, Kd, RHO)
                want = np.zeros(N, complex)
                if kept:
                    want[sb] = H[sb]
                assert np.max(np.abs(Hw - want)) < 1e-12, (pre, post, n0)
                assert abs(tail - (0.0 if kept else N / M * abs(amp) ** 2)) < 1e-12 * N
                assert not Hw[np.setdiff1d(np.arange(N), sb)].any()
                wg = np.conj(want[db]) / (np.abs(want[db]) ** 2 + RHO) * np.exp(2j * np.pi * lag * db / N)
                assert np.max(np.abs(g - wg)) < 1e-12 / RHO                  # |dg| <= |dH'| / rho, at H' = 0


@pytest.mark.parametrize("N,Ks", [(64, 62), (64, 52), (64, 64), (256, 254)])
def test_full_window_is_the_identity_on_the_sync_bins(N, Ks):
    rng = np.random.default_rng(N + Ks)
    H = rng.standard_normal(N) + 1j * rng.standard_normal(N)                 # energy on every bin, also outside the sync bins
    sb = chanwin_ref.bins_p(Ks, N)
    for pre, post in [(0, N), (N - 1, 1), (N // 2, N // 2)]:
        Hw, _, tail = chanwin_ref.window_row(H, 2, pre, post, Ks, 48, RHO)
        want = np.zeros(N, complex)
        want[sb] = H[sb]
        assert np.max(np.abs(Hw - want)) < 1e-12 and tail == 0.0 and not np.signbit(tail)


def test_rows_without_a_sync_and_bad_windows():
    rng = np.random.default_rng(3)
    H = np.stack([wc.random_row(rng, 64, 62) for _ in range(3)])
    tsr = np.array([[5, 1, 9, 1], [0, 0, 0, 0], [7, 2, 9, 1]])
    prev_H, prev_g = np.full((3, 64), 7 + 7j), np.full((3, 60), 9 - 9j)
    Hw, g, tail = chanwin_ref.window_rows(H, tsr, 4, 12, 62, 60, RHO, prev_H, prev_g)
    assert (Hw[1] == 7 + 7j).all() and (g[1] == 9 - 9j).all() and tail[1] == 0.0
    assert tail[0] > 0 and tail[2] > 0 and not (Hw[0] == 7 + 7j).any()
    for pre, post in [(-1, 4), (0, 0), (4, 0), (60, 5)]:
        with pytest.raises(ValueError):
            chanwin_ref.kept_taps(64, pre, post)


def test_window_removes_the_noise_outside_it():
    """white noise on the estimate of a 4-tap channel: the window (4, 12) keeps 16/64 of it"""
    rng = np.random.default_rng(4)
    N, Ks = 64, 64
    h = np.zeros(N, complex)
    h[:4] = [0.7, 0, 0, 0.6]
    H0 = np.fft.fft(h)
    err_ls, err_w, tails = [], [], []
    for _ in range(200):
        w = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.1 / 2)
        Hw, _, tail = chanwin_ref.window_row(H0 + w, 0, 4, 12, Ks, 60, RHO)
        keep = chanwin_ref.bins_p(Ks, N)
        err_ls.append(np.mean(np.abs(w[keep]) ** 2))
        err_w.append(np.mean(np.abs((Hw - H0)[keep]) ** 2))
        tails.append(tail)
    assert 0.2 < np.mean(err_w) / np.mean(err_ls) < 0.32                     # 16/64 = 0.25, plus what bin 0 leaks
    assert abs(np.mean(tails) - 0.1) < 0.01                                  # the tail power is the noise per bin


# ------------------------------------------------------------------------------------------ the benefit, on the reference alone
def received_branch(mod_case, taps, seed, noise_var, window):
    """the case's frames over one branch through the oracle's receiver -> dict of z, a (LS) and zw, aw, tail (windowed)"""
    c = mod_case
    info = c.info_bits()
    coded = turbo_ref.encode_segments(info, c.F1, c.F2, c.SEG_BITS)
    rows = [r for r in range(c.N_SYM) if r % 4 != 3]
    db = orc.bins_p(c.KD, c.N)
    noise = channel_ref.noise(seed, c.N_FRAMES, c.FRAME_LEN, noise_var)
    rho = 1.0 / 10.0 ** (c.SNR_ARG / 20.0)
    out = dict(z=np.zeros((c.N_FRAMES, c.N_DSYM, c.KD), np.complex64), a=np.zeros((c.N_FRAMES, c.KD), np.float32),
               zw=np.zeros((c.N_FRAMES, c.N_DSYM, c.KD), np.complex64), aw=np.zeros((c.N_FRAMES, c.KD), np.float32),
               tail=np.zeros(c.N_FRAMES), lag=np.zeros(c.N_FRAMES, int), info=info)
    for f in range(c.N_FRAMES):
        tx = orc.tx_modulate(coded[f], c.N, c.CP, c.KS, c.KD, c.N_SYM, modulation=c.MOD)
        x = np.zeros(c.FRAME_LEN, complex)
        y = np.convolve(tx, taps)[:c.FRAME_LEN - c.LEAD]
        x[c.LEAD:c.LEAD + len(y)] = y
        x += noise[f]
        o = orc.RxOracle(c.N_SYM, c.N, c.CP, c.KS, [1, 3], c.KD, c.SNR_ARG, c.GATE, force_fp64=True)
        o.work(x.astype(np.complex64), np.zeros(c.FRAME_LEN, np.complex64))
        assert o.corr_obs >= 0, "every frame of the case finds its sync"
        H = np.asarray(o.est_chan_freq_P[0], dtype=np.complex128)
        z = np.asarray(o.est_data_freq[rows], dtype=np.complex128)
        lag = int(o.time_synch_ref[1])
        Hw, gw, tail = chanwin_ref.window_row(H, lag, window[0], window[1], c.KS, c.KD, rho)
        g = np.conj(H[db]) / (np.abs(H[db]) ** 2 + rho) * np.exp(2j * np.pi * lag * db / c.N)   # the receiver's own gains
        out["z"][f], out["a"][f] = z, csi_ref.csi_row(H.astype(np.complex64), db)
        out["zw"][f], out["aw"][f] = z * (gw / g)[None, :], csi_ref.csi_row(Hw.astype(np.complex64), db)
        out["tail"][f], out["lag"][f] = tail, lag
    return out


def csi_lost(z, a, info, rho):
    llr = np.stack([csi_ref.demap_csi_segment(z[f], a[f], rho, cc.MOD)[0] for f in range(z.shape[0])])
    return wrong_blocks(llr, info)


def test_benefit_one_branch():
    rho = np.float32(1.0 / 10.0 ** (cc.SNR_ARG / 20.0))
    lost, tails = {}, {}
    for nv in wc.CSI_LEVELS:
        r = received_branch(cc, cc.TAPS, cc.SEED_NOISE, nv, wc.LINK_WINDOW)
        lost[nv] = (csi_lost(r["z"], r["a"], r["info"], rho), csi_lost(r["zw"], r["aw"], r["info"], rho))
        tails[nv] = float(np.mean(r["tail"]))
        print("noise %.4f: LS loses %d of %d, windowed %d; mean tail %.4f; lags %r"
              % (nv, lost[nv][0], cc.N_FRAMES, lost[nv][1], tails[nv], sorted(set(r["lag"]))))
    for nv in wc.CSI_LEVELS:
        assert lost[nv][0] >= wc.LS_MIN_LOST and lost[nv][1] == 0, (nv, lost[nv])
    assert wc.TAIL_MEAN_BOUNDS[0] <= tails[wc.CSI_LEVELS[0]] <= wc.TAIL_MEAN_BOUNDS[1]


def test_benefit_two_branches():
    rho = np.float32(1.0 / 10.0 ** (mc.SNR_ARG / 20.0))
    nv = wc.MRC_LEVEL
    br = [received_branch(mc, mc.TAPS[b], mc.SEED_NOISE + b, nv, wc.LINK_WINDOW) for b in range(mc.N_BRANCH)]
    info = br[0]["info"]
    z, a = np.stack([b["z"] for b in br]), np.stack([b["a"] for b in br])
    zw, aw = np.stack([b["zw"] for b in br]), np.stack([b["aw"] for b in br])
    tail = np.stack([b["tail"] for b in br])
    lost = dict(ls=wrong_blocks(mrc_ref.combine_segments(z, a, rho, mc.MOD, [nv] * mc.N_BRANCH)[0], info),
                given=wrong_blocks(mrc_ref.combine_segments(zw, aw, rho, mc.MOD, [nv] * mc.N_BRANCH)[0], info),
                tail=wrong_blocks(mrc_ref.combine_segments(zw, aw, rho, mc.MOD, tail)[0], info))
    print("noise %.2f, wrong blocks of %d: %r; mean tail %.4f" % (nv, mc.N_FRAMES, lost, float(tail.mean())))
    assert lost["ls"] >= wc.LS_MIN_LOST
    assert lost["given"] == 0 and lost["tail"] == 0
