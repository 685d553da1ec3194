"""The cases of the delay-window channel-estimate denoising tests, shared by test_chanwin_ref_host.py (the reference alone) and
test_gpu_chanwin.py (the device against the reference): planted single-tap rows, random LS-like rows, the shapes that reach every
FFT plan, and the two link cases (csi_cases / mrc_cases at noise levels where the LS estimate loses blocks)."""
import numpy as np

import chanwin_ref

# ---- the link cases: csi_cases (one branch) and mrc_cases (two branches) with this window
LINK_WINDOW = (4, 12)                        # (pre, post) of 64 taps; the channel has 4, the search may lock 3 taps late
CSI_LEVELS = (0.175, 0.2203)                 # noise variances: the LS estimate loses 15 and 58 of 64 blocks, the windowed one none
MRC_LEVEL = 0.40                             # two branches, noise given: 57 of 64 with the LS estimate, none windowed
LS_MIN_LOST = 8
TAIL_MEAN_BOUNDS = (0.14, 0.19)              # mean tail of the 64 frames at 0.175: sigma^2/(1 + sigma^2) = 0.149, + 0.014 leakage

# ---- the stand-alone call
NFFTS = (64, 128, 256, 512, 1024, 2048, 4096)
CP = {64: 16, 128: 32, 256: 20, 512: 36, 1024: 72, 2048: 144, 4096: 288}
LAGS = (0, 3, -2)


def slots(N):
    """rows per workgroup of the library's FFT plan (fft_core.hpp: P = 8 points per lane at 64-pt, else 16; 64 lanes at least)"""
    T = N // (8 if N == 64 else 16)
    return 1 if T >= 64 else 64 // T


def windows(N):
    cp = CP[N]
    return [(cp // 4, 3 * cp // 4), (0, 1), (0, N), (N - 1, 1)]


def sync_bin_counts(N):
    return [N - 2, 52, N] if N == 64 else [N - 2]


def planted_taps(N, pre, post):
    """-> [(n0, kept)] for n0 in {0, post-1, post, N-pre-1, N-pre, N-1}, the ones that exist, each once"""
    keep = chanwin_ref.kept_taps(N, pre, post)
    cand = sorted({n for n in (0, post - 1, post, N - pre - 1, N - pre, N - 1) if 0 <= n < N})
    return [(n, bool(keep[n])) for n in cand]


def planted_row(N, n0, amp):
    """H of the single tap amp at delay n0, on every bin: its inverse FFT is that tap and nothing else"""
    return amp * np.exp(-2j * np.pi * n0 * np.arange(N) / N)


def random_row(rng, N, Ks, taps=6):
    """an LS-like row: a few taps around delay 0 plus white noise, zero outside the sync bins"""
    h = np.zeros(N, complex)
    idx = np.r_[0:taps, N - 2:N]
    h[idx] = (rng.standard_normal(idx.size) + 1j * rng.standard_normal(idx.size)) * 0.4
    H = np.fft.fft(h) + 0.2 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    out = np.zeros(N, complex)
    sb = chanwin_ref.bins_p(Ks, N)
    out[sb] = H[sb]
    return out


def standalone_rows(N, Ks, pre, post, seed):
    """-> H_in [n][N] complex64, tsr [n][4] int32 with n = slots(N) + 1 rows (a partly filled last workgroup): planted taps and
    random rows in turn, every lag of LAGS, and one row without a sync"""
    rng = np.random.default_rng(seed)
    n = slots(N) + 1
    planted = planted_taps(N, pre, post)
    H = np.zeros((n, N), np.complex64)
    tsr = np.zeros((n, 4), np.int32)
    for r in range(n):
        if r % 2 == seed % 2:
            n0, _ = planted[(r // 2 + seed) % len(planted)]
            H[r] = planted_row(N, n0, complex(0.8, -0.5))
        else:
            H[r] = random_row(rng, N, Ks)
        tsr[r] = [100 + r, LAGS[(r + seed) % len(LAGS)], 50, 1]
    tsr[n // 2, 3] = 0                       # a frame without a sync
    return H, tsr
