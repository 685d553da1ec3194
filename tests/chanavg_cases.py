"""The cases of the channel-estimate averaging tests, shared by test_chanavg_ref_host.py (the reference alone) and
test_gpu_chanavg.py (the device against the reference): the link case (csi_cases at noise levels where the LS estimate loses
blocks) and the frame batches of the stand-alone call."""
import numpy as np

from oracle import ofdm_oracle as orc

# ---- the link case: csi_cases, three patterns per frame
LEVELS = (0.175, 0.2203)                     # noise variances: the LS estimate loses 15 and 58 of 64 blocks, the averaged one none
LS_MIN_LOST = 8
LEVEL_HIGH = 0.30                            # the window alone loses 33, the average alone 36, the average then the window 5
SINGLE_MIN_LOST = 24
PAIR_MAX_LOST = 12
SPREAD_MEAN_BOUNDS = (0.12, 0.16)            # mean spread of the 64 frames at 0.175: sigma^2/(1 + sigma^2) = 0.149 less the bias of
                                             # an estimate of three (measured 0.1383)
LINK_WINDOW = (4, 12)

# ---- the stand-alone call
NFFTS = (64, 128, 256, 512, 1024, 2048, 4096)
CP = {64: 16, 128: 32, 256: 20, 512: 36, 1024: 72, 2048: 144, 4096: 288}
LAGS = (0, 3, -2)
SNR_ARG = 30.0                               # the receiver's snr argument (UTSA law: snr_ls = snr_data = 10^(snr/20))
SYNCH_DAT = (1, 1)                           # short frames: one data symbol per pattern
TAPS = np.array([1.0, 0.0, 0.0, 0.9]) / np.linalg.norm([1.0, 0.0, 0.0, 0.9])
LINE = 16                                    # complex64 samples per 128-byte line


def slots(N):
    """work items per workgroup of the library's FFT plan (fft_core.hpp: 8 points per lane at 64-pt, else 16; 64 lanes at least)"""
    T = N // (8 if N == 64 else 16)
    return 1 if T >= 64 else 64 // T


def snr_lin():
    return 10.0 ** (SNR_ARG / 20.0)


def make_batch(N, Ks, Kd, n_pat, seed, late=False):
    """n = slots(N) + 1 frames of n_pat (1, 1) patterns over the two-path channel -> dict(iq [n][stride] complex64, stride (odd),
    frame_len, tsr [n][4] int32, theta [n], p_rot [n], zeroed (frame, pattern) or None).
      lag      LAGS in turn; t0 = (start of the first sync symbol's body) - lag, so the lag is the true one
      t0       every third frame on a 128-byte line of the buffer's first frame, the others off it
      noise    variance 0.1 .. 0.3 across the frames
      theta    the samples of pattern p_rot's span are multiplied by e^{j theta}
      zeroed   one sync window of one frame set to exact zeros (n_pat >= 3)
      one frame (n // 2) has no sync
      late     every frame starts 2L - N + 1 + (f % 3) samples later, so that a frame_len of t0 + L*SD*(n_pat - 1) + N still holds
               n_pat whole patterns: the last window can be cut without the pattern count changing"""
    rng = np.random.default_rng(seed)
    cp = CP[N]
    L, SD = N + cp, sum(SYNCH_DAT)
    n = slots(N) + 1
    n_sym = SD * n_pat
    t0 = np.zeros(n, int)
    tsr = np.zeros((n, 4), np.int32)
    frames = []
    theta = rng.uniform(-np.pi, np.pi, n)
    p_rot = np.array([(1 + f) % n_pat for f in range(n)])
    for f in range(n):
        lag = LAGS[(f + seed) % len(LAGS)]
        lead = (lag - cp) % LINE if f % 3 == 0 else (lag - cp) % LINE + 1 + (f % 5)
        if late:
            lead = 2 * L - N + 1 + (f % 3) - cp + lag
        bits = rng.integers(0, 2, n_pat * Kd * 2).astype(np.uint8)
        tx = orc.tx_modulate(bits, N, cp, Ks, Kd, n_sym, synch_dat=SYNCH_DAT)
        p = p_rot[f]
        tx[L * SD * p:L * SD * (p + 1)] *= np.exp(1j * theta[f])
        y = np.convolve(tx, TAPS)
        nv = 0.1 + 0.2 * f / max(n - 1, 1)
        x = np.zeros(lead + len(y), complex)
        x[lead:] = y
        x += (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * np.sqrt(nv / 2)
        t0[f] = lead + cp - lag
        tsr[f] = [t0[f], lag, 40, 1]
        frames.append(x)
    frame_len = max(len(x) for x in frames)
    stride = frame_len + 3 + (frame_len % 2)                                # odd
    iq = np.zeros((n, stride), np.complex64)
    for f, x in enumerate(frames):
        iq[f, :len(x)] = x
    zeroed = None
    if n_pat >= 3:
        zf, zp = (n - 1 if n - 1 != n // 2 else 0, n_pat - 2)           # a frame with a sync
        w = t0[zf] + L * SD * zp
        iq[zf, w:w + N] = 0
        zeroed = (zf, zp)
    tsr[n // 2, 3] = 0
    return dict(iq=iq, stride=stride, frame_len=frame_len, tsr=tsr, theta=theta, p_rot=p_rot, zeroed=zeroed, t0=t0, n_pat=n_pat)


def standalone_cases():
    """(N, Ks, Kd, n_pat, n_avg) of the stand-alone call: every FFT size at 17 patterns (a full chunk and a remainder of 1); at
    64-pt 33 patterns with n_avg below, at and above the pattern count (P = 1, 2, 16, 17, 33) and the other sync-bin counts"""
    out = [(N, N - 2, N - 4, 17, -1) for N in NFFTS]
    out += [(64, 62, 60, 33, n_avg) for n_avg in (1, 2, 16, 17, 33, 40, -1)]
    out += [(64, 52, 48, 17, -1), (64, 64, 64, 17, -1), (64, 64, 60, 2, 5)]
    return out
