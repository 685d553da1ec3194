"""The cases of the channel-tracking tests, shared by test_chantrack_ref_host.py (the reference alone) and test_gpu_chantrack.py
(the device against the reference): the link case (a two-path channel with Doppler on its paths) and the frame batches of the
stand-alone call."""
import numpy as np

from oracle import ofdm_oracle as orc

MODS = {2: "QPSK", 4: "16QAM", 6: "64QAM"}

# ---- the link case: 64-pt, eight (1, 3) patterns, QPSK; two paths whose samples turn by e^{+-j 2 pi 0.005 n / N}
LINK = dict(N=64, cp=16, Ks=62, Kd=60, synch_dat=(1, 3), n_pat=8, mod="QPSK", snr_arg=30.0, delays=(0, 3), gains=(1.0, 0.9),
            doppler=0.005, noise_var=1e-4, seeds=(0, 1, 2, 3))
LINK_BITS = 7 * 3 * 60 * 2                   # patterns 0-6: 2520 bits (the last pattern has no following sync symbol and holds)
# chantrack_ref alone on the four seeds (test_chantrack_ref_host.py prints them): the estimate of pattern 0 held for the whole
# frame loses 499 .. 503 of the 2520 bits, OFDM_TRACK_HOLD (the latest sync symbol's estimate) 39 .. 41, OFDM_TRACK_LINEAR none;
# the last pattern, which LINEAR holds, loses 6 or 7 of its 360.  At noise variance 1e-2: held 470 .. 523, LINEAR 22 .. 51.
LINK_HELD_LOST = {0: 499, 1: 500, 2: 502, 3: 503}
LINK_HELD_MIN = 400
LINK_LINEAR_LOST = 0

# ---- the stand-alone call
NFFTS = (64, 128, 256, 512, 1024, 2048, 4096)
CP = {64: 16, 128: 32, 256: 20, 512: 36, 1024: 72, 2048: 144, 4096: 288}
LAGS = (0, 3, -2)
SNR_ARG = 30.0                               # the receiver's snr argument (UTSA law: snr_ls = snr_data = 10^(snr/20))
TAPS = np.array([1.0, 0.0, 0.0, 0.9]) / np.linalg.norm([1.0, 0.0, 0.0, 0.9])
LINE = 16                                    # complex64 samples per 128-byte line
WINDOW = (4, 12)
RUN = 12                                     # data symbols one work item of the demod kernel walks (CHANTRACK_RUN)


def slots(N):
    """work items per workgroup of the library's FFT plan (fft_core.hpp: 8 points per lane at 64-pt, else 16; 64 lanes at least)"""
    T = N // (8 if N == 64 else 16)
    return 1 if T >= 64 else 64 // T


def snr_lin(snr_arg=SNR_ARG):
    return 10.0 ** (snr_arg / 20.0)


def link_frame(seed, noise_var=None):
    """the link case -> dict(x complex128 [frame_len], bits uint8 [n_pat*D*Kd*2], tsr [t0 = cp, lag 0, 0, 1], frame_len)"""
    c = LINK
    N, cp = c["N"], c["cp"]
    S, D = c["synch_dat"]
    rng = np.random.default_rng(seed)
    n_sym = (S + D) * c["n_pat"]
    bits = rng.integers(0, 2, D * c["n_pat"] * c["Kd"] * 2).astype(np.uint8)
    tx = orc.tx_modulate(bits, N, cp, c["Ks"], c["Kd"], n_sym, synch_dat=c["synch_dat"], modulation=c["mod"])
    g = np.array(c["gains"]) / np.linalg.norm(c["gains"])
    n = np.arange(len(tx) + max(c["delays"]))
    y = np.zeros(len(n), complex)
    for gain, delay, sign in zip(g, c["delays"], (+1, -1)):
        path = np.zeros(len(n), complex)
        path[delay:delay + len(tx)] = gain * tx
        y += path * np.exp(sign * 2j * np.pi * c["doppler"] * n / N)
    nv = c["noise_var"] if noise_var is None else noise_var
    y = y + (rng.standard_normal(len(y)) + 1j * rng.standard_normal(len(y))) * np.sqrt(nv / 2)
    return dict(x=y, bits=bits, tsr=np.array([cp, 0, 0, 1], np.int32), frame_len=len(y))


def bit_errors(eq_rows, bits, mod="QPSK"):
    """hard decisions of rows [r][Kd] against the transmitted bits of the same rows"""
    got = orc.demap_hard(np.asarray(eq_rows).astype(np.complex64).ravel(), mod)
    return int(np.count_nonzero(got != np.asarray(bits).ravel()[:got.size]))


def make_batch(N, Ks, Kd, n_pat, seed, synch_dat=(1, 1), mod="QPSK", late=False, noise=(0.002, 0.02), drift=0.004, n_frames=None):
    """n = slots(N) + 1 frames (or n_frames) of n_pat patterns over the two-path channel -> dict(iq [n][stride] complex64, stride (odd), frame_len,
    tsr [n][4] int32, t0 [n], planted {frame: (kind, pattern)}).
      lag      LAGS in turn; t0 = (start of the first sync symbol's body) - lag, so the lag is the true one
      t0       every third frame on a 128-byte line of the buffer's first frame, the others off it
      drift    every frame turns by e^{j 2 pi drift n / N} with a sign and size of its own, so the estimates of a frame differ
      noise    variance noise[0] .. noise[1] across the frames
      planted  sync windows set to exact zeros in the frames with a sync, in this order as far as the batch has frames: one in the
               middle (pattern n_pat // 2), the last one, the one of pattern 0 (n_pat >= 3)
      one frame (n // 2) has no sync
      late     every frame starts 2L - N + 1 + (f % 3) samples later, so that frame_len can cut the last pattern's windows without
               the pattern count changing"""
    rng = np.random.default_rng(seed)
    cp = CP[N]
    S, D = synch_dat
    L, SD = N + cp, S + D
    n = slots(N) + 1 if n_frames is None else n_frames
    n_sym = SD * n_pat
    bps = {"QPSK": 2, "16QAM": 4, "64QAM": 6}[mod]
    t0 = np.zeros(n, int)
    tsr = np.zeros((n, 4), np.int32)
    frames, sent = [], []
    for f in range(n):
        lag = LAGS[(f + seed) % len(LAGS)]
        lead = (lag - cp) % LINE if f % 3 == 0 else (lag - cp) % LINE + 1 + (f % 5)
        if late:
            lead = 2 * L - N + 1 + (f % 3) - cp + lag
        bits = rng.integers(0, 2, D * n_pat * Kd * bps).astype(np.uint8)
        tx = orc.tx_modulate(bits, N, cp, Ks, Kd, n_sym, synch_dat=synch_dat, modulation=mod)
        y = np.convolve(tx, TAPS)
        y = y * np.exp(2j * np.pi * drift * (1 + f % 3) * (-1) ** f * np.arange(len(y)) / N)
        nv = noise[0] + (noise[1] - noise[0]) * f / max(n - 1, 1)
        x = np.zeros(lead + len(y), complex)
        x[lead:] = y
        x += (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) * np.sqrt(nv / 2)
        t0[f] = lead + cp - lag
        tsr[f] = [t0[f], lag, 40, 1]
        frames.append(x)
        sent.append(bits)
    frame_len = max(len(x) for x in frames)
    stride = frame_len + 3 + (frame_len % 2)                                # odd
    iq = np.zeros((n, stride), np.complex64)
    for f, x in enumerate(frames):
        iq[f, :len(x)] = x
    tsr[n // 2, 3] = 0
    planted = {}
    if n_pat >= 3:
        live = [f for f in range(n) if f != n // 2]
        for f, (kind, p) in zip(live, (("mid", n_pat // 2), ("last", n_pat - 1), ("first", 0))):
            w = t0[f] + L * SD * p
            iq[f, w:w + N] = 0
            planted[f] = (kind, p)
    return dict(iq=iq, stride=stride, frame_len=frame_len, tsr=tsr, t0=t0, n_pat=n_pat, planted=planted, bits=sent)


WIDE = 5                                     # frames of the second batch of the large plans


def standalone_cases():
    """(N, Ks, Kd, synch_dat, n_pat, n_frames) of the stand-alone call; n_frames None = slots(N) + 1.  Every FFT size with 17
    (1, 1) patterns (17 data symbols: a full run of 12 and a remainder); at 64-pt eight (1, 3) patterns (two full runs) and the
    other bin counts.  From 512-pt on slots(N) + 1 is 3 or 2 frames, one of them without a sync: too few for every lag, a t0 off
    the 128-byte line and all three planted erasures among the frames WITH a sync, so those sizes get a second batch of WIDE
    frames."""
    out = [(N, N - 2, N - 4, (1, 1), 17, None) for N in NFFTS]
    out += [(N, N - 2, N - 4, (1, 1), 17, WIDE) for N in NFFTS if slots(N) + 1 < WIDE - 1]
    out += [(64, 62, 60, (1, 3), 8, None), (64, 52, 48, (1, 1), 17, None), (64, 64, 64, (1, 1), 17, None), (64, 64, 60, (1, 3), 8, None)]
    return out
