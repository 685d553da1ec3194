"""The delay-window channel-estimate denoising contract of include/ofdm_mi355x.h ("delay-window channel-estimate denoising")
written literally in fp64 NumPy, step by step.  Shares no code with the library; np.fft is the transform."""
import numpy as np


def bins_p(num_bins, nfft):
    """binsP(K): [-K/2..-1, 1..K/2] + N mod N"""
    h = num_bins // 2
    return (np.array(list(range(-h, 0)) + list(range(1, h + 1)), dtype=np.int64) + nfft) % nfft


def kept_taps(nfft, pre, post):
    """step 2: bool [N], True for n in [0, post) and [N - pre, N)"""
    if not (pre >= 0 and post >= 1 and pre + post <= nfft):
        raise ValueError("window needs pre >= 0, post >= 1, pre + post <= nfft")
    n = np.arange(nfft)
    return (n < post) | (n >= nfft - pre)


def window_row(H_ls, lag, pre, post, Ks, Kd, rho):
    """One row with a sync -> (H' [N] complex128, gain [Kd] complex128, tail float).  rho = 1/snr_data of the equaliser."""
    H_ls = np.asarray(H_ls, dtype=np.complex128)
    N = H_ls.size
    h = np.fft.ifft(H_ls)                                                    # 1
    keep = kept_taps(N, pre, post)                                           # 2
    M = N - pre - post
    tail = float(N) / M * float(np.sum(np.abs(h[~keep]) ** 2)) if M > 0 else 0.0   # 3
    full = np.fft.fft(np.where(keep, h, 0.0))                                # 4
    Hw = np.zeros(N, dtype=np.complex128)
    sb = bins_p(Ks, N)
    Hw[sb] = full[sb]
    db = bins_p(Kd, N)                                                       # 5
    hd = Hw[db]
    gain = np.conj(hd) / (np.abs(hd) ** 2 + float(rho)) * np.exp(2j * np.pi * float(lag) * db / N)
    return Hw, gain, tail


def window_rows(H_in, tsr, pre, post, Ks, Kd, rho, H_prev=None, gain_prev=None):
    """The stage over rows: H_in [n][N], tsr [n][4].  A row without a sync (tsr[3] != 1) keeps H_prev / gain_prev (step 6; NaN where
    none is given, so that a comparison cannot pass by accident) and gets tail 0.  -> H' [n][N], gain [n][Kd], tail [n], all fp64"""
    H_in = np.asarray(H_in)
    n, N = H_in.shape
    Hw = np.full((n, N), complex(np.nan, np.nan)) if H_prev is None else np.array(H_prev, dtype=np.complex128)
    g = np.full((n, Kd), complex(np.nan, np.nan)) if gain_prev is None else np.array(gain_prev, dtype=np.complex128)
    tail = np.zeros(n)
    for r in range(n):
        if int(tsr[r][3]) == 1:
            Hw[r], g[r], tail[r] = window_row(H_in[r], int(tsr[r][1]), pre, post, Ks, Kd, rho)
    return Hw, g, tail
