"""The contract of include/ofdm_mi355x.h, "channel tracked across the sync symbols of a frame", written literally in fp64 NumPy,
step by step.  Shares no code with the library; np.fft is the transform.  The order of the sums is not restated: in fp64 it moves
the results by 1e-16, far below what the float32 library is held to."""
import numpy as np

HOLD, LINEAR = 0, 1                          # OFDM_TRACK_HOLD / OFDM_TRACK_LINEAR
FIRST = -1                                   # not a mode of the library: every symbol with a_0, what ofdm_rx_demod_frames does


def bins_p(num_bins, nfft):
    """binsP(K): [-K/2..-1, 1..K/2] + N mod N"""
    h = num_bins // 2
    return (np.array(list(range(-h, 0)) + list(range(1, h + 1)), dtype=np.int64) + nfft) % nfft


def zadoff_chu(Ks, root=23):
    """the receiver's preamble sequence for synch_S == 1 and an even Ks"""
    n = np.arange(Ks, dtype=np.float64)
    return np.exp(-1j * (2 * np.pi / Ks) * root * (n ** 2 / 2))


def patterns(frame_len, N, cp, S, D):
    if S != 1:
        raise ValueError("the stage needs synch_S == 1")
    return (frame_len // (N + cp)) // (S + D)


def window_ok(N, pre, post):
    return (pre, post) == (0, 0) or (pre >= 0 and post >= 1 and pre + post <= N)


def pattern_estimate(x, frame_len, w, lag, N, Ks, snr_ls, zc):
    """step 1 for the window starting at w -> a_p as an N-vector (zero outside the sync bins), or None if the pattern does not
    take part"""
    if not (0 <= w and w + N <= frame_len):                                  # a candidate lies inside the frame
        return None
    sb = bins_p(Ks, N)
    with np.errstate(all="ignore"):
        Y = np.fft.fft(np.asarray(x[w:w + N], dtype=np.complex128))
        y = Y[sb]
        E = float(np.sum(np.abs(y) ** 2))                                    # over the LIST (Ks == N counts bin N/2 twice)
        if not (np.isfinite(E) and E > 0):
            return None
        a_list = np.sqrt(Ks / E) * y * np.exp(2j * np.pi * lag * sb / N) * np.conj(zc) / (1.0 + 1.0 / snr_ls)
    a = np.zeros(N, dtype=np.complex128)
    a[sb] = a_list                                                           # a bin listed twice keeps its last entry
    return a


def delay_window(a, pre, post, Ks):
    """step 2: H' of steps 1-4 of the delay-window contract on one row"""
    N = a.size
    h = np.fft.ifft(a)
    n = np.arange(N)
    keep = (n < post) | (n >= N - pre)
    full = np.fft.fft(np.where(keep, h, 0.0))
    out = np.zeros(N, dtype=np.complex128)
    sb = bins_p(Ks, N)
    out[sb] = full[sb]
    return out


def neighbours(takes, p):
    """step 3: (lo, hi or None) of pattern p; pattern 0 takes part"""
    lo = max(q for q in range(p + 1) if takes[q])
    later = [q for q in range(p + 1, len(takes)) if takes[q]]
    return lo, (later[0] if later else None)


def symbol_estimate(a, takes, p, m, mode, S, D):
    """step 3: H of data symbol m of pattern p, and the weight used (None where there is no interpolation)"""
    if mode == FIRST:
        return a[0], None
    lo, hi = neighbours(takes, p)
    if mode == HOLD or hi is None:
        return a[lo], None
    SD = S + D
    s = p * SD + S + m
    w = float(np.float32(s - lo * SD) / np.float32((hi - lo) * SD))
    return a[lo] + w * (a[hi] - a[lo]), w


def track_frame(x, frame_len, tsr_row, mode, N, cp, S, D, Ks, Kd, snr_ls, rho, window=(0, 0), zc=None):
    """One frame -> dict(on, eq [n_pat*D][Kd], csi [n_pat*D][Kd], H_pat [n_pat][N], takes [n_pat] int, weight [n_pat*D] (nan where
    none), demod [n_pat] bool).  rho = 1/snr_data of the equaliser.  A frame without a sync, or whose pattern 0 does not take
    part: zero rows, csi 0, H_pat 0, takes 0."""
    if mode not in (HOLD, LINEAR, FIRST):
        raise ValueError("unknown mode")
    pre, post = window
    if not window_ok(N, pre, post):
        raise ValueError("window needs pre >= 0, post >= 1, pre + post <= nfft, or (0, 0)")
    zc = zadoff_chu(Ks) if zc is None else zc
    n_pat = patterns(frame_len, N, cp, S, D)
    L, SD = N + cp, S + D
    out = dict(on=False, eq=np.zeros((n_pat * D, Kd), complex), csi=np.zeros((n_pat * D, Kd)), H_pat=np.zeros((n_pat, N), complex),
               takes=np.zeros(n_pat, np.int32), weight=np.full(n_pat * D, np.nan), demod=np.zeros(n_pat, bool))
    if int(tsr_row[3]) != 1 or n_pat == 0:
        return out
    t0, lag = int(tsr_row[0]), int(tsr_row[1])
    a = [pattern_estimate(x, frame_len, t0 + L * SD * p, lag, N, Ks, snr_ls, zc) for p in range(n_pat)]     # 1
    if a[0] is None:
        return out
    takes = [ap is not None for ap in a]
    if (pre, post) != (0, 0):                                                # 2
        a = [delay_window(ap, pre, post, Ks) if ap is not None else None for ap in a]
    out["on"] = True
    out["takes"][:] = takes
    for p in range(n_pat):
        if takes[p]:
            out["H_pat"][p] = a[p]
    db = bins_p(Kd, N)
    x = np.asarray(x)
    for p in range(n_pat):
        ptr = t0 + L * (p * SD + 1)                                          # 4: the guard of ofdm_rx_demod_frames
        dem = ptr + N - 1 <= frame_len
        out["demod"][p] = dem
        for m in range(D):
            r = p * D + m
            H, w = symbol_estimate(a, takes, p, m, mode, S, D)               # 3
            if w is not None:
                out["weight"][r] = w
            Hd = H[db]
            out["csi"][r] = Hd.real * Hd.real + Hd.imag * Hd.imag            # 5
            if not dem:
                continue
            start = ptr + L * m
            seg = np.zeros(N, complex)                                       # samples outside [0, frame_len) read as zero
            i0, i1 = max(start, 0), min(start + N, frame_len)
            if i1 > i0:
                seg[i0 - start:i1 - start] = x[i0:i1]
            with np.errstate(all="ignore"):
                Y = np.fft.fft(seg)[db]
                P = np.sum(np.abs(Y) ** 2)
                out["eq"][r] = Y * np.sqrt(Kd / P) * np.conj(Hd) / (np.abs(Hd) ** 2 + float(rho)) * np.exp(2j * np.pi * lag * db / N)
    return out


def track_frames(iq, frame_len, tsr, mode, N, cp, S, D, Ks, Kd, snr_ls, rho, window=(0, 0)):
    """The stage over frames iq [n][>= frame_len] -> list of track_frame results"""
    zc = zadoff_chu(Ks)
    return [track_frame(iq[f], frame_len, tsr[f], mode, N, cp, S, D, Ks, Kd, snr_ls, rho, window, zc) for f in range(len(iq))]
