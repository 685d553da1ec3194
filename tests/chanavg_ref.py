"""The contract of include/ofdm_mi355x.h, "channel estimate averaged over every sync symbol of a frame", written literally in fp64
NumPy, step by step.  Shares no code with the library; np.fft is the transform.  The order of the sums is not restated: in fp64 it
moves the results by 1e-16, far below what the float32 library is held to."""
import numpy as np

CHUNK = 16                                   # OFDM_CHANAVG_CHUNK (the reference only reports it: see above)


def bins_p(num_bins, nfft):
    """binsP(K): [-K/2..-1, 1..K/2] + N mod N"""
    h = num_bins // 2
    return (np.array(list(range(-h, 0)) + list(range(1, h + 1)), dtype=np.int64) + nfft) % nfft


def zadoff_chu(Ks, root=23):
    """the receiver's preamble sequence for synch_S == 1 and an even Ks"""
    n = np.arange(Ks, dtype=np.float64)
    return np.exp(-1j * (2 * np.pi / Ks) * root * (n ** 2 / 2))


def patterns(frame_len, N, cp, S, D, n_avg):
    """P = min(n_avg, n_pat), n_avg == -1 meaning all"""
    if S != 1:
        raise ValueError("the stage needs synch_S == 1")
    if n_avg == 0 or n_avg < -1:
        raise ValueError("n_avg must be >= 1 or -1")
    n_pat = (frame_len // (N + cp)) // (S + D)
    return n_pat if n_avg < 0 else min(n_avg, n_pat)


def pattern_estimate(x, frame_len, w, lag, N, Ks, snr_ls, zc):
    """steps 2-5 for the window starting at w -> a_p as an N-vector (zero outside the sync bins), or None if the pattern is no
    candidate or its E_p is not finite and positive"""
    if not (0 <= w and w + N <= frame_len):                                   # 2
        return None
    sb = bins_p(Ks, N)
    with np.errstate(all="ignore"):
        Y = np.fft.fft(np.asarray(x[w:w + N], dtype=np.complex128))          # 3
        y = Y[sb]
        E = float(np.sum(np.abs(y) ** 2))                                    # 4: over the LIST (Ks == N counts bin N/2 twice)
        if not (np.isfinite(E) and E > 0):
            return None
        a_list = np.sqrt(Ks / E) * y * np.exp(2j * np.pi * lag * sb / N) * np.conj(zc) / (1.0 + 1.0 / snr_ls)   # 5
    a = np.zeros(N, dtype=np.complex128)
    a[sb] = a_list                                                           # a bin listed twice keeps its last entry
    return a


def average_frame(x, frame_len, tsr_row, n_avg, N, cp, S, D, Ks, Kd, snr_ls, rho, zc=None):
    """One frame -> dict(on, H [N], gain [Kd], spread, n_used, rot [P], a [P] list of per-pattern estimates or None, coh [P]).
    on == False: a row without a sync (or whose pattern 0 does not take part): H and gain are None, spread 0, n_used 0, rot 0.
    rho = 1/snr_data of the equaliser; coh[p] = |c_p| / (|a_p| |a_0|), the coherence the tests keep above 0.5."""
    zc = zadoff_chu(Ks) if zc is None else zc
    P = patterns(frame_len, N, cp, S, D, n_avg)
    off = dict(on=False, H=None, gain=None, spread=0.0, n_used=0, rot=np.zeros(P, complex), a=[None] * P, coh=np.zeros(P))
    if int(tsr_row[3]) != 1 or P == 0:
        return off
    t0, lag = int(tsr_row[0]), int(tsr_row[1])
    L, SD = N + cp, S + D
    a = [pattern_estimate(x, frame_len, t0 + L * SD * p, lag, N, Ks, snr_ls, zc) for p in range(P)]
    if a[0] is None:
        return off
    rot = np.zeros(P, complex)
    coh = np.zeros(P)
    rot[0], coh[0] = 1.0, 1.0
    d = [np.zeros(N, complex)]                                               # d_0 = 0
    for p in range(1, P):
        if a[p] is None:
            continue
        with np.errstate(all="ignore"):
            c = np.sum(a[p] * np.conj(a[0]))
            mag = abs(c)
        if not (np.isfinite(mag) and mag > 0):
            a[p] = None
            continue
        rot[p] = c / mag
        coh[p] = mag / (np.linalg.norm(a[p]) * np.linalg.norm(a[0]))
        d.append(np.conj(rot[p]) * a[p] - a[0])
    n = len(d)
    dsum = np.sum(d, axis=0)
    H = a[0] + dsum / n
    sb = bins_p(Ks, N)
    mask = np.zeros(N, bool)
    mask[sb] = True
    H[~mask] = 0.0
    spread = 0.0
    if n >= 2:
        spread = float((sum(np.sum(np.abs(dp) ** 2) for dp in d) - np.sum(np.abs(dsum) ** 2) / n) / ((n - 1) * Ks))
    db = bins_p(Kd, N)
    gain = np.conj(H[db]) / (np.abs(H[db]) ** 2 + float(rho)) * np.exp(2j * np.pi * lag * db / N)
    return dict(on=True, H=H, gain=gain, spread=spread, n_used=n, rot=rot, a=a, coh=coh)


def gain_of(H, lag, Kd, rho):
    """the gain expression on a given estimate row (the device's own Hbar, in the GPU test)"""
    H = np.asarray(H, dtype=np.complex128)
    N = H.size
    db = bins_p(Kd, N)
    return np.conj(H[db]) / (np.abs(H[db]) ** 2 + float(rho)) * np.exp(2j * np.pi * lag * db / N)


def average_frames(iq, frame_len, tsr, n_avg, N, cp, S, D, Ks, Kd, snr_ls, rho):
    """The stage over frames iq [n][>= frame_len] -> list of average_frame results"""
    zc = zadoff_chu(Ks)
    return [average_frame(iq[f], frame_len, tsr[f], n_avg, N, cp, S, D, Ks, Kd, snr_ls, rho, zc) for f in range(len(iq))]
