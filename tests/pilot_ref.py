"""fp64 restatement of the pilot-aided phase-tracking stage (include/ofdm_mi355x.h, "pilot-aided phase tracking") and the
frame builder its tests share.  No reference code exists for the stage: this file IS the contract the GPU is held against.

Receive-side convention: a row holds the K OCCUPIED bins in the list order of bins_p(K, nfft); n_pilots of them are pilots
(signed bin offsets), Kd' = K - n_pilots data entries remain, in list order."""
import numpy as np

from oracle import ofdm_oracle as orc

CPE, CPE_SLOPE = 0, 1


def layout(K, locations):
    """-> (pidx, pk, didx, dk): ascending list indices of the pilots, their signed offsets, the same for the data entries."""
    K = int(K)
    h = K // 2
    offs = np.array(list(range(-h, 0)) + list(range(1, h + 1)), dtype=np.int64)          # offset of list index i
    loc = [int(x) for x in locations]
    assert len(set(loc)) == len(loc) and all(x != 0 and -h <= x <= h for x in loc), "bad pilot locations"
    pidx = np.sort(np.array([x + h if x < 0 else h + x - 1 for x in loc], dtype=np.int64))
    mask = np.ones(K, bool)
    mask[pidx] = False
    didx = np.nonzero(mask)[0]
    return pidx, offs[pidx], didx, offs[didx]


def track_rows(z, locations, pilot_value=1.0 + 0j, mode=CPE, data_offsets=None):
    """z [..., K] -> dict(data [..., Kd'], cpe [...], slope [...], U [...], usable [...]) in fp64.  Only the decision "usable" is
    taken as the contract takes it, on |U|^2 = ur*ur + ui*ui evaluated in float32: a pilot sum whose square overflows float32 or
    underflows it to 0 is not usable.  data_offsets replaces the data entries' bin offsets (tests that show what a wrong offset
    does to their inputs)."""
    z = np.asarray(z).astype(np.complex128)
    K = z.shape[-1]
    pidx, pk, didx, dk = layout(K, locations)
    if data_offsets is not None:
        dk = np.asarray(data_offsets, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return _track(z, pidx, pk, didx, dk, pilot_value, mode)


def _track(z, pidx, pk, didx, dk, pilot_value, mode):
    pv = complex(pilot_value)
    w = z[..., pidx] * np.conj(pv)
    U = np.zeros(z.shape[:-1], np.complex128)
    for p in range(len(pidx)):                                       # ascending p
        U = U + w[..., p]
    ur, ui = U.real.astype(np.float32), U.imag.astype(np.float32)
    n2f = ur * ur + ui * ui                                          # the contract's |U|^2: float32, may overflow or underflow to 0
    n2 = U.real ** 2 + U.imag ** 2
    usable = np.isfinite(n2f) & (n2f > 0)
    mag = np.sqrt(np.where(usable, n2, 1.0))
    c = np.where(usable, np.conj(U) / mag, 1.0 + 0j)
    cpe = np.where(usable, U / mag, 0j)
    slope = np.zeros(z.shape[:-1])
    rot = c[..., None] * np.ones(len(didx))
    if mode == CPE_SLOPE:
        assert len(pidx) >= 2
        theta = np.angle(w * c[..., None])
        kbar = pk.mean()
        tau = ((pk - kbar) * theta).sum(axis=-1) / ((pk - kbar) ** 2).sum()
        delta = theta.mean(axis=-1) - tau * kbar
        tau = np.where(usable, tau, 0.0)
        delta = np.where(usable, delta, 0.0)
        slope = tau
        rot = c[..., None] * np.exp(-1j * (delta[..., None] + tau[..., None] * dk))
    return dict(data=rot * z[..., didx], cpe=cpe, slope=slope, U=np.where(usable, U, 0j), usable=usable)


def cfo_estimate(U, usable, rows_per_pattern, nfft, cp_len):
    """U, usable: [rows] of ONE segment -> carrier offset in subcarrier spacings (NaN without any pair)."""
    acc, n = 0j, 0
    for s in range(len(U) - 1):                                      # ascending s
        if s % rows_per_pattern == rows_per_pattern - 1 or not (usable[s] and usable[s + 1]):
            continue
        acc += U[s + 1] * np.conj(U[s])
        n += 1
    if n == 0:
        return float("nan")
    return float(np.angle(acc) / (2 * np.pi * (nfft + cp_len) / nfft))


def hard_bits(data, modulation):
    """the project's hard decision of the float32-stored data, one bit per byte, [b0, b1, ..] per symbol"""
    return orc.demap_hard(np.asarray(data).astype(np.complex64).ravel(), modulation)


# ------------------------------------------------------------------------------------------ frames with pilots
def make_frame(nfft, cp, K, locations, modulation, n_sym, eps, noise, seed, lead=7, pilot_value=1.0 + 0j, frame_len=None,
               sync_every=3, row_phase=None, row_slope=None):
    """One frame: random bits -> map -> OFDM_Modulation grid with pilots -> IFFT -> CP -> SynchDataMux (ZC root 23) -> reference
    channel -> `lead` samples in front -> carrier offset eps (subcarrier spacings; x[n] e^{j 2 pi eps n / N} in fp64) -> complex
    noise of standard deviation `noise` per component.  row_phase [n_data] / row_slope [n_data] (radians, radians per bin) rotate
    the grid rows before the IFFT (known per-row rotations for the restatement's own tests).
    -> (iq complex128 [frame_len], bits uint8 [n_data * Kd' * bps])"""
    rng = np.random.default_rng(seed)
    L = nfft + cp
    Kd = K - len(locations)
    bps = orc.BITS_PER_SYMBOL[modulation]
    n_data = n_sym // (1 + sync_every) * sync_every
    bits = rng.integers(0, 2, n_data * Kd * bps).astype(np.uint8)
    sym = orc.map_bits(bits, modulation).reshape(n_data, Kd)
    grid = orc.tx_stage_grid(sym, nfft, Kd, locations, pilot_value)
    if row_phase is not None or row_slope is not None:
        k = np.fft.fftfreq(nfft, 1.0 / nfft)                          # signed offset of every bin
        ph = np.zeros((n_data, nfft))
        if row_phase is not None:
            ph = ph + np.asarray(row_phase)[:, None]
        if row_slope is not None:
            ph = ph + np.asarray(row_slope)[:, None] * k[None, :]
        grid = grid * np.exp(1j * ph)
    rows = orc.tx_stage_cp(orc.tx_stage_ifft(grid), cp)
    tx = orc.tx_stage_mux(rows, nfft, cp, 23, sync_every, nfft - 2).ravel()
    x = np.concatenate([np.zeros(lead), orc.channel_apply(tx, orc.REF_TAPS, nfft)])
    fl = frame_len or n_sym * L + cp
    x = np.concatenate([x, np.zeros(max(0, fl - len(x)))])[:fl]
    x = x * np.exp(2j * np.pi * eps * np.arange(fl) / nfft)
    x = x + noise * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))
    return x, bits


def oracle_rows(iq, nfft, cp, K, n_sym, snr=100, sync_dat=(1, 3)):
    """rows [n_data][K] of a fresh fp64 RxOracle on one frame (rows 3, 7, .. of est_data_freq dropped, as the block does)"""
    S, D = sync_dat
    o = orc.RxOracle(n_sym, nfft, cp, nfft - 2, [S, D], K, snr, 0.7, force_fp64=True)
    o.work(np.asarray(iq), np.zeros(len(iq), np.complex128))
    keep = [r for r in range(n_sym) if r % (S + D) != D]
    return o.est_data_freq[keep][:n_sym // (S + D) * D]
