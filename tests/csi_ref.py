"""The channel-state-weighted LLR contract of include/ofdm_mi355x.h ("channel-state-weighted LLRs") written literally in NumPy
float32: every product, sum, difference and quotient is one float32 operation on float32 operands (NumPy rounds each on its own,
division correctly), sigma2 is the only double.  Shares no code with the library.  `dtype=np.float64` evaluates the same formulas
in fp64 for test_csi_ref_host.py."""
import math

import numpy as np

BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}
UNIT = {4: 0.31622776601683794, 6: 0.15430334996209191}


def _bps(mod):
    return BPS[mod] if isinstance(mod, str) else int(mod)


def levels(bps, dtype=np.float32):
    """-> (levels [M], labels [NB][M]): step 2 of the contract"""
    f = dtype
    if bps == 2:
        c = f(np.float32(0.70710678))
        return np.array([c, -c], dtype=f), np.array([[0, 1]], dtype=bool)
    M = 4 if bps == 4 else 8
    m = np.arange(M) * 2 - (M - 1)
    lv = (m.astype(np.float32) * np.float32(UNIT[bps])).astype(f)          # the library's float32 levels, also in the fp64 run
    am = np.abs(m)
    lab = [m < 0, am == 3] if bps == 4 else [m < 0, am > 4, (am == 1) | (am == 7)]
    return lv, np.array(lab, dtype=bool)


def _axis(x, bps, f):
    """step 3: d[j] per axis bit, and the smallest squared distance"""
    lv, lab = levels(bps, f)
    diff = (x[:, None] - lv[None, :]).astype(f)
    sq = (diff * diff).astype(f)
    d = np.stack([(np.min(sq[:, lab[j]], axis=1) - np.min(sq[:, ~lab[j]], axis=1)).astype(f) for j in range(lab.shape[0])], axis=1)
    return d, np.min(sq, axis=1)


def symbols(z, a, rho, mod, dtype=np.float32):
    """steps 1-4 and 6 for flat arrays z (complex), a (per symbol) -> usable [n] bool, d [n][bps], e [n] (0 where not usable),
    in_sum [n] bool (usable and e finite)"""
    f = dtype
    bps = _bps(mod)
    z = np.asarray(z).ravel()
    zr, zi = z.real.astype(f), z.imag.astype(f)
    a = np.asarray(a).ravel().astype(f)
    rho = f(rho)
    with np.errstate(all="ignore"):
        s = ((a + rho).astype(f) / a).astype(f)
        ur, ui = (zr * s).astype(f), (zi * s).astype(f)
        usable = (np.isfinite(a) & (a > 0) & np.isfinite(zr) & np.isfinite(zi) & ~((zr == 0) & (zi == 0)) & np.isfinite(s)
                  & np.isfinite(ur) & np.isfinite(ui))
        dr, mr = _axis(ur, bps, f)
        di, mi = _axis(ui, bps, f)
        d = np.empty((z.size, bps), dtype=f)
        d[:, 0::2] = dr
        d[:, 1::2] = di
        e = (a * (mr + mi).astype(f)).astype(f)
    in_sum = usable & np.isfinite(e)
    return usable, d, np.where(in_sum, e, f(0)), in_sum


def llr_from(usable, d, a, sigma2, dtype=np.float32):
    """step 5 for one segment: w_den = float(sigma2)"""
    f = dtype
    a = np.asarray(a).ravel().astype(f)
    with np.errstate(all="ignore"):
        w_den = f(sigma2)
        ok_w = bool(np.isfinite(w_den) and w_den > 0)
        w = (a / w_den).astype(f)
        v = (w[:, None] * d).astype(f)
    good = usable[:, None] & np.isfinite(v) & ok_w
    return np.where(good, v, f(0)).astype(f)


def demap_csi_segment(z, a_row, rho, mod, noise_var=None, dtype=np.float32):
    """One segment: z [rows][row_len] complex, a_row [row_len].  noise_var None: OFDM_CSI_NOISE_EST.  -> llr [rows*row_len*bps],
    sigma2 (Python float), n_used (int), e [n] float64 terms of the sum (for the tests' own summation)"""
    z = np.asarray(z)
    rows, row_len = z.shape
    a = np.tile(np.asarray(a_row)[:row_len], rows)
    usable, d, e, in_sum = symbols(z, a, rho, mod, dtype)
    terms = e[in_sum].astype(np.float64)
    if noise_var is None:
        n_used = int(in_sum.sum())
        sigma2 = math.fsum(terms) / n_used if n_used else 0.0
    else:
        n_used = int(usable.sum())
        sigma2 = float(noise_var)
    return llr_from(usable, d, a, sigma2, dtype).ravel(), sigma2, n_used, terms


def llr_with_sigma2(z, a_row, rho, mod, sigma2, dtype=np.float32):
    """The LLRs of a segment for a sigma2 that is given from outside (the device's own estimate)"""
    z = np.asarray(z)
    rows, row_len = z.shape
    a = np.tile(np.asarray(a_row)[:row_len], rows)
    usable, d, _, _ = symbols(z, a, rho, mod, dtype)
    return llr_from(usable, d, a, sigma2, dtype).ravel()


def csi_row(H, bins):
    """ofdm_rx_csi_frames: re*re + im*im in float32, each product rounded"""
    h = np.asarray(H)[np.asarray(bins)]
    re, im = h.real.astype(np.float32), h.imag.astype(np.float32)
    return ((re * re).astype(np.float32) + (im * im).astype(np.float32)).astype(np.float32)
