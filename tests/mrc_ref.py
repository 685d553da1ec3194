"""The receive-diversity combining contract of include/ofdm_mi355x.h ("receive-diversity combining") written literally in NumPy
float32: every product, sum, difference and quotient is one float32 operation on float32 operands (NumPy rounds each on its own,
division correctly), the noise variances are the only doubles.  Shares no code with the library; levels and the axis rule come
from csi_ref.  `dtype=np.float64` evaluates the same formulas in fp64 for test_mrc_ref_host.py."""
import numpy as np

import csi_ref

BPS = csi_ref.BPS


def entries(a, rho, sigma2, dtype=np.float32):
    """step 1 for one unit: a [row_len], sigma2 a double -> c [row_len], t [row_len], usable [row_len]"""
    f = dtype
    a = np.asarray(a).astype(f)
    rho = f(rho)
    with np.errstate(all="ignore"):
        w_den = f(sigma2)
        c = ((a + rho).astype(f) / w_den).astype(f)
        t = (a / w_den).astype(f)
        usable = (np.isfinite(a) & (a > 0) & bool(np.isfinite(w_den) and w_den > 0) & np.isfinite(c) & np.isfinite(t) & (t > 0))
    return c, t, usable


def combine(z, a, rho, mod, sigma2, dtype=np.float32):
    """One output segment.  z [B][rows][row_len] complex (the branches' equalised symbols), a [B][row_len] channel powers, sigma2
    [B] doubles (the variance of each branch's unit) -> llr [rows*row_len*bps], sym [rows*row_len] complex, weight [rows*row_len],
    took_part [B][rows*row_len] bool"""
    f = dtype
    c_t = np.complex64 if f == np.float32 else np.complex128
    bps = csi_ref._bps(mod)
    z = np.asarray(z)
    B, rows, row_len = z.shape
    n = rows * row_len
    Nr, Ni, A = np.zeros(n, f), np.zeros(n, f), np.zeros(n, f)         # step 3: the sums start from +0
    any_in = np.zeros(n, bool)
    took = np.zeros((B, n), bool)
    with np.errstate(all="ignore"):
        for b in range(B):                                              # branch order 0 .. B-1
            c, t, ent = entries(np.asarray(a[b])[:row_len], rho, float(sigma2[b]), f)
            c, t, ent = np.tile(c, rows), np.tile(t, rows), np.tile(ent, rows)
            zr, zi = z[b].real.astype(f).ravel(), z[b].imag.astype(f).ravel()
            pr, pi = (zr * c).astype(f), (zi * c).astype(f)             # step 2
            part = ent & np.isfinite(zr) & np.isfinite(zi) & ~((zr == 0) & (zi == 0)) & np.isfinite(pr) & np.isfinite(pi)
            Nr = np.where(part, (Nr + pr).astype(f), Nr)                # a branch that does not take part leaves the sums
            Ni = np.where(part, (Ni + pi).astype(f), Ni)
            A = np.where(part, (A + t).astype(f), A)
            any_in |= part
            took[b] = part
        ur, ui = (Nr / A).astype(f), (Ni / A).astype(f)                 # step 4: usable only after the divisions
        usable = any_in & np.isfinite(A) & (A > 0) & np.isfinite(ur) & np.isfinite(ui)
        dr, _ = csi_ref._axis(ur, bps, f)                               # step 5
        di, _ = csi_ref._axis(ui, bps, f)
        d = np.empty((n, bps), dtype=f)
        d[:, 0::2] = dr
        d[:, 1::2] = di
        v = (A[:, None] * d).astype(f)                                  # step 6
    llr = np.where(usable[:, None] & np.isfinite(v), v, f(0)).astype(f).ravel()
    sym = np.zeros(n, c_t)
    sym.real = np.where(usable, ur, f(0))
    sym.imag = np.where(usable, ui, f(0))
    weight = np.where(usable, A, f(0)).astype(f)
    return llr, sym, weight, took


def combine_segments(z, a, rho, mod, sigma2, dtype=np.float32):
    """The branch-major batch: z [B][n_seg][rows][row_len], a [B][n_seg][row_len], sigma2 [B][n_seg] (per unit) or [B] (one per
    branch: OFDM_MRC_NOISE_GIVEN) -> llr [n_seg][rows*row_len*bps], sym [n_seg][rows*row_len], weight [n_seg][rows*row_len]"""
    z, a = np.asarray(z), np.asarray(a)
    B, n_seg = z.shape[:2]
    s2 = np.asarray(sigma2, np.float64)
    if s2.ndim == 1:
        s2 = np.repeat(s2[:, None], n_seg, axis=1)
    out = [combine(z[:, s], a[:, s], rho, mod, s2[:, s], dtype) for s in range(n_seg)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
