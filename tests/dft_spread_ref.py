"""The DFT-spread OFDM contract of include/ofdm_mi355x.h ("DFT-spread OFDM") restated in fp64 NumPy: transform precoding, the
entry mask, the inverse transform, the per-segment weights and the outputs.  Shares no code with the library.  What the contract
states as a function of the device's OWN stored float32 values (llr and bits from sym and weight) is outputs_from()."""
import math

import numpy as np

import csi_ref

BPS = csi_ref.BPS


def size_ok(M):
    if M < 1 or M > 4096:
        return False
    for p in (2, 3, 5):
        while M % p == 0:
            M //= p
    return M == 1


def spread(x):
    """transform precoding of rows [.., M]: DFT / sqrt(M) in fp64"""
    x = np.asarray(x, np.complex128)
    return np.fft.fft(x, axis=-1) / math.sqrt(x.shape[-1])


def inverse(z):
    z = np.asarray(z, np.complex128)
    return np.fft.ifft(z, axis=-1) * math.sqrt(z.shape[-1])


def usable_entries(a_row):
    a = np.asarray(a_row, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (a > 0)


def masked(z, a_row=None):
    """step 1: z' [rows][M] complex128 (exactly the float32 values or 0)"""
    z = np.asarray(z, np.complex64)
    ok = np.isfinite(z.real) & np.isfinite(z.imag)
    if a_row is not None:
        ok = ok & usable_entries(a_row)[None, :]
    return np.where(ok, z, 0).astype(np.complex128)


def weights(a_row, rho, sigma2):
    """step 3 -> dict(beta, nu, w doubles; usable; beta32, inv32, weight32 the float32 values the device holds)"""
    a32 = np.asarray(a_row, np.float32)
    M = a32.size
    ok = usable_entries(a32)
    a = a32.astype(np.float64)
    rho = float(np.float32(rho))
    with np.errstate(all="ignore"):
        b = np.where(ok, a / (a + rho), 0.0)
        beta = math.fsum(b) / M
        noise = np.where(ok, float(sigma2) * a / ((a + rho) * (a + rho)), 0.0)
        terms = (b - beta) ** 2 + noise
        nu = math.fsum(terms) / M if np.isfinite(terms).all() else float(np.sum(terms)) / M
        w = beta * beta / nu if nu != 0 else math.inf
        good = all(math.isfinite(v) and v > 0 for v in (beta, nu, w))
        inv32 = np.float32(1.0 / beta) if beta != 0 else np.float32(np.inf)
        w32 = np.float32(w)
        usable = bool(good and np.isfinite(inv32) and np.isfinite(w32))
    z = np.float32(0)
    return dict(beta=beta, nu=nu, w=w, usable=usable, beta32=np.float32(beta) if usable else z, inv32=inv32 if usable else z,
                weight32=w32 if usable else z)


def despread_segment(z, a_row, rho, sigma2):
    """One segment: z [rows][M] complex64, a_row [M] or None (the plain inverse transform) -> sym [rows][M] complex128 (the
    contract's u in fp64, +0 for erasures and unusable segments), the weights dict, erased [rows] bool"""
    z = np.asarray(z, np.complex64)
    zp = masked(z, a_row)
    erased = ~np.any(zp != 0, axis=1)
    wt = weights(a_row, rho, sigma2) if a_row is not None else dict(beta=1.0, nu=1.0, w=1.0, usable=True, beta32=np.float32(1),
                                                                    inv32=np.float32(1), weight32=np.float32(1))
    u = inverse(zp) * float(wt["inv32"])
    u[erased] = 0
    if not wt["usable"]:
        u[:] = 0
    return u, wt, erased


def outputs_from(sym, weight32, mod):
    """step 4 from the device's own stored sym (complex64, flat) and weight (float32): llr [n*bps] float32 (every product rounded
    on its own, +0 where not finite) and hard bits [n*bps] uint8 (ofdm_demap's rule)"""
    from oracle import ofdm_oracle as orc
    bps = csi_ref._bps(mod)
    sym = np.asarray(sym, np.complex64).ravel()
    f = np.float32
    with np.errstate(all="ignore"):
        dr, _ = csi_ref._axis(sym.real.astype(f), bps, f)
        di, _ = csi_ref._axis(sym.imag.astype(f), bps, f)
        d = np.empty((sym.size, bps), dtype=f)
        d[:, 0::2] = dr
        d[:, 1::2] = di
        v = (f(weight32) * d).astype(f)
    llr = np.where(np.isfinite(v) & (v != 0) & (sym != 0)[:, None], v, f(0)).astype(f).ravel()
    name = {2: "QPSK", 4: "16QAM", 6: "64QAM"}[bps]
    return llr, np.asarray(orc.demap_hard(sym, name), np.uint8).ravel()


def pack_bits(bits):
    return np.packbits(np.asarray(bits, np.uint8))
