"""The contract "receive diversity for DFT-spread OFDM" of include/ofdm_mi355x.h restated in NumPy: steps 1-4 (the combiner's
entries, the takes-part rule, the sums in branch order and the MMSE division) literally in float32, every operation rounded on
its own, in the manner of mrc_ref.py (whose step 1 is reused); the inverse transform and the per-row weights in fp64 with
math.fsum.  What the contract states as a function of the device's OWN stored float32 values (llr and bits from sym and the
row's weight) is dft_spread_ref.outputs_from.  Shares no code with the library."""
import math

import numpy as np

import dft_spread_ref
import mrc_ref

BPS = mrc_ref.BPS
outputs_from = dft_spread_ref.outputs_from
pack_bits = dft_spread_ref.pack_bits


def combine_rows(z, a, rho, sigma2):
    """Steps 1-4 of one output segment.  z [B][rows][M] complex64, a [B][M] channel powers, sigma2 [B] doubles ->
    v [rows][M] complex64, A [rows][M] float32 (0 where the symbol is not combined), took [B][rows][M] bool"""
    f = np.float32
    z = np.asarray(z, np.complex64)
    B, rows, M = z.shape
    n = rows * M
    Nr, Ni, A = np.zeros(n, f), np.zeros(n, f), np.zeros(n, f)         # step 3: the sums start from +0
    any_in = np.zeros(n, bool)
    took = np.zeros((B, n), bool)
    with np.errstate(all="ignore"):
        for b in range(B):                                              # branch order 0 .. B-1
            c, t, ent = mrc_ref.entries(np.asarray(a[b])[:M], rho, float(sigma2[b]), f)       # step 1
            c, t, ent = np.tile(c, rows), np.tile(t, rows), np.tile(ent, rows)
            zr, zi = z[b].real.astype(f).ravel(), z[b].imag.astype(f).ravel()
            pr, pi = (zr * c).astype(f), (zi * c).astype(f)             # step 2
            part = ent & np.isfinite(zr) & np.isfinite(zi) & ~((zr == 0) & (zi == 0)) & np.isfinite(pr) & np.isfinite(pi)
            Nr = np.where(part, (Nr + pr).astype(f), Nr)
            Ni = np.where(part, (Ni + pi).astype(f), Ni)
            A = np.where(part, (A + t).astype(f), A)
            any_in |= part
            took[b] = part
        den = (A + f(1.0)).astype(f)                                    # step 4
        vr, vi = (Nr / den).astype(f), (Ni / den).astype(f)
        combined = any_in & np.isfinite(A) & (A > 0) & np.isfinite(vr) & np.isfinite(vi)
    v = np.zeros(n, np.complex64)
    v.real = np.where(combined, vr, f(0))
    v.imag = np.where(combined, vi, f(0))
    return v.reshape(rows, M), np.where(combined, A, f(0)).astype(f).reshape(rows, M), took.reshape(B, rows, M)


def row_weights(A_row, erased=False):
    """step 6 for one row: A_row [M] float32 (0 where not combined) -> dict(beta, eps, w doubles; usable; beta32, inv32,
    weight32 the float32 values the device holds, +0 where the row is not usable)"""
    A = np.asarray(A_row, np.float32).astype(np.float64)
    M = A.size
    b = A / (A + 1.0)
    e = 1.0 / (A + 1.0)
    beta, eps = math.fsum(b) / M, math.fsum(e) / M
    with np.errstate(all="ignore"):
        w = beta / eps if eps != 0 else math.inf
        good = all(math.isfinite(x) and x > 0 for x in (beta, eps, w))
        inv32 = np.float32(1.0 / beta) if beta != 0 else np.float32(np.inf)
        w32 = np.float32(w)
    usable = bool(good and np.isfinite(inv32) and np.isfinite(w32) and not erased)
    z = np.float32(0)
    return dict(beta=beta, eps=eps, w=w, usable=usable, beta32=np.float32(beta) if usable else z, inv32=inv32 if usable else z,
                weight32=w32 if usable else z)


def despread_rows(v, A):
    """Steps 5-7 on the float32 v of step 4: -> x [rows][M] complex128 (the transform alone), u [rows][M] complex128 (the
    contract's u in fp64, +0 for rows that are not usable), the rows' weight dicts, erased [rows] bool"""
    v = np.asarray(v, np.complex64)
    erased = ~np.any(v != 0, axis=1)
    x = dft_spread_ref.inverse(v.astype(np.complex128))
    wts = [row_weights(A[r], bool(erased[r])) for r in range(v.shape[0])]
    u = x * np.array([float(wt["inv32"]) for wt in wts])[:, None]
    for r, wt in enumerate(wts):
        if not wt["usable"]:
            u[r] = 0
    return x, u, wts, erased


def combine_despread_segment(z, a, rho, sigma2):
    """One output segment: z [B][rows][M], a [B][M], sigma2 [B] -> dict(comb [rows][M] complex64, A [rows][M] float32, x, sym
    [rows][M] complex128, beta32 and weight32 [rows] float32, usable and erased [rows] bool, wts the rows' dicts)"""
    v, A, took = combine_rows(z, a, rho, sigma2)
    x, u, wts, erased = despread_rows(v, A)
    return dict(comb=v, A=A, took=took, x=x, sym=u, wts=wts, erased=erased,
                beta32=np.array([wt["beta32"] for wt in wts], np.float32), weight32=np.array([wt["weight32"] for wt in wts], np.float32),
                usable=np.array([wt["usable"] for wt in wts], bool))


def segment_llr(seg, mod):
    """llr [rows*M*bps] float32 and hard bits of a restated segment, from its own sym rounded to float32"""
    rows = seg["sym"].shape[0]
    out = [outputs_from(seg["sym"][r].astype(np.complex64), seg["weight32"][r], mod) for r in range(rows)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
