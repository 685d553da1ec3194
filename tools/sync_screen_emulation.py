#!/usr/bin/env python3
"""CPU emulation of the sliding energy sums of the screened sync search (csrc/rx_sync_scan.hpp) in fp32 and in the kernel's order
of operations, over the corpus of tests/sync_hostile_cases.py: how far the in-band energy E_j = N W_j - |sum x|^2 - |sum (-1)^n x|^2
of a screened trial can be from its fp64 value, in units of 2^-24 * hist_j (hist_j: N times the window energy at the anchor plus
all the energy that has entered since).  NumPy only; it follows a reading of the kernel, it is not the kernel:
it takes the anchor's own sums as correctly rounded and models no fused multiply-add, and what it predicts for the planted trials
of the corpus was NOT reproduced on an MI355X.

    python tools/sync_screen_emulation.py [N ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sync_hostile_cases as hc  # noqa: E402

f32 = np.float32
EPS = 2.0 ** -24


def geom(N, cp):
    """ScanGeom<N> restated: T, W (scan width), MX, BMAX, RMAX, B"""
    P = 8 if N == 64 else 16
    T = N // P
    QM = 2 if T >= 256 else 3 if T >= 128 else 4 if T >= 64 else 6 if T >= 32 else min(P, 12)
    BMAX = min(QM * T, 256)
    MX = 5 if T >= 256 else 3 if T >= 128 else 2 if T >= 64 else 1
    BX = MX * BMAX
    return dict(T=T, W=min(T, 64), MX=MX, BMAX=BMAX, RMAX=(BX + T - 1) // T, B=hc.scan_block(N, cp))


def cnorm2(z):
    return (z.real * z.real + z.imag * z.imag).astype(f32)   # (the compiler may fuse one product: half an ulp, not modelled)


def block_sums(x, N, cp, P0, nbx, G):
    """fp32 thresholds' energies of the trials P0 + 1 .. P0 + nbx - 1 of a block anchored at P0, as the kernel forms them.
    x: complex64 frame.  -> (ej32 [nbx - 1], nwj32 [nbx - 1], wbound32, ej64 [nbx - 1], hist32 [nbx - 1]); hist_j =
    N W_0 + N * (the energy that entered the window up to the end of the chunk of trials that j's lane owns) bounds every N W the
    sums passed through on their way to trial j"""
    T, W, RMAX = G["T"], G["W"], G["RMAX"]
    w0 = P0 + cp
    n = nbx - 1
    idx = np.arange(T * RMAX).reshape(T, RMAX)               # i = t * RMAX + r
    live = idx < n
    o = np.where(live, x[np.minimum(w0 + idx, len(x) - 1)], 0).astype(np.complex64)
    nn = np.where(live, x[np.minimum(w0 + N + idx, len(x) - 1)], 0).astype(np.complex64)
    sgn = np.where(idx & 1, 1.0, -1.0).astype(f32)
    dterm = (cnorm2(nn) - cnorm2(o)).astype(f32)
    aterm = (nn - o).astype(np.complex64)
    bterm = ((o - nn) * sgn).astype(np.complex64)
    dw, wadd = np.zeros(T, f32), np.zeros(T, f32)
    da, db = np.zeros(T, np.complex64), np.zeros(T, np.complex64)
    for r in range(RMAX):
        dw = (dw + dterm[:, r]).astype(f32)
        wadd = (wadd + cnorm2(nn[:, r])).astype(f32)
        da = (da + aterm[:, r]).astype(np.complex64)
        db = (db + bterm[:, r]).astype(np.complex64)
    # inclusive scan over the lanes of a wave (Hillis-Steele), then the totals of the waves before
    sw, swa, sa, sb = dw.copy(), wadd.copy(), da.copy(), db.copy()
    lane = np.arange(T) & (W - 1)
    dlt = 1
    while dlt < W:
        up = lambda v: np.concatenate([np.zeros(dlt, v.dtype), v[:-dlt]])
        m = lane >= dlt
        sw = np.where(m, (sw + up(sw)).astype(f32), sw)
        swa = np.where(m, (swa + up(swa)).astype(f32), swa)
        sa = np.where(m, (sa + up(sa)).astype(np.complex64), sa)
        sb = np.where(m, (sb + up(sb)).astype(np.complex64), sb)
        dlt <<= 1
    if T > 64:
        NW = T // 64
        tot = [(sw[w * 64 + 63], swa[w * 64 + 63], sa[w * 64 + 63], sb[w * 64 + 63]) for w in range(NW)]
        tot_add = f32(0)
        for w in range(NW):
            tot_add = f32(tot_add + tot[w][1])
            sel = (np.arange(T) >> 6) > w
            sw = np.where(sel, (sw + tot[w][0]).astype(f32), sw)
            swa = np.where(sel, (swa + tot[w][1]).astype(f32), swa)
            sa = np.where(sel, (sa + tot[w][2]).astype(np.complex64), sa)
            sb = np.where(sel, (sb + tot[w][3]).astype(np.complex64), sb)
    else:
        tot_add = swa[W - 1]
    pw = (sw - dw).astype(f32)
    pa, pb = (sa - da).astype(np.complex64), (sb - db).astype(np.complex64)
    # the anchor's exact trial supplies E_0, sum x and sum (-1)^n x (fp32 FFT: taken as the rounded fp64 values)
    win = x[w0:w0 + N].astype(np.complex128)
    alt = (-1.0) ** np.arange(N)
    y0, yh = np.complex64(win.sum()), np.complex64((win * alt).sum())
    e0 = f32(N * np.sum(np.abs(win) ** 2) - abs(win.sum()) ** 2 - abs((win * alt).sum()) ** 2)
    nw0 = f32(f32(e0 + cnorm2(y0)) + cnorm2(yh))
    wbound = f32(nw0 + f32(N) * tot_add)
    ej = np.zeros((T, RMAX), f32)
    nwj = np.zeros((T, RMAX), f32)
    hist = np.zeros((T, RMAX), f32)
    for r in range(RMAX):
        hist[:, r] = (nw0 + f32(N) * swa).astype(f32)            # through the END of the lane's chunk: its exclusive prefix is
                                                                 # formed as (inclusive - own total) and carries that rounding
        pw = (pw + dterm[:, r]).astype(f32)
        pa = (pa + aterm[:, r]).astype(np.complex64)
        pb = (pb + bterm[:, r]).astype(np.complex64)
        nwj[:, r] = (nw0 + f32(N) * pw).astype(f32)
        ej[:, r] = ((nwj[:, r] - cnorm2((y0 + pa).astype(np.complex64))).astype(f32) - cnorm2((yh + pb).astype(np.complex64))).astype(f32)
    # fp64 truth of the same trials
    xd = x.astype(np.complex128)
    c2 = np.concatenate([[0], np.cumsum(np.abs(xd) ** 2)])
    c1 = np.concatenate([[0], np.cumsum(xd)])
    ca = np.concatenate([[0], np.cumsum(xd * (-1.0) ** np.arange(len(xd)))])
    s = w0 + 1 + np.arange(n)
    e64 = N * (c2[s + N] - c2[s]) - np.abs(c1[s + N] - c1[s]) ** 2 - np.abs(ca[s + N] - ca[s]) ** 2
    return ej.ravel()[:n], nwj.ravel()[:n], wbound, e64, hist.ravel()[:n]


def survey(N, anchors_per_frame=24, seed=0):
    """-> rows (kind, level, worst |E32 - E64| / E64 over trials the two fixed guards trust, worst |E32 - E64| / (2^-24 hist_j),
    worst relative error where the new test trusts too)"""
    cp = hc.SIZES[N][0]
    G = geom(N, cp)
    B = G["B"]
    rng = np.random.default_rng(seed)
    rows = []
    for kind in hc.KINDS:
        b = hc.batch(N, kind)
        for lv in np.unique(b.level):
            worst_rel, worst_c, worst_rel_new = 0.0, 0.0, 0.0
            for f in np.nonzero(b.level == lv)[0]:
                hit = int(b.hit[f])
                cand = np.unique(np.concatenate([[0, max(0, hit - B + 1), (hit // B) * B, max(0, hit - 1)],
                                                 rng.integers(0, hit + 1, anchors_per_frame)]))
                for P0 in cand:
                    for nbx in sorted({B, (G["MX"] * B + B) // 2, G["MX"] * B}):
                        e32, nw32, wb, e64, hs = block_sums(b.iq[f], N, cp, int(P0), nbx, G)
                        upto = min(len(e32), hit + cp - int(P0))         # trials up to the end of the first sync symbol
                        if upto <= 0:
                            continue
                        e32, nw32, e64, hs = e32[:upto].astype(np.float64), nw32[:upto].astype(np.float64), e64[:upto], hs[:upto].astype(np.float64)
                        err = np.abs(e32 - e64)
                        worst_c = max(worst_c, float(np.max(err / (EPS * hs))))
                        trusted = (nw32 > hc.GUARD_NW * float(wb)) & (e32 > hc.GUARD_E * nw32) & (e64 > 0)
                        if trusted.any():
                            worst_rel = max(worst_rel, float(np.max(err[trusted] / e64[trusted])))
                        new = trusted & (SHARE * e32 > C * EPS * hs)
                        if new.any():
                            worst_rel_new = max(worst_rel_new, float(np.max(err[new] / e64[new])))
            rows.append((kind, float(lv), worst_rel, worst_c, worst_rel_new))
    return rows


C = 16.0                                                     # candidate bound: twice the largest factor the survey finds
SHARE = 1e-4                                                 # a quarter of the 4e-4 the 2e-4 margin is worth in |u|^2


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or sorted(hc.SIZES)
    print("# N kind level | worst rel. error of E_j where the two fixed guards trust it | worst error / (2^-24 hist_j) | worst rel. error where"
          " also %g E_j > %g 2^-24 hist_j" % (SHARE, C))
    for N in sizes:
        for kind, lv, rel, c, rel_new in survey(N):
            print("%5d %-8s %8g   %.2e   %6.2f   %.2e" % (N, kind, lv, rel, c, rel_new), flush=True)
