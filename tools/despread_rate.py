#!/usr/bin/env python3
"""Rate of the DFT-spread OFDM stages (ofdm_dft_despread_frames, ofdm_tx_dft_spread) next to ofdm_demap_csi_frames with the noise
given (llr only), timed in the same session on the same buffers.

  despread llr      : ofdm_dft_despread_frames, noise given, llr only      -- reads 8 B, writes 4*bps B per symbol
  despread sym+llr  : the same with sym as well                            -- reads 8 B, writes 8 + 4*bps B per symbol
  precoder          : ofdm_tx_dft_spread out of place                      -- reads 8 B, writes 8 B per symbol
  demap_csi (given) : ofdm_demap_csi_frames, noise given, llr only         -- reads 8 B, writes 4*bps B per symbol (the yardstick)
  every time as algorithmic bytes over 8 TB/s, the ratio despread llr / demap_csi, and the min..max of every timed call over its
  median (run-to-run spread)

Device events around each call on one stream, 3 warm-up calls, median of --reps (15).  The 2048-pt numerology: M = 1200, 512
segments (frames) of 240 rows (data symbols) of random equalised symbols with random channel powers; QPSK, 16-QAM, 64-QAM.
Not timed: the composite calls (their other stages have their own records), hard bits, sizes other than 1200, the per-segment
table launch on its own (it is inside every despread time).  Writes --out (profiles/despread_rate.txt) and prints the same lines."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

import torch  # noqa: E402

import ofdm_mi355x as om  # noqa: E402

HBM = 8.0e12
M, N_SEG, ROWS = 1200, 512, 240


def timed(fn, s, reps):
    """-> (median, min, max) seconds"""
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        s.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / 1e3)
    return statistics.median(ms), min(ms), max(ms)


def run(mod, reps, bufs):
    bps = om._lib.MODULATION_BITS[mod]
    d_sym, d_out, d_llr, d_a = bufs
    seg = ROWS * M
    n = N_SEG * seg
    rx = om.RxEngine(8, 2048, 144, 2046, (1, 3), M, 30, 0.7, modulation=mod)
    tx = om.TxEngine(2048, 144, 2046, M, (1, 3), mod)
    rx.reserve_despread(M, N_SEG)
    rx.reserve_csi(N_SEG, ROWS, M)
    tx.reserve_spread(M)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = s.cuda_stream
    rho = rx.csi_rho
    t = {}
    t["llr"] = timed(lambda: rx.dft_despread_frames(d_sym, N_SEG, ROWS, M, seg, d_a, M, rho, mod, d_llr=d_llr,
                                                    noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=1e-3, stream=ss), s, reps)
    t["sym_llr"] = timed(lambda: rx.dft_despread_frames(d_sym, N_SEG, ROWS, M, seg, d_a, M, rho, mod, d_sym_out=d_out, d_llr=d_llr,
                                                        noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=1e-3, stream=ss), s, reps)
    t["pre"] = timed(lambda: tx.dft_spread(d_sym, N_SEG * ROWS, M, d_out, stream=ss), s, reps)
    t["csi"] = timed(lambda: rx.demap_csi_frames(d_sym, N_SEG, ROWS, M, seg, d_a, M, rho, mod, d_llr, noise_mode=om.CSI_NOISE_GIVEN,
                                                 noise_var=1e-3, stream=ss), s, reps)
    s.synchronize()
    by = dict(llr=n * (8 + 4 * bps), sym_llr=n * (16 + 4 * bps), pre=n * 16, csi=n * (8 + 4 * bps))
    spread = max(max(t[k][2] / t[k][0] - 1, 1 - t[k][1] / t[k][0]) for k in t)
    frac = {k: by[k] / t[k][0] / HBM for k in t}
    return ("M %d %-5s %d seg x %d rows (%4.0f MB of symbols) | despread llr %7.3f ms (%.2f of 8 TB/s) | sym+llr %7.3f ms (%.2f) | "
            "precoder %7.3f ms (%.2f) | demap_csi_frames given, llr %7.3f ms (%.2f) | ratio despread/demap_csi %.2f | "
            "spread of the timed calls +-%.1f %%" % (M, mod, N_SEG, ROWS, n * 8 / 1e6, t["llr"][0] * 1e3, frac["llr"], t["sym_llr"][0] * 1e3,
                                                     frac["sym_llr"], t["pre"][0] * 1e3, frac["pre"], t["csi"][0] * 1e3, frac["csi"],
                                                     t["llr"][0] / t["csi"][0], spread * 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "despread_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    n = N_SEG * ROWS * M
    g = torch.Generator(device="cuda").manual_seed(5)
    bufs = (torch.randn(n * 2, dtype=torch.float32, device="cuda", generator=g) * 0.7,
            torch.empty(n * 2, dtype=torch.float32, device="cuda"), torch.empty(n * 6, dtype=torch.float32, device="cuda"),
            torch.rand(N_SEG * M, dtype=torch.float32, device="cuda", generator=g) * 2 + 0.02)
    lines = ["# tools/despread_rate.py --reps %d on %s; algorithmic bytes per symbol: 8 B read + 4*bps B (llr) + 8 B (sym) written; "
             "precoder 8 B + 8 B" % (a.reps, torch.cuda.get_device_name(0))]
    for mod in ("QPSK", "16QAM", "64QAM"):
        lines.append(run(mod, a.reps, bufs))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
