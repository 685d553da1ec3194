#!/usr/bin/env python3
"""Rate of ofdm_combine_despread_frames (B branches combined per bin, then despread) next to the chain a user would have to make
from the earlier calls -- ofdm_combine_csi_frames (sym + weight) followed by ofdm_dft_despread_frames (llr) -- timed in the same
session on the same buffers.  The chain's weights are wrong for this waveform: it is a yardstick for time only.

  fused llr      : ofdm_combine_despread_frames, noise given, llr only   -- reads 8 B per branch, writes 4*bps B per symbol
  fused sym+llr  : the same with sym as well                             -- 8 B more written
  chain          : combine_csi_frames (sym, weight) + dft_despread_frames (llr, no channel state): both calls inside one pair of
                   events -- reads 8 B per branch, writes 8 + 4 B, reads 8 B again, writes 4*bps B per symbol
  every time as algorithmic bytes over 8 TB/s, the ratio fused llr / chain, and the min..max of every timed call over its median
  (run-to-run spread)

Device events around each call on one stream, 3 warm-up calls, median of --reps (15).  M = 1200, 240 rows per segment, B = 2 and
B = 4 with as many segments as keep the B input buffers at the 1180 MB of tools/despread_rate.py (256 and 128); QPSK, 16-QAM,
64-QAM.  Writes --out (profiles/mrc_despread_rate.txt) and prints the same lines."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

import torch  # noqa: E402

import ofdm_mi355x as om  # noqa: E402

HBM = 8.0e12
M, ROWS, UNITS = 1200, 240, 512


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


def run(mod, B, reps, bufs):
    bps = om._lib.MODULATION_BITS[mod]
    d_sym, d_out, d_w, d_llr, d_a = bufs
    n_seg = UNITS // B
    seg = ROWS * M
    n = n_seg * seg
    rx = om.RxEngine(8, 2048, 144, 2046, (1, 3), M, 30, 0.7, modulation=mod)
    rx.reserve_mrc_despread(M, B, n_seg)
    rx.reserve_mrc(B, n_seg, ROWS, M)
    rx.reserve_despread(M, n_seg)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = s.cuda_stream
    rho = rx.csi_rho
    nv = [1e-3] * B

    def chain():
        rx.combine_csi_frames(d_sym, B, n_seg, ROWS, M, seg, d_a, M, rho, mod, noise_var=nv, d_sym_out=d_out, d_weight=d_w, stream=ss)
        rx.dft_despread_frames(d_out, n_seg, ROWS, M, seg, None, 0, rho, mod, d_llr=d_llr, stream=ss)

    t = {}
    t["llr"] = timed(lambda: rx.combine_despread_frames(d_sym, B, n_seg, ROWS, M, seg, d_a, M, rho, mod, noise_var=nv, d_llr=d_llr,
                                                        stream=ss), s, reps)
    t["sym_llr"] = timed(lambda: rx.combine_despread_frames(d_sym, B, n_seg, ROWS, M, seg, d_a, M, rho, mod, noise_var=nv, d_sym_out=d_out,
                                                            d_llr=d_llr, stream=ss), s, reps)
    t["chain"] = timed(chain, s, reps)
    s.synchronize()
    by = dict(llr=n * (8 * B + 4 * bps), sym_llr=n * (8 * B + 8 + 4 * bps), chain=n * (8 * B + 12 + 8 + 4 * bps))
    spread = max(max(t[k][2] / t[k][0] - 1, 1 - t[k][1] / t[k][0]) for k in t)
    frac = {k: by[k] / t[k][0] / HBM for k in t}
    return ("M %d %-5s B %d, %d seg x %d rows (%4.0f MB of input symbols) | fused llr %7.3f ms (%.2f of 8 TB/s) | fused sym+llr %7.3f ms "
            "(%.2f) | chain combine_csi + despread %7.3f ms (%.2f) | ratio fused llr / chain %.2f | spread of the timed calls +-%.1f %%"
            % (M, mod, B, n_seg, ROWS, B * n * 8 / 1e6, t["llr"][0] * 1e3, frac["llr"], t["sym_llr"][0] * 1e3, frac["sym_llr"],
               t["chain"][0] * 1e3, frac["chain"], t["llr"][0] / t["chain"][0], spread * 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrc_despread_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    n_in = UNITS * ROWS * M                                  # input symbols of all branches
    n_out = n_in // 2                                        # output symbols at B = 2
    g = torch.Generator(device="cuda").manual_seed(5)
    bufs = (torch.randn(n_in * 2, dtype=torch.float32, device="cuda", generator=g) * 0.7,
            torch.empty(n_out * 2, dtype=torch.float32, device="cuda"), torch.empty(n_out, dtype=torch.float32, device="cuda"),
            torch.empty(n_out * 6, dtype=torch.float32, device="cuda"),
            torch.rand(UNITS * M, dtype=torch.float32, device="cuda", generator=g) * 2 + 0.02)
    lines = ["# tools/mrc_despread_rate.py --reps %d on %s; algorithmic bytes per output symbol: 8 B read per branch + 4*bps B (llr) + 8 B "
             "(sym) written; the chain writes and reads 8 B (sym) and writes 4 B (weight) more" % (a.reps, torch.cuda.get_device_name(0))]
    for B in (2, 4):
        for mod in ("QPSK", "16QAM", "64QAM"):
            lines.append(run(mod, B, a.reps, bufs))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
