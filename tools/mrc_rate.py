#!/usr/bin/env python3
"""Rate of the receive-diversity combiner (ofdm_combine_csi_frames) next to the channel-state-weighted LLR stage
(ofdm_demap_csi_frames) over one branch, measured in the same session on the same buffers.

  combiner : combine_csi_frames, noise given, llr only, B = 2 and 4 branches -- 8*B + 4*bps algorithmic bytes per output symbol
  csi      : demap_csi_frames, noise given, llr only, over branch 0 -- 8 + 4*bps bytes per symbol: the yardstick
  fraction : algorithmic bytes / time / 8 TB/s; spread: the min..max of every timed call over its median (run to run)

Device events around each call on one stream, 3 warm-up calls, median of --reps (15).  The branches' frames come from the device
transmitter and the reference 5-tap channel with a noise seed per branch, demodulated by one demod_frames call over all of them.
2048-pt 144/1200 with QPSK / 16-QAM / 64-QAM, 512 output frames of 320 symbols (240 data symbols).  Writes --out
(profiles/mrc_rate.txt) and prints the same lines."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ofdm_mi355x as om  # noqa: E402

HBM = 8.0e12
TAPS = np.array([0.3977, 0.7954 - 0.3977j, -0.1988, 0.0994, -0.0398])           # the reference channel (TX:64)
CONFIGS = [(2048, 144, 1200, "QPSK", 512, 320), (2048, 144, 1200, "16QAM", 512, 320), (2048, 144, 1200, "64QAM", 512, 320)]
BRANCHES = (2, 4)
NOISE_VAR = 1e-3


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


def run(N, cp, Kd, mod, n_frames, n_sym, reps):
    bps = om._lib.MODULATION_BITS[mod]
    fl = n_sym * (N + cp)
    b_max = max(BRANCHES)
    units = b_max * n_frames
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    rx = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    nds = rx.data_symbols_per_frame(fl)
    seg = nds * Kd
    nb = txe.bits_per_frame(n_sym)
    d_bits = torch.empty(n_frames * nb, dtype=torch.uint8, device="cuda")
    d_tx = torch.empty(n_frames * fl * 2, dtype=torch.float32, device="cuda")
    d_iq = torch.empty(units * fl * 2, dtype=torch.float32, device="cuda")
    taps = torch.from_numpy((TAPS / np.linalg.norm(TAPS)).astype(np.complex64).view(np.float32)).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = s.cuda_stream
    txe.random_bits(7, 0, d_bits, n_frames * nb, stream=ss)
    txe.modulate_frames(d_bits, n_frames, n_sym, d_tx, stream=ss)
    for b in range(b_max):                                   # the same transmission, a noise stream per branch
        txe.channel(d_tx, n_frames, fl, fl, taps, len(TAPS), d_iq.data_ptr() + b * n_frames * fl * 8, fl, fl, noise_var=NOISE_VAR,
                    seed=3 + b, stream=ss)
    s.synchronize()
    del d_tx
    d_eq = torch.empty(units * seg * 2, dtype=torch.float32, device="cuda")
    d_llr = torch.empty(n_frames * seg * bps, dtype=torch.float32, device="cuda")
    d_a = torch.empty(units * Kd, dtype=torch.float32, device="cuda")
    rx.reserve(units)
    rx.reserve_mrc(b_max, n_frames, nds, Kd)
    rx.demod_frames(d_iq, units, fl, fl, d_eq, stream=ss)
    rx.csi_frames(units, d_a, stream=ss)
    s.synchronize()
    del d_iq
    t = {"csi": timed(lambda: rx.demap_csi_frames(d_eq, n_frames, nds, Kd, seg, d_a, Kd, rx.csi_rho, mod, d_llr,
                                                  noise_mode=om.CSI_NOISE_GIVEN, noise_var=NOISE_VAR, stream=ss), s, reps)}
    for B in BRANCHES:
        t[B] = timed(lambda: rx.combine_csi_frames(d_eq, B, n_frames, nds, Kd, seg, d_a, Kd, rx.csi_rho, mod, [NOISE_VAR] * B,
                                                   d_llr=d_llr, stream=ss), s, reps)
    s.synchronize()
    n = n_frames * seg
    spread = max(max(v[2] / v[0] - 1, 1 - v[1] / v[0]) for v in t.values())
    frac = {k: n * (8 * (1 if k == "csi" else k) + 4 * bps) / v[0] / HBM for k, v in t.items()}
    return ("%4d-pt %-5s %4d output frames x %3d data sym | demap_csi_frames given, one branch %7.3f ms (%.2f of 8 TB/s) | "
            "combine_csi_frames given, llr only: %s | spread of the timed calls +-%.1f %%" % (
                N, mod, n_frames, nds, t["csi"][0] * 1e3, frac["csi"],
                ", ".join("B = %d %7.3f ms (%.2f, %.2f of the csi fraction)" % (B, t[B][0] * 1e3, frac[B], frac[B] / frac["csi"])
                          for B in BRANCHES), spread * 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrc_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    lines = ["# tools/mrc_rate.py --reps %d on %s; algorithmic bytes per output symbol: 8*B + 4*bps (combiner), 8 + 4*bps (csi stage)"
             % (a.reps, torch.cuda.get_device_name(0))]
    for cfg in CONFIGS:
        lines.append(run(*cfg, a.reps))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
