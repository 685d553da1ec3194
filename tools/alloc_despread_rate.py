#!/usr/bin/env python3
"""Rate of ofdm_dft_despread_alloc_frames (every allocation of a row despread in one pass) next to what a user had to do before:
per allocation a dense column gather followed by ofdm_dft_despread_frames.  Timed in the same session on the same buffers.

  fused          : ofdm_dft_despread_alloc_frames, channel state given, llr only
  gather + calls : per allocation torch gathers of the symbol columns and the csi columns into dense buffers, then
                   ofdm_dft_despread_frames -- all allocations inside one pair of events (the yardstick)
  calls alone    : the same calls on buffers gathered beforehand, all inside one pair of events: the sum of the per-allocation
                   calls WITHOUT their gathers.  The expectation to confirm or refute: fused is no slower than this.
  single         : the set {(0, 1200)} next to ofdm_dft_despread_frames on the same buffer

Device events around each variant on one stream, 3 warm-up calls, median of --reps (15) with the min..max of the timed calls over
the median (run-to-run spread).  240 rows per segment, row_len 1200, 16-QAM.  Writes --out (profiles/alloc_despread_rate.txt) and
prints the same lines."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

import torch  # noqa: E402

import ofdm_mi355x as om  # noqa: E402

HBM = 8.0e12
ROW_LEN, ROWS, N_SEG, MOD, BPS = 1200, 240, 128, "16QAM", 4
SETS = {"4 users": [(0, 300), (300, 600), (900, 288), (1188, 12)], "single": [(0, 1200)]}


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


def run(name, allocs, reps, d_sym, d_csi, d_llr):
    rx = om.RxEngine(8, 2048, 144, 2046, (1, 3), ROW_LEN, 30, 0.7, modulation=MOD)
    rx.set_allocations([(s, M, BPS) for s, M in allocs])
    rx.reserve_despread_alloc(N_SEG)
    for _, M in allocs:
        rx.reserve_despread(M, N_SEG)
    lay = om.alloc_layout([M for _, M in allocs], [BPS] * len(allocs), N_SEG, ROWS)
    rho = rx.csi_rho
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    seg = ROWS * ROW_LEN
    sym3 = d_sym.view(N_SEG, ROWS, ROW_LEN, 2)
    dense = [torch.empty(N_SEG * ROWS * M * 2, dtype=torch.float32, device="cuda") for _, M in allocs]
    dcsi = [torch.empty(N_SEG * M, dtype=torch.float32, device="cuda") for _, M in allocs]
    llr = [d_llr[int(o):int(o) + N_SEG * ROWS * M * BPS] for o, (_, M) in zip(lay["llr_off"], allocs)]
    torch.cuda.synchronize()

    def gather():
        for (st, M), g, c in zip(allocs, dense, dcsi):
            g.view(N_SEG, ROWS, M, 2).copy_(sym3[:, :, st:st + M, :])
            c.view(N_SEG, M).copy_(d_csi.view(N_SEG, ROW_LEN)[:, st:st + M])

    def calls():
        for (st, M), g, c, o in zip(allocs, dense, dcsi, llr):
            rx.dft_despread_frames(g, N_SEG, ROWS, M, ROWS * M, c, M, rho, MOD, d_llr=o, stream=ss)

    def both():
        gather()
        calls()

    def fused():
        rx.dft_despread_alloc_frames(d_sym, N_SEG, ROWS, ROW_LEN, seg, d_csi, ROW_LEN, rho, d_llr=d_llr, stream=ss)

    t = {}
    for rnd in range(2):                                     # the variants alternate; the second round is reported
        t["fused"] = timed(fused, s, reps)
        t["both"] = timed(both, s, reps)
        t["calls"] = timed(calls, s, reps)
        if name == "single":
            t["existing"] = timed(lambda: rx.dft_despread_frames(d_sym, N_SEG, ROWS, ROW_LEN, seg, d_csi, ROW_LEN, rho, MOD, d_llr=d_llr,
                                                                 stream=ss), s, reps)
    s.synchronize()
    n = N_SEG * ROWS * sum(M for _, M in allocs)
    by = n * (8 + 4 * BPS)
    spread = max(max(t[k][2] / t[k][0] - 1, 1 - t[k][1] / t[k][0]) for k in t)
    line = ("%-7s %d allocation(s), %d seg x %d rows x %d (%4.0f MB of symbols) | fused %7.3f ms (%.2f of 8 TB/s) | gather + calls %7.3f ms "
            "| calls alone %7.3f ms | fused / calls alone %.2f | fused / (gather + calls) %.2f"
            % (name, len(allocs), N_SEG, ROWS, ROW_LEN, N_SEG * seg * 8 / 1e6, t["fused"][0] * 1e3, by / t["fused"][0] / HBM,
               t["both"][0] * 1e3, t["calls"][0] * 1e3, t["fused"][0] / t["calls"][0], t["fused"][0] / t["both"][0]))
    if "existing" in t:
        line += " | existing call on the same buffer %7.3f ms, fused / existing %.2f" % (t["existing"][0] * 1e3, t["fused"][0] / t["existing"][0])
    return line + " | spread of the timed calls +-%.1f %%" % (spread * 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alloc_despread_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    n = N_SEG * ROWS * ROW_LEN
    g = torch.Generator(device="cuda").manual_seed(7)
    d_sym = torch.randn(n * 2, dtype=torch.float32, device="cuda", generator=g) * 0.7
    d_csi = torch.rand(N_SEG * ROW_LEN, dtype=torch.float32, device="cuda", generator=g) * 2 + 0.02
    d_llr = torch.empty(n * BPS, dtype=torch.float32, device="cuda")
    lines = ["# tools/alloc_despread_rate.py --reps %d on %s; algorithmic bytes per allocated symbol: 8 B read + 4*bps B (llr) written; "
             "16-QAM, llr only, channel state given" % (a.reps, torch.cuda.get_device_name(0))]
    for name, allocs in SETS.items():
        lines.append(run(name, allocs, a.reps, d_sym, d_csi, d_llr))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
