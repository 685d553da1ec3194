#!/usr/bin/env python3
"""Rate of ofdm_combine_despread_alloc_frames (B branches combined and every allocation of a row despread in one pass) next to
what a user had to do before: per allocation the dense column gathers of every branch's symbols and channel powers, followed by
ofdm_combine_despread_frames.  Timed in the same session on the same buffers.

  fused          : ofdm_combine_despread_alloc_frames, noise given, llr only
  gather + calls : per allocation torch gathers of the symbol columns and the csi columns of all B*n_seg units into dense
                   buffers, then ofdm_combine_despread_frames -- all allocations inside one pair of events (the yardstick)
  calls alone    : the same calls on buffers gathered beforehand, all inside one pair of events: the sum of the per-allocation
                   calls WITHOUT their gathers.  The expectation to confirm or refute: fused is no slower than this.
  single         : the set {(0, 1200)} next to ofdm_combine_despread_frames on the same buffer

Device events around each variant on one stream, 3 warm-up calls, median of --reps (15) with the min..max of the timed calls over
the median (run-to-run spread); the variants alternate and the second round is reported.  128 segments of 240 rows, row_len
1200, B = 2 and 4, 16-QAM.  Writes --out (profiles/mrc_despread_alloc_rate.txt) and prints the same lines."""
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
BRANCHES = (2, 4)
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


def run(name, allocs, B, reps, d_sym, d_csi, d_llr):
    units = B * N_SEG
    rx = om.RxEngine(8, 2048, 144, 2046, (1, 3), ROW_LEN, 30, 0.7, modulation=MOD)
    rx.set_allocations([(s, M, BPS) for s, M in allocs])
    rx.reserve_mrc_despread_alloc(B, N_SEG, ROW_LEN)
    for _, M in allocs:
        rx.reserve_mrc_despread(M, B, N_SEG)
    lay = om.alloc_layout([M for _, M in allocs], [BPS] * len(allocs), N_SEG, ROWS)
    rho, nv = rx.csi_rho, [0.05] * B
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    seg = ROWS * ROW_LEN
    sym3 = d_sym[:units * seg * 2].view(units, ROWS, ROW_LEN, 2)
    csi2 = d_csi[:units * ROW_LEN].view(units, ROW_LEN)
    dense = [torch.empty(units * ROWS * M * 2, dtype=torch.float32, device="cuda") for _, M in allocs]
    dcsi = [torch.empty(units * M, dtype=torch.float32, device="cuda") for _, M in allocs]
    llr = [d_llr[int(o):int(o) + N_SEG * ROWS * M * BPS] for o, (_, M) in zip(lay["llr_off"], allocs)]
    torch.cuda.synchronize()

    def gather():
        for (st, M), g, c in zip(allocs, dense, dcsi):
            g.view(units, ROWS, M, 2).copy_(sym3[:, :, st:st + M, :])
            c.view(units, M).copy_(csi2[:, st:st + M])

    def calls():
        for (st, M), g, c, o in zip(allocs, dense, dcsi, llr):
            rx.combine_despread_frames(g, B, N_SEG, ROWS, M, ROWS * M, c, M, rho, MOD, noise_var=nv, d_llr=o, stream=ss)

    def both():
        gather()
        calls()

    def fused():
        rx.combine_despread_alloc_frames(d_sym, B, N_SEG, ROWS, ROW_LEN, seg, d_csi, ROW_LEN, rho, noise_var=nv, d_llr=d_llr, stream=ss)

    def existing():
        rx.combine_despread_frames(d_sym, B, N_SEG, ROWS, ROW_LEN, seg, d_csi, ROW_LEN, rho, MOD, noise_var=nv, d_llr=d_llr, stream=ss)

    t = {}
    for rnd in range(2):                                     # the variants alternate; the second round is reported
        t["fused"] = timed(fused, s, reps)
        t["both"] = timed(both, s, reps)
        t["calls"] = timed(calls, s, reps)
        if name == "single":
            t["existing"] = timed(existing, s, reps)
    s.synchronize()
    n = N_SEG * ROWS * sum(M for _, M in allocs)
    by = n * (8 * B + 4 * BPS)
    spread = max(max(t[k][2] / t[k][0] - 1, 1 - t[k][1] / t[k][0]) for k in t)
    line = ("%-7s B = %d, %d allocation(s), %d seg x %d rows x %d (%4.0f MB of symbols) | fused %7.3f ms (%.2f of 8 TB/s) | gather + calls "
            "%7.3f ms | calls alone %7.3f ms | fused / calls alone %.2f | fused / (gather + calls) %.2f"
            % (name, B, len(allocs), N_SEG, ROWS, ROW_LEN, units * seg * 8 / 1e6, t["fused"][0] * 1e3, by / t["fused"][0] / HBM,
               t["both"][0] * 1e3, t["calls"][0] * 1e3, t["fused"][0] / t["calls"][0], t["fused"][0] / t["both"][0]))
    if "existing" in t:
        line += " | existing call on the same buffer %7.3f ms, fused / existing %.2f" % (t["existing"][0] * 1e3, t["fused"][0] / t["existing"][0])
    return line + " | spread of the timed calls +-%.1f %%" % (spread * 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrc_despread_alloc_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    n = max(BRANCHES) * N_SEG * ROWS * ROW_LEN
    g = torch.Generator(device="cuda").manual_seed(7)
    d_sym = torch.randn(n * 2, dtype=torch.float32, device="cuda", generator=g) * 0.7
    d_csi = torch.rand(max(BRANCHES) * N_SEG * ROW_LEN, dtype=torch.float32, device="cuda", generator=g) * 2 + 0.02
    d_llr = torch.empty(N_SEG * ROWS * ROW_LEN * BPS, dtype=torch.float32, device="cuda")
    lines = ["# tools/mrc_despread_alloc_rate.py --reps %d on %s; algorithmic bytes per allocated symbol: 8*B B read + 4*bps B (llr) "
             "written; 16-QAM, llr only, noise given" % (a.reps, torch.cuda.get_device_name(0))]
    for B in BRANCHES:
        for name, allocs in SETS.items():
            lines.append(run(name, allocs, B, a.reps, d_sym, d_csi, d_llr))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
