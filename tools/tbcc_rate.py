#!/usr/bin/env python3
"""Rate of the TBCC decoder (ofdm_tbcc_decode_frames) behind the soft batch receiver, and of the encoder in front of the
transmitter.

  batch    : 2048-pt 144/1200 16-QAM, 512 frames of 240 symbols (180 data symbols: 864000 LLRs per frame, 1.77 GB per batch);
             device transmitter with encoded random information bits, reference 5-tap channel with noise
  per K    : K in {40, 256, 1024}, floor(864000 / 3K) blocks per frame; median time of the decode call (packed bits + metric +
             tb_ok), decoded information Mbit/s, trellis steps/s (K + 192 steps per block), block errors against the sent bits,
             and the time of the demod_frames_soft call that produced the LLRs in the same session
  ceiling  : instructions per trellis step of the decoder's inner loop, read from the code object with tools/dev/isa_blocks.py
             (the basic block with the ds_bpermute pairs holds 8 steps).  Model: a SIMD issues one vector / LDS wave-instruction
             per 4 cycles, so steps/s <= 256 CUs * 4 SIMDs * 2.4 GHz / (4 * vector-and-LDS instructions per step); the fraction
             reached is measured steps/s over that.

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/tbcc_rate.txt and, unless
--no-trace, runs itself once more with --quick under `rocprofv3 --kernel-trace --stats` (a fresh child process) and keeps the
kernel statistics as <outdir>/tbcc_kernel_stats.csv."""
import argparse
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

TAPS = [0.3977, 0.7954 - 0.3977j, -0.1988, 0.0994, -0.0398]                       # the reference channel (TX:64)
N, CP, KD, MOD, FRAMES, N_SYM = 2048, 144, 1200, "16QAM", 512, 240
KS = (40, 256, 1024)
CUS, SIMDS, CLOCK = 256, 4, 2.4e9
STEPS_PER_BLOCK_OF_CODE = 8                                                        # the unroll of tbcc_viterbi_kernel's step loop


def inner_loop_mix():
    """-> dict(v=, ds=, s=, w=, total=) per trellis step from the code object, or None without a compiler"""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dev", "isa_blocks.py"), "tbcc.hip",
                              r"_ZN4ofdm\w*tbcc_viterbi_kernelILb0"], check=True, capture_output=True, text=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return None
    best = None
    for line in out.splitlines():
        m = re.match(r"^(\.LBB\S+)(?: LOOP)?\s+(\d+)\s+(\{.*?\})", line)
        if not m:
            continue
        mix = json.loads(m.group(3).replace("'", '"'))
        if best is None or mix.get("ds", 0) > best[1].get("ds", 0):
            best = (int(m.group(2)), mix)
    if best is None:
        return None
    n, mix = best
    d = {k: mix.get(k, 0) / STEPS_PER_BLOCK_OF_CODE for k in ("v", "ds", "s", "w", "br")}
    d["total"] = n / STEPS_PER_BLOCK_OF_CODE
    return d


def timed(torch, fn, s, reps):
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
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) / 1e3


def measure(frames, reps, emit):
    import numpy as np
    import torch
    import ofdm_mi355x as om
    torch.cuda.init()
    om.load()
    L = N + CP
    fl = N_SYM * L
    txe = om.TxEngine(N, CP, N - 2, KD, (1, 3), MOD)
    rx = om.RxEngine(N_SYM, N, CP, N - 2, (1, 3), KD, 100, 0.7, modulation=MOD)
    seg_bits = txe.bits_per_frame(N_SYM)
    nds = rx.data_symbols_per_frame(fl + CP)
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    flr = fl + CP                                  # received frames are cp samples longer: every pattern passes the guard
    taps = np.zeros(CP + 1, np.complex64)          # zero-padded taps let the channel deliver that tail
    taps[:len(TAPS)] = np.asarray(TAPS) / np.linalg.norm(TAPS)
    d_taps = torch.from_numpy(taps.view(np.float32)).cuda()
    d_coded = torch.empty(frames * seg_bits, dtype=torch.uint8, device="cuda")
    d_tx = torch.empty(frames * fl * 2, dtype=torch.float32, device="cuda")
    d_iq = torch.empty(frames * flr * 2, dtype=torch.float32, device="cuda")
    d_eq = torch.empty(frames * nds * KD * 2, dtype=torch.float32, device="cuda")
    d_llr = torch.empty(frames * seg_bits, dtype=torch.float32, device="cuda")
    rx.reserve(frames)
    rx.reserve_soft(frames, nds * KD)
    mix = inner_loop_mix()
    emit("# %d-pt %s, %d frames x %d symbols (%d data symbols, %d LLRs per frame, %.2f GB of LLRs), noise_var 0.02" % (
        N, MOD, frames, N_SYM, nds, seg_bits, frames * seg_bits * 4 / 1e9))
    if mix:
        ceiling = CUS * SIMDS * CLOCK / (4.0 * (mix["v"] + mix["ds"]))
        emit("# inner loop per trellis step (code object): %.2f instructions = %.2f vector + %.2f LDS + %.2f scalar + %.2f waitcnt; "
             "issue-bound ceiling %.3g steps/s" % (mix["total"], mix["v"], mix["ds"], mix["s"], mix["w"], ceiling))
    else:
        ceiling = None
        emit("# inner loop: no compiler here, instruction count not taken")
    for K in KS:
        nblk = om.tbcc_blocks(seg_bits, K)
        n_blocks = frames * nblk
        d_info = torch.empty(n_blocks * K // 8, dtype=torch.uint8, device="cuda")
        d_rand = torch.empty(n_blocks * K, dtype=torch.uint8, device="cuda")
        d_dec = torch.empty(n_blocks * K // 8, dtype=torch.uint8, device="cuda")
        d_m = torch.empty(n_blocks, dtype=torch.float32, device="cuda")
        d_ok = torch.empty(n_blocks, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        txe.random_bits(7 + K, 0, d_rand, n_blocks * K, stream=ss)
        s.synchronize()
        with torch.cuda.stream(s):
            w = (2 ** torch.arange(7, -1, -1, device="cuda", dtype=torch.int32))
            d_info.copy_((d_rand.view(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8))
        s.synchronize()
        enc = lambda: txe.tbcc_encode_frames(d_info, frames, nblk, K, d_coded, seg_bits, info_mode=om.BITS_PACKED, stream=ss)  # noqa: E731
        t_enc = timed(torch, enc, s, reps)
        txe.modulate_frames(d_coded, frames, N_SYM, d_tx, stream=ss)
        txe.channel(d_tx, frames, fl, fl, d_taps, len(taps), d_iq, flr, flr, noise_var=0.02, seed=3, stream=ss)
        soft = lambda: rx.demod_frames_soft(d_iq, frames, flr, flr, d_eq, d_llr=d_llr, stream=ss)  # noqa: E731
        t_soft = timed(torch, soft, s, reps)
        rx.reserve_tbcc(n_blocks, K)
        dec = lambda: rx.tbcc_decode_frames(d_llr, frames, seg_bits, nblk, K, d_bits=d_dec, bits_mode=om.BITS_PACKED,  # noqa: E731
                                            d_metric=d_m, d_tb_ok=d_ok, stream=ss)
        t_dec = timed(torch, dec, s, reps)
        s.synchronize()
        wrong = int((d_dec.view(n_blocks, K // 8) != d_info.view(n_blocks, K // 8)).any(1).sum())
        steps = n_blocks * (K + 192)
        line = ("K=%4d  %7d blocks | decode %8.3f ms = %8.1f Mbit/s decoded, %.3g steps/s%s | demod_frames_soft %8.3f ms | encode %7.3f ms"
                " | block errors %d, tb_ok %d" % (
                    K, n_blocks, t_dec * 1e3, n_blocks * K / t_dec / 1e6, steps / t_dec,
                    (" (%.2f of the issue-bound ceiling)" % (steps / t_dec / ceiling)) if ceiling else "", t_soft * 1e3, t_enc * 1e3,
                    wrong, int(d_ok.sum())))
        emit(line)
        del d_info, d_rand, d_dec, d_m, d_ok
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="one short pass (32 frames, 3 repetitions), nothing written")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.quick:
        measure(32, 3, lambda t: print(t, flush=True))
        return
    os.makedirs(a.outdir, exist_ok=True)
    lines = ["# Generated by: python3 tools/tbcc_rate.py"]

    def emit(t):
        print(t, flush=True)
        lines.append(t)
    measure(FRAMES, a.reps, emit)
    with open(os.path.join(a.outdir, "tbcc_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if a.no_trace or not shutil.which("rocprofv3"):
        return
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "tbcc", "--",
                        sys.executable, os.path.abspath(__file__), "--quick"], check=True, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if found:
            shutil.copy(found[0], os.path.join(a.outdir, "tbcc_kernel_stats.csv"))
            print("kernel statistics ->", os.path.join(a.outdir, "tbcc_kernel_stats.csv"))


if __name__ == "__main__":
    main()
