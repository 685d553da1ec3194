#!/usr/bin/env python3
"""Rate of the turbo decoder (ofdm_turbo_decode_frames) behind the soft batch receiver, and of the encoder in front of the
transmitter, on the batch of tools/tbcc_rate.py.

  batch    : 2048-pt 144/1200 16-QAM, 512 frames of 240 symbols (180 data symbols: 864000 LLRs per frame); device transmitter
             with encoded random information bits, reference 5-tap channel with noise
  per K    : K in {40, 1024, 6144} with floor(864000 / (3K + 12)) blocks per frame, n_iter in {1, 6}: median time of the decode
             call (packed bits), decoded information Mbit/s, trellis steps/s counted as K * 2 * n_iter per block (what the
             algorithm needs; the kernel runs each step three times: forward, forward again from the checkpoint, backward),
             block errors against the sent bits, the encode call's time
  same run : the demod_frames_soft call that produced the LLRs, and ofdm_tbcc_decode_frames at K = 1024 on the same LLR buffer
  ceiling  : vector and LDS instructions of the three step loops, read from the code object with tools/dev/isa_blocks.py (each
             unrolled block holds 8 steps).  Model as in tools/tbcc_rate.py: a SIMD issues one vector / LDS wave-instruction per
             4 cycles and a wave carries 8 blocks, so counted steps/s <= 8 * 256 CUs * 4 SIMDs * 2.4 GHz / (4 * instructions
             per counted step), instructions per counted step = forward-only + forward-kept + backward.

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/turbo_rate.txt."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

TAPS = [0.3977, 0.7954 - 0.3977j, -0.1988, 0.0994, -0.0398]                       # the reference channel (TX:64)
N, CP, KD, MOD, FRAMES, N_SYM = 2048, 144, 1200, "16QAM", 512, 240
CASES = ((40, 3, 10), (1024, 31, 64), (6144, 263, 480))                           # K, f1, f2
ITERS = (1, 6)
TBCC_K = 1024
CUS, SIMDS, CLOCK, GROUP, UNROLL = 256, 4, 2.4e9, 8, 8


def step_loops():
    """-> [(vector, LDS) instructions per step] of the three unrolled step loops (the blocks with the most ds instructions), or
    None without a compiler"""
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dev", "isa_blocks.py"), "turbo.hip",
                              r"_ZN4ofdm\w*turbo_decode_kernel"], check=True, capture_output=True, text=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return None
    blocks = []
    for line in out.splitlines():
        m = re.match(r"^(\.LBB\S+)(?: LOOP)?\s+(\d+)\s+(\{.*?\})", line)
        if m:
            mix = json.loads(m.group(3).replace("'", '"'))
            blocks.append((mix.get("ds", 0), mix.get("v", 0)))
    blocks.sort(reverse=True)
    return [(v / UNROLL, ds / UNROLL) for ds, v in blocks[:3]] if len(blocks) >= 3 else None


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
    flr = fl + CP
    txe = om.TxEngine(N, CP, N - 2, KD, (1, 3), MOD)
    rx = om.RxEngine(N_SYM, N, CP, N - 2, (1, 3), KD, 100, 0.7, modulation=MOD)
    seg_bits = txe.bits_per_frame(N_SYM)
    nds = rx.data_symbols_per_frame(flr)
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    taps = np.zeros(CP + 1, np.complex64)
    taps[:len(TAPS)] = np.asarray(TAPS) / np.linalg.norm(TAPS)
    d_taps = torch.from_numpy(taps.view(np.float32)).cuda()
    d_coded = torch.empty(frames * seg_bits, dtype=torch.uint8, device="cuda")
    d_tx = torch.empty(frames * fl * 2, dtype=torch.float32, device="cuda")
    d_iq = torch.empty(frames * flr * 2, dtype=torch.float32, device="cuda")
    d_eq = torch.empty(frames * nds * KD * 2, dtype=torch.float32, device="cuda")
    d_llr = torch.empty(frames * seg_bits, dtype=torch.float32, device="cuda")
    rx.reserve(frames)
    rx.reserve_soft(frames, nds * KD)
    emit("# %d-pt %s, %d frames x %d symbols (%d data symbols, %d LLRs per frame), noise_var 0.02" % (N, MOD, frames, N_SYM, nds, seg_bits))
    loops = step_loops()
    if loops:
        per_step = sum(v + ds for v, ds in loops)
        ceiling = GROUP * CUS * SIMDS * CLOCK / (4.0 * per_step)
        emit("# step loops (code object, per trellis step and wave): %s vector + LDS; %.1f per counted step; issue-bound ceiling "
             "%.3g counted steps/s" % (", ".join("%.2f + %.2f" % l for l in loops), per_step, ceiling))
    else:
        ceiling = None
        emit("# step loops: no compiler here, instruction count not taken")
    for K, f1, f2 in CASES:
        nblk = om.turbo_blocks(seg_bits, K)
        n_blocks = frames * nblk
        d_rand = torch.empty(n_blocks * K, dtype=torch.uint8, device="cuda")
        d_dec = torch.empty(n_blocks * K // 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        txe.random_bits(7 + K, 0, d_rand, n_blocks * K, stream=ss)
        s.synchronize()
        with torch.cuda.stream(s):
            w = (2 ** torch.arange(7, -1, -1, device="cuda", dtype=torch.int32))
            d_info = (d_rand.view(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)
        s.synchronize()
        del d_rand
        enc = lambda: txe.turbo_encode_frames(d_info, frames, nblk, K, f1, f2, d_coded, seg_bits, info_mode=om.BITS_PACKED, stream=ss)  # noqa: E731
        t_enc = timed(torch, enc, s, reps)
        txe.modulate_frames(d_coded, frames, N_SYM, d_tx, stream=ss)
        txe.channel(d_tx, frames, fl, fl, d_taps, len(taps), d_iq, flr, flr, noise_var=0.02, seed=3, stream=ss)
        soft = lambda: rx.demod_frames_soft(d_iq, frames, flr, flr, d_eq, d_llr=d_llr, stream=ss)  # noqa: E731
        t_soft = timed(torch, soft, s, reps)
        rx.reserve_turbo(n_blocks, K)
        for n_iter in ITERS:
            dec = lambda: rx.turbo_decode_frames(d_llr, frames, seg_bits, nblk, K, f1, f2, n_iter, d_bits=d_dec,  # noqa: E731
                                                 bits_mode=om.BITS_PACKED, stream=ss)
            t_dec = timed(torch, dec, s, reps)
            s.synchronize()
            wrong = int((d_dec.view(n_blocks, K // 8) != d_info.view(n_blocks, K // 8)).any(1).sum())
            steps = n_blocks * K * 2 * n_iter
            emit("K=%4d n_iter=%d  %7d blocks | decode %9.3f ms = %8.1f Mbit/s decoded, %.3g steps/s%s | demod_frames_soft %8.3f ms | "
                 "encode %7.3f ms | block errors %d" % (
                     K, n_iter, n_blocks, t_dec * 1e3, n_blocks * K / t_dec / 1e6, steps / t_dec,
                     (" (%.2f of the issue-bound ceiling)" % (steps / t_dec / ceiling)) if ceiling else "", t_soft * 1e3, t_enc * 1e3, wrong))
        if K == TBCC_K:
            nb_t = frames * om.tbcc_blocks(seg_bits, TBCC_K)
            d_tb = torch.empty(nb_t * TBCC_K // 8, dtype=torch.uint8, device="cuda")
            rx.reserve_tbcc(nb_t, TBCC_K)
            tb = lambda: rx.tbcc_decode_frames(d_llr, frames, seg_bits, nb_t // frames, TBCC_K, d_bits=d_tb, bits_mode=om.BITS_PACKED, stream=ss)  # noqa: E731
            emit("K=%4d TBCC    %7d blocks | ofdm_tbcc_decode_frames on the same LLR buffer %9.3f ms" % (TBCC_K, nb_t, timed(torch, tb, s, reps) * 1e3))
            del d_tb
        del d_info, d_dec
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--quick", action="store_true", help="one short pass (32 frames, 3 repetitions), nothing written")
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.quick:
        measure(32, 3, lambda t: print(t, flush=True))
        return
    os.makedirs(a.outdir, exist_ok=True)
    lines = ["# Generated by: python3 tools/turbo_rate.py" + ("" if a.frames == FRAMES else " --frames %d" % a.frames)]

    def emit(t):
        print(t, flush=True)
        lines.append(t)
    measure(a.frames, a.reps, emit)
    with open(os.path.join(a.outdir, "turbo_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
