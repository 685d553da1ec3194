#!/usr/bin/env python3
"""Rate of the turbo decoder with early termination (ofdm_turbo_decode_es_frames) against the fixed decoder
(ofdm_turbo_decode_frames at n_iter = max_iter) on the same LLRs in the same session.

  blocks   : CRC24B-terminated code blocks (random payload, parity from ofdm_crc_compute_long), device encoder, BPSK over AWGN
             made on the device (LLR = 2 y / sigma^2), one block per segment
  shapes   : K = 6144 (16384 blocks = 2048 waves) and K = 1024 (98304 blocks), max_iter 6, min_iter 1
  per Es/N0: the histogram of iters, the blocks whose CRC never passed, the mean over the waves (8 consecutive blocks) of the
             wave's largest iters -- what the kernel can reach, a wave runs as long as its slowest block --, the time of the ES call,
             the time of the fixed decoder, their ratio and the ratio the wave maxima predict (mean wave max / max_iter)
  overhead : one more row per K with min_iter = max_iter, where nothing can stop: its difference to the fixed decoder is the
             price of the post stores and the CRC passes

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/turbo_es_rate.txt."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

CASES = ((6144, 263, 480, 16384), (1024, 31, 64, 98304))                          # K, f1, f2, blocks
POINTS_DB = (0.0, -3.0, -3.75, -4.25)
MAX_ITER = 6


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
    return statistics.median(ms)


def crc_blocks(np, om, K, n, seed):
    """-> packed [n][K / 8]: random payload, then its CRC24B (zero mask)"""
    info = np.random.default_rng(seed).integers(0, 256, (n, K // 8), dtype=np.uint8)
    for b in range(n):
        crc = om.crc_compute_long(om.CRC24B, info[b], K - 24)
        info[b, -3:] = (crc >> 16) & 0xff, (crc >> 8) & 0xff, crc & 0xff
    return info


def measure(scale, reps, emit):
    import numpy as np
    import torch
    import ofdm_mi355x as om
    torch.cuda.init()
    om.load()
    txe = om.TxEngine(64, 16, 62, 60)
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    for K, f1, f2, n_full in CASES:
        n = max(8, n_full // scale)
        per = 3 * K + 12
        d_info = torch.from_numpy(crc_blocks(np, om, K, n, 100 + K)).cuda()
        d_coded = torch.empty(n * per, dtype=torch.uint8, device="cuda")
        d_llr = torch.empty(n * per, dtype=torch.float32, device="cuda")
        d_bits = torch.empty(n * K // 8, dtype=torch.uint8, device="cuda")
        d_fixed = torch.empty(n * K // 8, dtype=torch.uint8, device="cuda")
        d_iters = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        txe.turbo_encode_frames(d_info, n, 1, K, f1, f2, d_coded, per, info_mode=om.BITS_PACKED, stream=ss)
        s.synchronize()
        rx.reserve_turbo_es(n, K)
        emit("# K = %d, %d blocks (%d waves), CRC24B, max_iter %d" % (K, n, (n + 7) // 8, MAX_ITER))

        def es(lo):
            rx.turbo_decode_es_frames(d_llr, n, per, 1, K, f1, f2, om.CRC24B, lo, MAX_ITER, d_bits=d_bits, bits_mode=om.BITS_PACKED,
                                      d_iters=d_iters, d_crc_ok=d_ok, stream=ss)

        def fixed():
            rx.turbo_decode_frames(d_llr, n, per, 1, K, f1, f2, MAX_ITER, d_bits=d_fixed, bits_mode=om.BITS_PACKED, stream=ss)

        for i, db in enumerate(POINTS_DB):
            sigma2 = 0.5 * 10.0 ** (-db / 10.0)
            with torch.cuda.stream(s):
                gen = torch.Generator(device="cuda").manual_seed(1000 + i)
                y = 1.0 - 2.0 * d_coded.to(torch.float32) + sigma2 ** 0.5 * torch.randn(n * per, generator=gen, device="cuda")
                d_llr.copy_(y * (2.0 / sigma2))
                del y
            s.synchronize()
            t_es = timed(torch, lambda: es(1), s, reps)
            t_fx = timed(torch, fixed, s, reps)
            s.synchronize()
            iters = d_iters.cpu().numpy()
            ok = d_ok.cpu().numpy()
            wrong = int((d_bits.view(n, K // 8) != d_info.view(n, K // 8)).any(1).sum())
            wave_max = float(iters[:n - n % 8].reshape(-1, 8).max(axis=1).mean()) if n >= 8 else float(iters.max())
            emit("K=%4d Es/N0 %+5.2f dB | iters 1..%d %s, never %d, block errors %d | mean wave max %.3f | ES %8.3f ms | fixed n_iter=%d "
                 "%8.3f ms | ES / fixed %.3f, wave max / max_iter %.3f, gap %+.3f" % (
                     K, db, MAX_ITER, np.bincount(iters, minlength=MAX_ITER + 1)[1:].tolist(), int((ok == 0).sum()), wrong, wave_max, t_es,
                     MAX_ITER, t_fx, t_es / t_fx, wave_max / MAX_ITER, t_es / t_fx - wave_max / MAX_ITER))
            if i == len(POINTS_DB) - 1:
                t_all = timed(torch, lambda: es(MAX_ITER), s, reps)
                s.synchronize()
                same = bool(torch.equal(d_bits, d_fixed))
                emit("K=%4d Es/N0 %+5.2f dB | min_iter = max_iter = %d (nothing can stop) | ES %8.3f ms | fixed %8.3f ms | overhead %+.3f ms "
                     "= %+.2f %% of the fixed decode | bits equal the fixed decoder's: %s" % (
                         K, db, MAX_ITER, t_all, t_fx, t_all - t_fx, 100.0 * (t_all - t_fx) / t_fx, same))
        del d_info, d_coded, d_llr, d_bits, d_fixed, d_iters, d_ok
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="one short pass (1/64 of the blocks, 3 repetitions), nothing written")
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.quick:
        measure(64, 3, lambda t: print(t, flush=True))
        return
    os.makedirs(a.outdir, exist_ok=True)
    lines = ["# Generated by: python3 tools/turbo_es_rate.py"]

    def emit(t):
        print(t, flush=True)
        lines.append(t)
    measure(1, a.reps, emit)
    with open(os.path.join(a.outdir, "turbo_es_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
