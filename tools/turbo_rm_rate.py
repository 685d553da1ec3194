#!/usr/bin/env python3
"""Rate of the turbo rate-matching calls: ofdm_tx_turbo_encode_rm_frames and ofdm_turbo_rate_dematch_frames.

  batch    : that of tools/turbo_rate.py -- 2048-pt 144/1200 16-QAM, 512 frames of 240 symbols (864000 LLRs per frame); device
             transmitter with rate-matched random information bits, reference 5-tap channel with noise, demod_frames_soft
  per case : K in {40, 1024, 6144} x E in {ceil(1.5 K), 3K + 12, 6K}, floor(864000 / E) blocks per frame, rv 0, Ncb = Kw:
             - the encoder against the plain turbo encoder on the same K (the same block count where 3K + 12 bits per block fit)
             - the de-matching kernel without and with accumulate against a plain device copy of the same bytes (the E floats
               it reads plus the 3K + 12 it writes per block)
             - the de-matching kernel against ofdm_turbo_decode_frames of the same blocks at n_iter 6

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/turbo_rm_rate.txt."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

TAPS = [0.3977, 0.7954 - 0.3977j, -0.1988, 0.0994, -0.0398]                       # the reference channel (TX:64)
N, CP, KD, MOD, FRAMES, N_SYM = 2048, 144, 1200, "16QAM", 512, 240
CASES = ((40, 3, 10), (1024, 31, 64), (6144, 263, 480))                           # K, f1, f2
N_ITER = 6


def es(K):
    return ((3 * K + 1) // 2, 3 * K + 12, 6 * K)


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
    txe.reserve_turbo_rm()
    rx.reserve_turbo_rm()
    emit("# %d-pt %s, %d frames x %d symbols (%d LLRs per frame), noise_var 0.02, rv 0, Ncb = Kw; times in ms, median of %d" % (
        N, MOD, frames, N_SYM, seg_bits, reps))
    for K, f1, f2 in CASES:
        per = 3 * K + 12
        for E in es(K):
            nblk = om.turbo_rm_blocks(seg_bits, K, E)
            nb = frames * nblk
            d_rand = torch.empty(nb * K, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            txe.random_bits(7 + K + E, 0, d_rand, nb * K, stream=ss)
            s.synchronize()
            with torch.cuda.stream(s):
                w = (2 ** torch.arange(7, -1, -1, device="cuda", dtype=torch.int32))
                d_info = (d_rand.view(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)
            s.synchronize()
            del d_rand
            d_soft = torch.zeros(nb * per, dtype=torch.float32, device="cuda")
            d_dec = torch.empty(nb * K // 8, dtype=torch.uint8, device="cuda")
            n_copy = nb * (E + per)
            d_src = torch.empty(n_copy // 2, dtype=torch.float32, device="cuda")
            d_dst = torch.empty(n_copy // 2, dtype=torch.float32, device="cuda")
            nblk_p = min(nblk, seg_bits // per)              # the plain encoder needs 3K + 12 bits per block: fewer fit for E < 3K + 12
            t_plain = timed(torch, lambda: txe.turbo_encode_frames(d_info, frames, nblk_p, K, f1, f2, d_coded, seg_bits,
                                                                   info_mode=om.BITS_PACKED, stream=ss), s, reps)
            t_enc = timed(torch, lambda: txe.turbo_encode_rm_frames(d_info, frames, nblk, K, f1, f2, E, d_coded, seg_bits,
                                                                    info_mode=om.BITS_PACKED, stream=ss), s, reps)
            txe.modulate_frames(d_coded, frames, N_SYM, d_tx, stream=ss)
            txe.channel(d_tx, frames, fl, fl, d_taps, len(taps), d_iq, flr, flr, noise_var=0.02, seed=3, stream=ss)
            rx.demod_frames_soft(d_iq, frames, flr, flr, d_eq, d_llr=d_llr, stream=ss)
            rx.reserve_turbo(nb, K)
            dem = lambda acc: rx.turbo_rate_dematch_frames(d_llr, frames, seg_bits, nblk, K, E, d_soft, nblk * per,  # noqa: E731
                                                           accumulate=acc, stream=ss)
            t_acc = timed(torch, lambda: dem(True), s, reps)
            t_dem = timed(torch, lambda: dem(False), s, reps)               # last: d_soft holds the first transmission alone
            t_copy = timed(torch, lambda: d_dst.copy_(d_src), s, reps)
            t_dec = timed(torch, lambda: rx.turbo_decode_frames(d_soft, frames, nblk * per, nblk, K, f1, f2, N_ITER, d_bits=d_dec,
                                                                bits_mode=om.BITS_PACKED, stream=ss), s, reps)
            s.synchronize()
            wrong = int((d_dec.view(nb, K // 8) != d_info.view(nb, K // 8)).any(1).sum())
            emit("K=%4d E=%5d %7d blocks | encode_rm %7.3f (plain encoder, %d blocks: %7.3f) | de-match %7.3f, accumulate %7.3f, copy of the same "
                 "%.1f MB %7.3f | decode n_iter %d %9.3f = %.1f x de-match | block errors %d" % (
                     K, E, nb, t_enc * 1e3, frames * nblk_p, t_plain * 1e3, t_dem * 1e3, t_acc * 1e3,
                     n_copy * 4 / 1e6, t_copy * 1e3, N_ITER, t_dec * 1e3, t_dec / t_dem, wrong))
            del d_info, d_soft, d_dec, d_src, d_dst
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
    lines = ["# Generated by: python3 tools/turbo_rm_rate.py" + ("" if a.frames == FRAMES else " --frames %d" % a.frames)]

    def emit(t):
        print(t, flush=True)
        lines.append(t)
    measure(a.frames, a.reps, emit)
    with open(os.path.join(a.outdir, "turbo_rm_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
