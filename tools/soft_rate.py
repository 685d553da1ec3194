#!/usr/bin/env python3
"""Rate of the segmented soft de-mapper on the frame-batched receiver (ofdm_rx_demod_frames_soft / ofdm_demap_frames).

  soft stage : median time of demod_frames_soft minus that of demod_frames on the same batch (eq + packed bits both times),
               and, on its own, ofdm_demap_frames over the batch's d_eq; for {soft0 + soft1, llr only}
  bytes      : algorithmic, per symbol 8 B read by each of the two passes + 4*bps B per requested array; fraction of 8 TB/s
  loop       : the per-frame ofdm_demap loop the batch call replaces (one call per frame, both metric arrays)

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Frames come from the device transmitter and
the reference 5-tap channel with noise.  2048-pt 144/1200 with QPSK / 16-QAM / 64-QAM, 512 frames of 320 symbols (240 data
symbols: d_eq = 1.2 GB, well past the 256 MiB Infinity Cache), and 64-pt 16/60 QPSK, 4369 frames of 16 symbols.  `--quick`
runs one short pass of every configuration (the kernel-trace run); --json adds one JSON line per configuration."""
import argparse
import json
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
CONFIGS = [(2048, 144, 1200, "QPSK", 512, 320), (2048, 144, 1200, "16QAM", 512, 320), (2048, 144, 1200, "64QAM", 512, 320),
           (64, 16, 60, "QPSK", 4369, 16)]


def timed(fn, s, reps):
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


def run(N, cp, Kd, mod, n_frames, n_sym, reps):
    bps = om._lib.MODULATION_BITS[mod]
    L = N + cp
    fl = n_sym * L
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    rx = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    nds = rx.data_symbols_per_frame(fl)
    seg = nds * Kd
    nb = txe.bits_per_frame(n_sym)
    d_bits = torch.empty(n_frames * nb, dtype=torch.uint8, device="cuda")
    d_tx = torch.empty(n_frames * fl * 2, dtype=torch.float32, device="cuda")
    d_iq = torch.empty(n_frames * fl * 2, dtype=torch.float32, device="cuda")
    taps = torch.from_numpy((TAPS / np.linalg.norm(TAPS)).astype(np.complex64).view(np.float32)).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    txe.random_bits(7, 0, d_bits, n_frames * nb, stream=s.cuda_stream)
    txe.modulate_frames(d_bits, n_frames, n_sym, d_tx, stream=s.cuda_stream)
    txe.channel(d_tx, n_frames, fl, fl, taps, len(TAPS), d_iq, fl, fl, noise_var=1e-3, seed=3, stream=s.cuda_stream)
    s.synchronize()
    del d_tx
    d_eq = torch.empty(n_frames * seg * 2, dtype=torch.float32, device="cuda")
    d_pb = torch.empty(n_frames * seg * bps // 8, dtype=torch.uint8, device="cuda")
    arr = [torch.empty(n_frames * seg * bps, dtype=torch.float32, device="cuda") for _ in range(2)]
    sig = torch.empty(n_frames, dtype=torch.float64, device="cuda")
    rx.reserve(n_frames)
    rx.reserve_soft(n_frames, seg)
    ss = s.cuda_stream
    sets = {"both": dict(d_soft0=arr[0], d_soft1=arr[1], d_sigma=sig), "llr": dict(d_llr=arr[0], d_sigma=sig)}
    t_plain = timed(lambda: rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_pb, om.BITS_PACKED, None, stream=ss), s, reps)
    rec = dict(nfft=N, cp=cp, Kd=Kd, mod=mod, frames=n_frames, data_symbols_per_frame=nds, symbols=n_frames * seg,
               eq_bytes=n_frames * seg * 8, demod_frames_ms=t_plain * 1e3)
    for name, kw in sets.items():
        t_soft = timed(lambda: rx.demod_frames_soft(d_iq, n_frames, fl, fl, d_eq, d_bits=d_pb, bits_mode=om.BITS_PACKED,
                                                    stream=ss, **kw), s, reps)
        t_stage = timed(lambda: rx.demap_frames(d_eq, n_frames, seg, seg, mod, stream=ss, **kw), s, reps)
        n_arr = 2 if name == "both" else 1
        alg = n_frames * seg * (16 + 4 * bps * n_arr)
        rec[name] = dict(demod_frames_soft_ms=t_soft * 1e3, soft_stage_ms=(t_soft - t_plain) * 1e3,
                         demap_frames_ms=t_stage * 1e3, alg_bytes=alg,
                         frac_8tbs_stage=alg / max(t_soft - t_plain, 1e-12) / HBM, frac_8tbs_demap_frames=alg / t_stage / HBM)

    def loop():
        for f in range(n_frames):
            rx.demap(d_eq.data_ptr() + f * seg * 8, seg, mod, None, arr[0].data_ptr() + f * seg * bps * 4,
                     arr[1].data_ptr() + f * seg * bps * 4, stream=ss)
    t_loop = timed(loop, s, max(3, reps // 5))
    rec["ofdm_demap_loop_ms"] = t_loop * 1e3
    rec["batch_speedup_vs_loop"] = t_loop / (rec["both"]["demap_frames_ms"] / 1e3)
    s.synchronize()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    for N, cp, Kd, mod, n_frames, n_sym in CONFIGS:
        rec = run(N, cp, Kd, mod, n_frames, n_sym, 3 if a.quick else a.reps)
        b, o = rec["both"], rec["llr"]
        print("%4d-pt %-5s %4d frames x %3d sym (eq %6.0f MB) | demod %7.3f ms | both: +%7.3f ms (%.2f of 8 TB/s), demap_frames "
              "%7.3f ms (%.2f) | llr: +%7.3f ms (%.2f), demap_frames %7.3f ms (%.2f) | ofdm_demap loop %8.3f ms = x%.0f" % (
                  N, mod, rec["frames"], rec["data_symbols_per_frame"], rec["eq_bytes"] / 1e6, rec["demod_frames_ms"],
                  b["soft_stage_ms"], b["frac_8tbs_stage"], b["demap_frames_ms"], b["frac_8tbs_demap_frames"],
                  o["soft_stage_ms"], o["frac_8tbs_stage"], o["demap_frames_ms"], o["frac_8tbs_demap_frames"],
                  rec["ofdm_demap_loop_ms"], rec["batch_speedup_vs_loop"]), flush=True)
        if a.json:
            print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
