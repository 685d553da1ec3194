#!/usr/bin/env python3
"""Cost of averaging the channel estimate over a frame's sync symbols inside ofdm_rx_demod_frames: the same call on the same
buffers with the stage off and on (n_avg = 4, 16 and -1 = all 60 patterns), alternating in one session.

  total     : device events around demod_frames on one stream
  sync leg  : the handle's own events (ofdm_rx_set_profiling): sync search + LS estimate, and -- stage on -- its two launches
  demod leg : the handle's own events: FFT + equalise + de-map

The stage reads n windows of N samples per frame (n = the patterns averaged) plus one more per chunk of 16 (pattern 0 again, which
the cache holds) and writes one partial row per chunk: its algorithmic bytes are counted as n*N*8 per frame read plus the partial
rows written and read back, the mean row and the gains.  They are put over the added sync-leg time as a fraction of 8 TB/s, next
to the same figure for the demod leg of the same session (its symbols read, its equalised bins written): the same access pattern
on the same chip.  No threshold.

3 warm-up calls per mode, then --rounds (7) rounds of [--reps (8) calls off, --reps calls on] per n_avg; a round's figure is the
mean of its calls, the result the median over the rounds with the min..max spread.  2048-pt 144/1200 QPSK, 512 frames of 240
symbols, frames from the device transmitter and the reference 5-tap channel.  Writes --out (profiles/chanavg_rate.txt) and prints
the same lines."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ofdm_mi355x as om  # noqa: E402

TAPS = np.array([0.3977, 0.7954 - 0.3977j, -0.1988, 0.0994, -0.0398])           # the reference channel (TX:64)
N, CP, KD, MOD, N_FRAMES, N_SYM = 2048, 144, 1200, "QPSK", 512, 240
NOISE_VAR = 1e-3
PEAK = 8e12                                                                      # bytes per second


def block(rx, call, s, reps):
    """reps calls -> (total, sync leg, demod leg) mean ms per call"""
    rx.set_profiling(True)                                   # restarts the handle's count
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        call()
    e1.record(s)
    e1.synchronize()
    sync_ms, demod_ms = rx.kernel_ms()
    return e0.elapsed_time(e1) / reps, sync_ms, demod_ms


def med(v):
    return "%7.3f ms (%.3f..%.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=N_FRAMES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chanavg_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    n_frames = a.frames
    fl = N_SYM * (N + CP)
    txe = om.TxEngine(N, CP, N - 2, KD, (1, 3), MOD)
    rx = om.RxEngine(N_SYM, N, CP, N - 2, (1, 3), KD, 30, 0.7, modulation=MOD)
    nds = rx.data_symbols_per_frame(fl)
    n_pat = N_SYM // 4
    nb = txe.bits_per_frame(N_SYM)
    d_bits = torch.empty(n_frames * nb, dtype=torch.uint8, device="cuda")
    d_tx = torch.empty(n_frames * fl * 2, dtype=torch.float32, device="cuda")
    d_iq = torch.empty(n_frames * fl * 2, dtype=torch.float32, device="cuda")
    taps = torch.from_numpy((TAPS / np.linalg.norm(TAPS)).astype(np.complex64).view(np.float32)).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = s.cuda_stream
    txe.random_bits(7, 0, d_bits, n_frames * nb, stream=ss)
    txe.modulate_frames(d_bits, n_frames, N_SYM, d_tx, stream=ss)
    txe.channel(d_tx, n_frames, fl, fl, taps, len(TAPS), d_iq, fl, fl, noise_var=NOISE_VAR, seed=3, stream=ss)
    s.synchronize()
    del d_tx
    d_eq = torch.empty(n_frames * nds * KD * 2, dtype=torch.float32, device="cuda")
    d_tsr = torch.zeros(n_frames * 4, dtype=torch.int32, device="cuda")
    rx.reserve(n_frames)
    rx.reserve_chan_average(n_frames, fl)

    def call():
        rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_tsr=d_tsr, stream=ss)

    lines = ["# tools/chanavg_rate.py --reps %d --rounds %d --frames %d on %s" % (a.reps, a.rounds, n_frames, torch.cuda.get_device_name(0)),
             "# %d-pt %d/%d %s, %d frames x %d symbols (%d data symbols, %d patterns)" % (N, CP, KD, MOD, n_frames, N_SYM, nds, n_pat),
             "# median over the rounds (min..max); a round = the mean of %d calls, off and on alternating" % a.reps]
    demod_bytes = n_frames * nds * (N * 8 + KD * 8)
    with torch.cuda.stream(s):
        for n_avg in (4, 16, -1):
            res = {False: [], True: []}
            for on in (False, True):
                rx.set_chan_average(n_avg if on else 0)
                for _ in range(3):
                    call()
            s.synchronize()
            found = int((d_tsr.view(n_frames, 4)[:, 3] == 1).sum())
            for _ in range(a.rounds):
                for on in (False, True):
                    rx.set_chan_average(n_avg if on else 0)
                    res[on].append(block(rx, call, s, a.reps))
            rx.set_chan_average(0)
            off, on = res[False], res[True]
            add_total = [b[0] - x[0] for x, b in zip(off, on)]
            add_sync = [b[1] - x[1] for x, b in zip(off, on)]
            n = n_pat if n_avg < 0 else min(n_avg, n_pat)
            chunks = (n + om.RxEngine.CHANAVG_CHUNK - 1) // om.RxEngine.CHANAVG_CHUNK
            stage_bytes = n_frames * (n * N * 8 + 2 * (chunks + 1) * N * 8 + N * 8 + KD * 8)
            t_stage, t_demod = statistics.median(add_sync) / 1e3, statistics.median([r[2] for r in off]) / 1e3
            lines += [
                "n_avg %3d (%d patterns, %d chunks per frame, %d frames with a sync): the stage's algorithmic bytes %.1f MB"
                % (n_avg, n, chunks, found, stage_bytes / 1e6),
                "  stage off : total %s | sync leg %s | demod leg %s" % tuple(med([r[i] for r in off]) for i in range(3)),
                "  stage on  : total %s | sync leg %s | demod leg %s" % tuple(med([r[i] for r in on]) for i in range(3)),
                "  added     : total %s | sync leg %s   (round by round, on - off)" % (med(add_total), med(add_sync)),
                "  stage: %.3f of 8 TB/s (%.2f TB/s) | demod leg, stage off: %.3f of 8 TB/s (%.2f TB/s over %.1f MB) | ratio %.2f"
                % (stage_bytes / t_stage / PEAK, stage_bytes / t_stage / 1e12, demod_bytes / t_demod / PEAK,
                   demod_bytes / t_demod / 1e12, demod_bytes / 1e6, (stage_bytes / t_stage) / (demod_bytes / t_demod)),
            ]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
