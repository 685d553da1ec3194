#!/usr/bin/env python3
"""Cost of tracking the channel across a frame's sync symbols: ofdm_rx_demod_frames_track (eq only, OFDM_TRACK_LINEAR, window off)
next to ofdm_rx_demod_frames on the same buffers, alternating in one session, and the stage alone (ofdm_chan_track_frames on the
tsr the call returned).

  demod_frames        : device events around the call; its sync and demod legs from the handle's own events (ofdm_rx_set_profiling)
  demod_frames_track  : device events around the call (the same sync launch, then the stage)
  stage               : device events around chan_track_frames: the estimate launch, the link launch and the demod launch

The stage's algorithmic bytes are every symbol of the frame read once (sync and data), eq written and the a_p rows written once.
They are put over the stage's time as a fraction of 8 TB/s, next to the same figure for the demod leg of demod_frames in the same
session (its data symbols read, its equalised bins written): the same access pattern on the same chip.  No threshold.

3 warm-up calls each, then --rounds (7) rounds of [--reps (8) calls of each]; a round's figure is the mean of its calls, the result
the median over the rounds with the min..max spread.  2048-pt 144/1200 QPSK, 512 frames of 240 symbols, frames from the device
transmitter and the reference 5-tap channel.  Writes --out (profiles/chantrack_rate.txt) and prints the same lines."""
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


def timed(call, s, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        call()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def med(v):
    return "%7.3f ms (%.3f..%.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=N_FRAMES)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chantrack_rate.txt"))
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
    rx.reserve_chan_track(n_frames, fl)

    def plain():
        rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_tsr=d_tsr, stream=ss)

    def tracked():
        rx.demod_frames_track(d_iq, n_frames, fl, fl, om.TRACK_LINEAR, d_eq, d_tsr=d_tsr, stream=ss)

    def stage():
        rx.chan_track_frames(d_iq, n_frames, fl, fl, d_tsr, om.TRACK_LINEAR, 0, 0, d_eq, stream=ss)

    res = dict(plain=[], sync=[], demod=[], tracked=[], stage=[])
    with torch.cuda.stream(s):
        for call in (plain, tracked, stage):
            for _ in range(3):
                call()
        s.synchronize()
        found = int((d_tsr.view(n_frames, 4)[:, 3] == 1).sum())
        for _ in range(a.rounds):
            rx.set_profiling(True)                           # restarts the handle's count
            res["plain"].append(timed(plain, s, a.reps))
            sync_ms, demod_ms = rx.kernel_ms()
            rx.set_profiling(False)
            res["sync"].append(sync_ms)
            res["demod"].append(demod_ms)
            res["tracked"].append(timed(tracked, s, a.reps))
            res["stage"].append(timed(stage, s, a.reps))
    demod_bytes = n_frames * nds * (N * 8 + KD * 8)
    stage_bytes = n_frames * (N_SYM * N * 8 + nds * KD * 8 + n_pat * N * 8)
    t_stage, t_demod = statistics.median(res["stage"]) / 1e3, statistics.median(res["demod"]) / 1e3
    lines = ["# tools/chantrack_rate.py --reps %d --rounds %d --frames %d on %s" % (a.reps, a.rounds, n_frames, torch.cuda.get_device_name(0)),
             "# %d-pt %d/%d %s, %d frames x %d symbols (%d data symbols, %d patterns), %d frames with a sync"
             % (N, CP, KD, MOD, n_frames, N_SYM, nds, n_pat, found),
             "# median over the rounds (min..max); a round = the mean of %d calls of each, alternating" % a.reps,
             "  demod_frames       : total %s | sync leg %s | demod leg %s" % (med(res["plain"]), med(res["sync"]), med(res["demod"])),
             "  demod_frames_track : total %s" % med(res["tracked"]),
             "  stage alone        : total %s   (chan_track_frames: estimate, link and demod launches)" % med(res["stage"]),
             "  added by tracking  : %s   (round by round, demod_frames_track - demod_frames)"
             % med([t - p for t, p in zip(res["tracked"], res["plain"])]),
             "  stage: %.1f MB, %.3f of 8 TB/s (%.2f TB/s) | demod leg: %.1f MB, %.3f of 8 TB/s (%.2f TB/s) | ratio %.2f"
             % (stage_bytes / 1e6, stage_bytes / t_stage / PEAK, stage_bytes / t_stage / 1e12, demod_bytes / 1e6,
                demod_bytes / t_demod / PEAK, demod_bytes / t_demod / 1e12, (stage_bytes / t_stage) / (demod_bytes / t_demod))]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
