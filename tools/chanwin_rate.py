#!/usr/bin/env python3
"""Cost of the delay-window channel-estimate denoising inside ofdm_rx_demod_frames: the same call on the same buffers with the
window off and on, alternating in one session.

  total     : device events around demod_frames on one stream
  sync leg  : the handle's own events (ofdm_rx_set_profiling): sync search + LS estimate, and -- window on -- the window launch
  demod leg : the handle's own events: FFT + equalise + de-map
  alone     : chan_window_frames on the same number of rows, out of place, events around the call

The stage moves about 16*N + 8*Kd bytes per frame (H row in and out, the gains out), one launch of ceil(frames / SLOTS)
workgroups: at 2048-pt, 512 frames that is 21 MB and 512 workgroups, so it should cost a launch and little more.  No threshold:
the added time is printed next to the sync leg's own time of the same session.

3 warm-up calls per mode, then --rounds (7) rounds of [--reps (8) calls off, --reps calls on]; a round's figure is the mean of its
calls, the result the median over the rounds with the min..max spread.  2048-pt 144/1200 QPSK, 512 frames of 240 symbols, frames
from the device transmitter and the reference 5-tap channel.  Writes --out (profiles/chanwin_rate.txt) and prints the same lines."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chanwin_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    fl = N_SYM * (N + CP)
    pre, post = CP // 4, 3 * CP // 4
    txe = om.TxEngine(N, CP, N - 2, KD, (1, 3), MOD)
    rx = om.RxEngine(N_SYM, N, CP, N - 2, (1, 3), KD, 30, 0.7, modulation=MOD)
    nds = rx.data_symbols_per_frame(fl)
    nb = txe.bits_per_frame(N_SYM)
    d_bits = torch.empty(N_FRAMES * nb, dtype=torch.uint8, device="cuda")
    d_tx = torch.empty(N_FRAMES * fl * 2, dtype=torch.float32, device="cuda")
    d_iq = torch.empty(N_FRAMES * fl * 2, dtype=torch.float32, device="cuda")
    taps = torch.from_numpy((TAPS / np.linalg.norm(TAPS)).astype(np.complex64).view(np.float32)).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = s.cuda_stream
    txe.random_bits(7, 0, d_bits, N_FRAMES * nb, stream=ss)
    txe.modulate_frames(d_bits, N_FRAMES, N_SYM, d_tx, stream=ss)
    txe.channel(d_tx, N_FRAMES, fl, fl, taps, len(TAPS), d_iq, fl, fl, noise_var=NOISE_VAR, seed=3, stream=ss)
    s.synchronize()
    del d_tx
    d_eq = torch.empty(N_FRAMES * nds * KD * 2, dtype=torch.float32, device="cuda")
    d_tsr = torch.zeros(N_FRAMES * 4, dtype=torch.int32, device="cuda")
    rx.reserve(N_FRAMES)

    def call():
        rx.demod_frames(d_iq, N_FRAMES, fl, fl, d_eq, d_tsr=d_tsr, stream=ss)

    res = {False: [], True: []}
    with torch.cuda.stream(s):
        for on in (False, True):
            rx.set_chan_window(pre if on else 0, post if on else 0)
            for _ in range(3):
                call()
        s.synchronize()
        found = int((d_tsr.view(N_FRAMES, 4)[:, 3] == 1).sum())
        for _ in range(a.rounds):
            for on in (False, True):
                rx.set_chan_window(pre if on else 0, post if on else 0)
                res[on].append(block(rx, call, s, a.reps))
        # the stage alone, out of place, on as many rows
        d_H = torch.randn(N_FRAMES * N * 2, dtype=torch.float32, device="cuda")
        d_Ho, d_g = torch.empty_like(d_H), torch.empty(N_FRAMES * KD * 2, dtype=torch.float32, device="cuda")
        d_t = torch.empty(N_FRAMES, dtype=torch.float32, device="cuda")
        alone = []
        for i in range(3 + a.rounds * a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            rx.chan_window_frames(d_H, d_tsr, N_FRAMES, pre, post, d_Ho, d_g, d_t, stream=ss)
            e1.record(s)
            e1.synchronize()
            if i >= 3:
                alone.append(e0.elapsed_time(e1))
    off, on = res[False], res[True]
    add_total = [b[0] - x[0] for x, b in zip(off, on)]
    add_sync = [b[1] - x[1] for x, b in zip(off, on)]
    mb = N_FRAMES * (16 * N + 8 * KD) / 1e6
    lines = [
        "# tools/chanwin_rate.py --reps %d --rounds %d on %s" % (a.reps, a.rounds, torch.cuda.get_device_name(0)),
        "# %d-pt %d/%d %s, %d frames x %d symbols (%d data symbols), %d frames with a sync; window (%d, %d); the stage moves %.1f MB"
        % (N, CP, KD, MOD, N_FRAMES, N_SYM, nds, found, pre, post, mb),
        "# median over the rounds (min..max); a round = the mean of %d calls, off and on alternating" % a.reps,
        "window off : total %s | sync leg %s | demod leg %s" % tuple(med([r[i] for r in off]) for i in range(3)),
        "window on  : total %s | sync leg %s | demod leg %s" % tuple(med([r[i] for r in on]) for i in range(3)),
        "added      : total %s | sync leg %s   (round by round, on - off)" % (med(add_total), med(add_sync)),
        "alone      : chan_window_frames, %d rows, out of place, events around the call %s = %.2f TB/s of the bytes above"
        % (N_FRAMES, med(alone), mb / 1e6 / (statistics.median(alone) / 1e3)),
        "added sync-leg time / sync leg (window off): %.3f" % (statistics.median(add_sync) / statistics.median([r[1] for r in off])),
    ]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
