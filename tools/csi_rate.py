#!/usr/bin/env python3
"""Rate of the channel-state-weighted LLR stage (ofdm_rx_demod_frames_csi / ofdm_demap_csi_frames) next to the llr-only soft
stage of ofdm_rx_demod_frames_soft, measured in the same session on the same buffers.

  csi stage  : median time of demod_frames_csi (llr only) minus that of demod_frames on the same batch, noise estimated and given
  soft stage : the same difference for demod_frames_soft with d_llr only -- the yardstick: both stages read 8 B per symbol per
               pass and write 4*bps B per symbol
  alone      : ofdm_demap_csi_frames / ofdm_demap_frames over the batch's d_eq
  ratio      : csi stage (noise estimated) / soft stage, and the min..max of every timed call over its median (run-to-run spread)

Device events around each call on one stream, 3 warm-up calls, median of --reps (15).  Frames come from the device transmitter
and the reference 5-tap channel with noise.  2048-pt 144/1200 with QPSK / 16-QAM / 64-QAM, 512 frames of 320 symbols (240 data
symbols), and 64-pt 16/60 QPSK, 4369 frames of 16 symbols.  Writes --out (profiles/csi_rate.txt) and prints the same lines."""
import argparse
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


def run(N, cp, Kd, mod, n_frames, n_sym, reps):
    bps = om._lib.MODULATION_BITS[mod]
    fl = n_sym * (N + cp)
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
    ss = s.cuda_stream
    txe.random_bits(7, 0, d_bits, n_frames * nb, stream=ss)
    txe.modulate_frames(d_bits, n_frames, n_sym, d_tx, stream=ss)
    txe.channel(d_tx, n_frames, fl, fl, taps, len(TAPS), d_iq, fl, fl, noise_var=1e-3, seed=3, stream=ss)
    s.synchronize()
    del d_tx
    d_eq = torch.empty(n_frames * seg * 2, dtype=torch.float32, device="cuda")
    d_pb = torch.empty(n_frames * seg * bps // 8, dtype=torch.uint8, device="cuda")
    d_llr = torch.empty(n_frames * seg * bps, dtype=torch.float32, device="cuda")
    d_a = torch.empty(n_frames * Kd, dtype=torch.float32, device="cuda")
    rx.reserve(n_frames)
    rx.reserve_soft(n_frames, seg)
    rx.reserve_csi(n_frames, nds, Kd)
    t = {}
    t["demod"] = timed(lambda: rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_pb, om.BITS_PACKED, None, stream=ss), s, reps)
    t["soft"] = timed(lambda: rx.demod_frames_soft(d_iq, n_frames, fl, fl, d_eq, d_llr=d_llr, d_bits=d_pb, bits_mode=om.BITS_PACKED,
                                                   stream=ss), s, reps)
    t["csi_est"] = timed(lambda: rx.demod_frames_csi(d_iq, n_frames, fl, fl, d_eq, d_llr, d_bits=d_pb, bits_mode=om.BITS_PACKED,
                                                     stream=ss), s, reps)
    t["csi_given"] = timed(lambda: rx.demod_frames_csi(d_iq, n_frames, fl, fl, d_eq, d_llr, noise_mode=om.CSI_NOISE_GIVEN,
                                                       noise_var=1e-3, d_bits=d_pb, bits_mode=om.BITS_PACKED, stream=ss), s, reps)
    t["soft_alone"] = timed(lambda: rx.demap_frames(d_eq, n_frames, seg, seg, mod, d_llr=d_llr, stream=ss), s, reps)
    rx.csi_frames(n_frames, d_a, stream=ss)
    t["csi_alone"] = timed(lambda: rx.demap_csi_frames(d_eq, n_frames, nds, Kd, seg, d_a, Kd, rx.csi_rho, mod, d_llr, stream=ss),
                           s, reps)
    t["csi_given_alone"] = timed(lambda: rx.demap_csi_frames(d_eq, n_frames, nds, Kd, seg, d_a, Kd, rx.csi_rho, mod, d_llr,
                                                             noise_mode=om.CSI_NOISE_GIVEN, noise_var=1e-3, stream=ss), s, reps)
    s.synchronize()
    n = n_frames * seg
    two_pass, one_pass = n * (16 + 4 * bps), n * (8 + 4 * bps)
    stage = {k: t[k][0] - t["demod"][0] for k in ("soft", "csi_est", "csi_given")}
    spread = max(max(t[k][2] / t[k][0] - 1, 1 - t[k][1] / t[k][0]) for k in t)
    return ("%4d-pt %-5s %4d frames x %3d data sym (eq %5.0f MB) | demod %7.3f ms | soft llr stage +%7.3f ms (%.2f of 8 TB/s) | "
            "csi stage est +%7.3f ms (%.2f), given +%7.3f ms (%.2f) | ratio csi/soft %.2f | alone: demap_frames %7.3f ms (%.2f), "
            "demap_csi_frames est %7.3f ms (%.2f), given %7.3f ms (%.2f) | spread of the timed calls +-%.1f %%" % (
                N, mod, n_frames, nds, n * 8 / 1e6, t["demod"][0] * 1e3, stage["soft"] * 1e3, two_pass / max(stage["soft"], 1e-12) / HBM,
                stage["csi_est"] * 1e3, two_pass / max(stage["csi_est"], 1e-12) / HBM, stage["csi_given"] * 1e3,
                one_pass / max(stage["csi_given"], 1e-12) / HBM, stage["csi_est"] / max(stage["soft"], 1e-12),
                t["soft_alone"][0] * 1e3, two_pass / t["soft_alone"][0] / HBM, t["csi_alone"][0] * 1e3, two_pass / t["csi_alone"][0] / HBM,
                t["csi_given_alone"][0] * 1e3, one_pass / t["csi_given_alone"][0] / HBM, spread * 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csi_rate.txt"))
    a = ap.parse_args()
    torch.cuda.init()
    om.load()
    lines = ["# tools/csi_rate.py --reps %d on %s; algorithmic bytes: 8 B per symbol per pass (two passes with the noise estimated, "
             "one with it given) + 4*bps B" % (a.reps, torch.cuda.get_device_name(0))]
    for cfg in CONFIGS:
        lines.append(run(*cfg, a.reps))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
