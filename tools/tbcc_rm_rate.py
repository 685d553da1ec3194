#!/usr/bin/env python3
"""Rate of the rate-matched TBCC calls: ofdm_tx_tbcc_encode_rm_frames, ofdm_tbcc_rate_dematch_frames, ofdm_tbcc_decode_rm_frames
(de-matching fused into the decoder's tile load) and the two-launch path de-match + ofdm_tbcc_decode_frames.

  batch    : that of tools/tbcc_rate.py -- 2048-pt 144/1200 16-QAM, 512 frames of 240 symbols (864000 LLRs per frame); device
             transmitter with rate-matched random information bits, reference 5-tap channel with noise, demod_frames_soft
  per case : K in {40, 256, 1024} x E in {ceil(1.5 K), 3K, 6K}, floor(864000 / E) blocks per frame; median time of each call
             (packed bits + metric + tb_ok), block errors of the fused call against the sent bits, and whether the fused outputs
             equal the two-launch path's
  yardstick: ofdm_tbcc_decode_frames of the PARENT commit's library (--parent-lib, built from a checkout of the parent) on the
             same K and block count as the E = 3K case, alternated with this build's in fresh child processes (--rounds each,
             OFDM_MI355X_LIB selects the library; Gaussian LLRs -- the decoder's time does not depend on the values)

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/tbcc_rm_rate.txt and, unless
--no-trace, runs itself once more with --quick under `rocprofv3 --kernel-trace --stats` (a fresh child process) and keeps the
kernel statistics as <outdir>/tbcc_rm_kernel_stats.csv."""
import argparse
import glob
import json
import os
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
SEG_BITS = 180 * KD * 4                                                            # 180 data symbols of 240


def es(K):
    return ((3 * K + 1) // 2, 3 * K, 6 * K)


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


def plain_only(frames, reps):
    """child process: the plain decoder of whichever library OFDM_MI355X_LIB names, one JSON line {K: ms}"""
    import ctypes
    import torch
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    torch.cuda.init()
    if os.environ.get("OFDM_MI355X_LIB"):          # a library of an older commit lacks the newer entry points: drop their prototypes
        raw = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.PROTOTYPES if not hasattr(raw, n)]:
            del _lib.PROTOTYPES[name]
    om.load()
    rx = om.RxEngine(N_SYM, N, CP, N - 2, (1, 3), KD, 100, 0.7, modulation=MOD)
    s = torch.cuda.Stream()
    out = {}
    for K in KS:
        nblk = SEG_BITS // (3 * K)
        nb = frames * nblk
        g = torch.Generator(device="cuda").manual_seed(K)
        d_llr = torch.randn(frames * SEG_BITS, generator=g, device="cuda", dtype=torch.float32) * 4
        d_dec = torch.empty(nb * K // 8, dtype=torch.uint8, device="cuda")
        d_m = torch.empty(nb, dtype=torch.float32, device="cuda")
        d_ok = torch.empty(nb, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rx.reserve_tbcc(nb, K)
        out[K] = 1e3 * timed(torch, lambda: rx.tbcc_decode_frames(d_llr, frames, SEG_BITS, nblk, K, d_bits=d_dec, bits_mode=om.BITS_PACKED,
                                                                  d_metric=d_m, d_tb_ok=d_ok, stream=s.cuda_stream), s, reps)
        del d_llr, d_dec, d_m, d_ok
        torch.cuda.empty_cache()
    print("PLAIN " + json.dumps(out), flush=True)


def alternate(parent_lib, rounds, frames, reps, emit):
    """-> {K: (median ms of this build, median ms of the parent)} from alternating child processes"""
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for tag in ("parent", "this"):
            env = dict(os.environ)
            env.pop("OFDM_MI355X_LIB", None)
            if tag == "parent":
                env["OFDM_MI355X_LIB"] = parent_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--frames", str(frames), "--reps", str(reps)],
                               env=env, capture_output=True, text=True, timeout=600, check=True)
            line = [t for t in p.stdout.splitlines() if t.startswith("PLAIN ")][-1]
            runs[tag].append({int(k): v for k, v in json.loads(line[6:]).items()})
    res = {}
    for K in KS:
        a, b = [r[K] for r in runs["this"]], [r[K] for r in runs["parent"]]
        res[K] = (statistics.median(a), statistics.median(b))
        emit("plain decode K=%4d | parent %s ms (median %.3f, spread %.1f %%) | this build %s ms (median %.3f, %+.1f %% against the parent)" % (
            K, " ".join("%.3f" % v for v in b), res[K][1], 100 * (max(b) - min(b)) / res[K][1],
            " ".join("%.3f" % v for v in a), res[K][0], 100 * (res[K][0] / res[K][1] - 1)))
    return res


def measure(frames, reps, emit, parent_ms=None):
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
    assert seg_bits == SEG_BITS
    nds = rx.data_symbols_per_frame(fl + CP)
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    flr = fl + CP
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
    emit("# %d-pt %s, %d frames x %d symbols (%d LLRs per frame, %.2f GB of LLRs), noise_var 0.02; times in ms, median of %d" % (
        N, MOD, frames, N_SYM, seg_bits, frames * seg_bits * 4 / 1e9, reps))
    for K in KS:
        for E in es(K):
            nblk = om.tbcc_rm_blocks(seg_bits, K, E)
            nb = frames * nblk
            d_rand = torch.empty(nb * K, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            txe.random_bits(7 + K + E, 0, d_rand, nb * K, stream=ss)
            s.synchronize()
            w = (2 ** torch.arange(7, -1, -1, device="cuda", dtype=torch.int32))
            d_info = (d_rand.view(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)
            del d_rand
            d_mid = torch.empty(nb * 3 * K, dtype=torch.float32, device="cuda")
            outs = [(torch.empty(nb * K // 8, dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.float32, device="cuda"),
                     torch.empty(nb, dtype=torch.int32, device="cuda")) for _ in range(2)]
            torch.cuda.synchronize()
            t_enc = timed(torch, lambda: txe.tbcc_encode_rm_frames(d_info, frames, nblk, K, E, d_coded, seg_bits, info_mode=om.BITS_PACKED,
                                                                   stream=ss), s, reps)
            txe.modulate_frames(d_coded, frames, N_SYM, d_tx, stream=ss)
            txe.channel(d_tx, frames, fl, fl, d_taps, len(taps), d_iq, flr, flr, noise_var=0.02, seed=3, stream=ss)
            rx.demod_frames_soft(d_iq, frames, flr, flr, d_eq, d_llr=d_llr, stream=ss)
            rx.reserve_tbcc(nb, K)
            t_dem = timed(torch, lambda: rx.tbcc_rate_dematch_frames(d_llr, frames, seg_bits, nblk, K, E, d_mid, nblk * 3 * K, stream=ss), s, reps)
            t_plain = timed(torch, lambda: rx.tbcc_decode_frames(d_mid, frames, nblk * 3 * K, nblk, K, d_bits=outs[0][0], bits_mode=om.BITS_PACKED,
                                                                 d_metric=outs[0][1], d_tb_ok=outs[0][2], stream=ss), s, reps)
            t_fused = timed(torch, lambda: rx.tbcc_decode_rm_frames(d_llr, frames, seg_bits, nblk, K, E, d_bits=outs[1][0],
                                                                    bits_mode=om.BITS_PACKED, d_metric=outs[1][1], d_tb_ok=outs[1][2],
                                                                    stream=ss), s, reps)
            s.synchronize()
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs))
            wrong = int((outs[1][0].view(nb, K // 8) != d_info.view(nb, K // 8)).any(1).sum())
            line = ("K=%4d E=%5d %7d blocks | encode_rm %7.3f | de-match %7.3f | plain decode of it %8.3f | de-match + plain %8.3f | "
                    "fused %8.3f = %.3f of the two launches | fused == two launches: %s | block errors %d" % (
                        K, E, nb, t_enc * 1e3, t_dem * 1e3, t_plain * 1e3, (t_dem + t_plain) * 1e3, t_fused * 1e3,
                        t_fused / (t_dem + t_plain), same, wrong))
            if parent_ms and E == 3 * K:
                line += " | fused / parent's plain decode (same K and blocks) %.3f" % (t_fused * 1e3 / parent_ms[K][1])
            emit(line)
            del d_info, d_mid, outs
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="one short pass (32 frames, 3 repetitions), nothing written")
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "tools", "experiments", "libofdm_g_parent.so"))
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.plain_only:
        plain_only(a.frames, a.reps)
        return
    if a.quick:
        measure(32, 3, lambda t: print(t, flush=True))
        return
    os.makedirs(a.outdir, exist_ok=True)
    lines = ["# Generated by: python3 tools/tbcc_rm_rate.py"]

    def emit(t):
        print(t, flush=True)
        lines.append(t)
    parent_ms = None
    if os.path.exists(a.parent_lib):
        emit("# plain decoder (ofdm_tbcc_decode_frames), %d frames, floor(%d / 3K) blocks per frame, Gaussian LLRs: %d alternating child "
             "processes per library" % (a.frames, SEG_BITS, a.rounds))
        parent_ms = alternate(a.parent_lib, a.rounds, a.frames, a.reps, emit)
    else:
        emit("# no parent library at %s: the plain decoder of the parent commit was not measured" % a.parent_lib)
    measure(a.frames, a.reps, emit, parent_ms)
    with open(os.path.join(a.outdir, "tbcc_rm_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if a.no_trace or not shutil.which("rocprofv3"):
        return
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "tbcc_rm", "--",
                        sys.executable, os.path.abspath(__file__), "--quick"], check=True, timeout=600)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if found:
            shutil.copy(found[0], os.path.join(a.outdir, "tbcc_rm_kernel_stats.csv"))
            print("kernel statistics ->", os.path.join(a.outdir, "tbcc_rm_kernel_stats.csv"))


if __name__ == "__main__":
    main()
