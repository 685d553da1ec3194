#!/usr/bin/env python3
"""Rate of the CRC and scrambling calls of csrc/bitproc.hip: ofdm_descramble_llr_frames, ofdm_tx_scramble_frames (both layouts),
ofdm_tx_crc_attach_frames and ofdm_crc_check_frames, next to ofdm_tbcc_decode_rm_frames of the same blocks.

  batch    : that of tools/tbcc_rm_rate.py -- 2048-pt 144/1200 16-QAM, 512 frames of 240 symbols: 864000 LLRs / coded bits per
             frame, one c_init per frame.  The calls' times do not depend on the values: Gaussian LLRs, random bits.
  scramble : GB/s of 8 B per LLR (4 read + 4 written), 2 B per unpacked bit, 0.25 B per packed bit; yardstick: the best copy
             kernel of tools/ubench/copy_bw (--copy-bw, built from tools/ubench/copy_bw.hip) at the LLR call's byte count, run
             as a child process in the same session
  CRC      : K = A + 16 in {40, 1024} with CRC16 and a mask per block, E = 3K, floor(864000 / E) blocks per frame, both layouts;
             attach and check (ok + syndrome + payload) next to the decode of the same blocks (packed bits + metric + tb_ok)
  step     : decode_rm alone against descramble + decode_rm + check: what the stage adds to the coded receive step

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/bitproc_rate.txt."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

N, CP, KD, MOD, FRAMES, N_SYM = 2048, 144, 1200, "16QAM", 512, 240
SEG_BITS = 180 * KD * 4                                                            # 180 data symbols of 240
KS = (40, 1024)


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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--copy-bw", default=os.path.join(ROOT, "tools", "ubench", "copy_bw"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bitproc_rate: no GPU (a rate is measured on the device or not at all)")
    import ofdm_mi355x as om
    om.load()
    os.makedirs(args.outdir, exist_ok=True)
    lines = []

    def emit(t):
        print(t, flush=True)
        lines.append(t)

    F = args.frames
    emit("bitproc_rate: %s, %d frames x %d bits, median (min .. max) of %d calls, device events" % (
        torch.cuda.get_device_name(0), F, SEG_BITS, args.reps))
    rx = om.RxEngine(N_SYM, N, CP, N - 2, (1, 3), KD, 100, 0.7, modulation=MOD)
    tx = om.TxEngine(N, CP, N - 2, KD, (1, 3), MOD)
    rx.reserve_bitproc()
    tx.reserve_bitproc()
    s = torch.cuda.Stream()
    st = s.cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    d_cinit = torch.randint(0, 2 ** 31 - 1, (F,), generator=g, device="cuda", dtype=torch.int32)
    n = F * SEG_BITS

    def rate(name, fn, nbytes):
        med, lo, hi = timed(torch, fn, s, args.reps)
        emit("%-44s %8.3f ms (%.3f .. %.3f)  %8.1f GB/s of %.3f GB" % (name, med, lo, hi, nbytes / med / 1e6, nbytes / 1e9))
        return med

    # ---- scrambling
    d_llr = torch.randn(n, generator=g, device="cuda", dtype=torch.float32) * 4
    d_out = torch.empty_like(d_llr)
    rate("descramble_llr_frames", lambda: rx.descramble_llr_frames(d_llr, F, SEG_BITS, SEG_BITS, d_cinit, d_out, stream=st), 8 * n)
    rate("descramble_llr_frames in place", lambda: rx.descramble_llr_frames(d_out, F, SEG_BITS, SEG_BITS, d_cinit, d_out, stream=st), 8 * n)
    rate("torch copy_ of the same floats", lambda: d_out.copy_(d_llr), 8 * n)
    del d_out
    if os.path.exists(args.copy_bw):
        torch.cuda.synchronize()
        p = subprocess.run([args.copy_bw, "%.6f" % (4 * n / 2 ** 30)], capture_output=True, text=True, timeout=300)
        best = None
        for t in p.stdout.splitlines():
            m = re.match(r"(copy .*?)\s+([0-9.]+) ms\s+([0-9.]+) GB/s", t)
            if m and (best is None or float(m.group(3)) > best[1]):
                best = (m.group(1).strip(), float(m.group(3)), float(m.group(2)))
        if best:
            emit("copy_bw, %.3f GB read + as much written: best %s, %.3f ms, %.1f GB/s" % (4 * n / 1e9, best[0], best[2], best[1]))
        else:
            emit("copy_bw: no result (exit %d): %s" % (p.returncode, (p.stdout + p.stderr)[-300:]))
    else:
        emit("copy_bw: %s not built, yardstick not measured" % args.copy_bw)
    d_bits = torch.randint(0, 2, (n,), generator=g, device="cuda", dtype=torch.uint8)
    d_bo = torch.empty_like(d_bits)
    rate("scramble_frames, one bit per byte", lambda: tx.scramble_frames(d_bits, F, SEG_BITS, d_cinit, d_bo, stream=st), 2 * n)
    rate("scramble_frames, packed", lambda: tx.scramble_frames(d_bits, F, SEG_BITS, d_cinit, d_bo, mode=om.BITS_PACKED, stream=st), n // 4)
    del d_bits, d_bo

    # ---- CRC next to the decoder
    for K in KS:
        A, E = K - 16, 3 * K
        nblk = SEG_BITS // E
        nb = F * nblk
        d_mask = torch.randint(0, 1 << 16, (nb,), generator=g, device="cuda", dtype=torch.int32)
        d_m = torch.empty(nb, dtype=torch.float32, device="cuda")
        d_tb = torch.empty(nb, dtype=torch.int32, device="cuda")
        d_ok = torch.empty(nb, dtype=torch.uint8, device="cuda")
        d_syn = torch.empty(nb, dtype=torch.int32, device="cuda")
        rx.reserve_tbcc(nb, K)
        emit("K = %d (A = %d, CRC16), E = %d: %d blocks per frame, %d blocks" % (K, A, E, nblk, nb))
        dec_ms = None
        for packed in (True, False):
            mode, tag = (om.BITS_PACKED, "packed") if packed else (om.BITS_UNPACKED, "one bit per byte")
            per = (lambda bits: bits // 8) if packed else (lambda bits: bits)
            d_pay = torch.randint(0, 2 if not packed else 256, (nb * per(A),), generator=g, device="cuda", dtype=torch.uint8)
            d_info = torch.empty(nb * per(K), dtype=torch.uint8, device="cuda")
            d_po = torch.empty_like(d_pay)
            att = rate("  crc_attach_frames, %s" % tag, lambda: tx.crc_attach_frames(d_pay, nb, A, om.CRC16, d_info, d_mask=d_mask,
                       payload_mode=mode, info_mode=mode, stream=st), nb * (per(A) + per(K) + 4))
            dec = rate("  tbcc_decode_rm_frames -> %s bits" % tag, lambda: rx.tbcc_decode_rm_frames(d_llr, F, SEG_BITS, nblk, K, E,
                       d_bits=d_info, bits_mode=mode, d_metric=d_m, d_tb_ok=d_tb, stream=st), nb * (4 * E + per(K) + 8))
            chk = rate("  crc_check_frames, %s" % tag, lambda: rx.crc_check_frames(d_info, nb, A, om.CRC16, d_mask=d_mask, info_mode=mode,
                       d_ok=d_ok, d_syndrome=d_syn, d_payload=d_po, payload_mode=mode, stream=st), nb * (per(K) + per(A) + 9))
            emit("  %s: attach / decode = %.4f, check / decode = %.4f" % (tag, att / dec, chk / dec))
            if packed:
                dec_ms = dec

                def step():
                    rx.descramble_llr_frames(d_llr, F, SEG_BITS, SEG_BITS, d_cinit, d_llr, stream=st)
                    rx.tbcc_decode_rm_frames(d_llr, F, SEG_BITS, nblk, K, E, d_bits=d_info, bits_mode=mode, d_metric=d_m, d_tb_ok=d_tb, stream=st)
                    rx.crc_check_frames(d_info, nb, A, om.CRC16, d_mask=d_mask, info_mode=mode, d_ok=d_ok, d_syndrome=d_syn, stream=st)
                full = rate("  descramble + decode_rm + check (ok, syndrome)", step, nb * (12 * E + 2 * per(K) + 17))
                emit("  coded receive step: %.3f ms -> %.3f ms, %+.1f %%" % (dec_ms, full, 100 * (full / dec_ms - 1)))
            del d_pay, d_info, d_po
        del d_mask, d_m, d_tb, d_ok, d_syn
        torch.cuda.empty_cache()
    with open(os.path.join(args.outdir, "bitproc_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
