#!/usr/bin/env python3
"""Rate of the transport-block calls: ofdm_tx_tb_encode_frames and ofdm_tb_decode_frames, and the share of the three kernels
this layer adds (segment, concat, desegment) in them.

  per case : a transport block size A at Z = 6144 with G = 2 sum (K_r + 4) rounded to q = 2 (rate about 1/2), rv 0, n_tb
             transport blocks per call:
             - tb_encode_frames, and the same groups through turbo_encode_rm_frames alone (the launches the call makes, on the
               same buffers): the difference is the segment and the concat kernel
             - tb_decode_frames at n_iter 6, and the same groups through turbo_rate_dematch_frames and turbo_decode_frames
               alone: the difference is the desegment kernel
             - the yardstick: turbo_decode_frames on the same blocks, the larger part of the line above
  The 'new' columns are differences of two medians and include the gaps between launches.  The three kernels' own times come
  from a kernel trace of one case at a time, where each of them runs at one shape only:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/tb_rate.py --case I
  (profiles/tb_kernel_stats_A*.csv are the kernel_stats files of such runs).

Device events around each call on one stream, 3 warm-up calls, median of --reps.  Writes <outdir>/tb_rate.txt."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lte-gnu-radio-code_amd")]

CASES = ((6120, 512), (20000, 256), (75376, 64))             # A, transport blocks per call
N_ITER = 6
QPP_6144 = (263, 480)                                        # a pair with a good spread for the largest block (tests/turbo_cases.py)


def qpp_for(K):
    """a pair the library accepts for any K that is a multiple of 8: f1 odd and coprime to K, f2 the product of K's prime factors"""
    rad, n, p = 1, K, 2
    while n > 1:
        if n % p == 0:
            rad *= p
            while n % p == 0:
                n //= p
        p += 1
    return QPP_6144 if K == 6144 else (next(f for f in range(3, K, 2) if math.gcd(f, K) == 1), rad)


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


def measure(scale, reps, emit, cases=CASES):
    import torch
    import ofdm_mi355x as om
    torch.cuda.init()
    om.load()
    txe = om.TxEngine(64, 16, 62, 60)
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    s = torch.cuda.Stream()
    ss = s.cuda_stream
    emit("# Z = 6144, q = 2, rv 0, n_iter %d; times in ms, median of %d; 'new' columns are differences of two medians" % (N_ITER, reps))
    for A, n_tb in cases:
        n_tb = max(1, n_tb // scale)
        seg = om.tb_geometry(A)
        Ks = [seg["K_minus"]] * seg["C_minus"] + [seg["K_plus"]] * seg["C_plus"]
        G = 2 * ((2 * sum(K + 4 for K in Ks) + 1) // 2)
        g = om.tb_geometry(A, 0, G, 2)
        qpp = {K: qpp_for(K) for K in set(Ks)}
        qm, qp = qpp.get(seg["K_minus"], (0, 0)), qpp[seg["K_plus"]]
        sf, C = g["soft_floats"], g["C"]
        d_pay = torch.randint(0, 256, (n_tb * A // 8,), dtype=torch.uint8, device="cuda")
        d_cw = torch.empty(n_tb * G, dtype=torch.uint8, device="cuda")
        d_soft = torch.zeros(n_tb * sf, dtype=torch.float32, device="cuda")
        d_out = torch.empty(n_tb * A // 8, dtype=torch.uint8, device="cuda")
        d_tb = torch.empty(n_tb, dtype=torch.uint8, device="cuda")
        d_cb = torch.empty(n_tb * C, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                             # the fills above ran on the default stream
        txe.reserve_tb(n_tb, A, G, q=2)
        rx.reserve_tb(n_tb, A)
        enc = lambda: txe.tb_encode_frames(d_pay, n_tb, A, G, qp, d_cw, G, qpp_minus=qm, q=2, payload_mode=om.BITS_PACKED, stream=ss)  # noqa: E731
        t_enc = timed(torch, enc, s, reps)
        s.synchronize()
        d_llr = (4.0 - 8.0 * d_cw.to(torch.float32)) + 2.0 * torch.randn(n_tb * G, device="cuda")        # noisy LLRs of the codewords
        torch.cuda.synchronize()
        dec = lambda: rx.tb_decode_frames(d_llr, n_tb, G, A, G, qp, d_soft, sf, N_ITER, qpp_minus=qm, q=2, d_payload=d_out,  # noqa: E731
                                          payload_mode=om.BITS_PACKED, d_tb_ok=d_tb, d_cb_ok=d_cb, stream=ss)
        t_dec = timed(torch, dec, s, reps)
        s.synchronize()
        ok = int(d_tb.sum().item())
        same = bool((d_out == d_pay).all().item())
        # the launches the two calls make through the existing kernels, alone, on buffers of the same shapes
        d_info = {i: torch.randint(0, 256, (n_tb * x["count"] * x["K"] // 8,), dtype=torch.uint8, device="cuda") for i, x in enumerate(g["groups"])}
        d_coded = {i: torch.empty(n_tb * x["count"] * x["E"], dtype=torch.uint8, device="cuda") for i, x in enumerate(g["groups"])}
        d_bits = torch.empty(n_tb * sum(Ks) // 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def enc_only():
            for i, x in enumerate(g["groups"]):
                txe.turbo_encode_rm_frames(d_info[i], n_tb, x["count"], x["K"], *qpp[x["K"]], x["E"], d_coded[i], x["count"] * x["E"],
                                           info_mode=om.BITS_PACKED, stream=ss)

        def dematch_only():
            for x in g["groups"]:
                rx.turbo_rate_dematch_frames(d_llr[x["cw_bit_offset"]:], n_tb, G, x["count"], x["K"], x["E"], d_soft[x["soft_offset"]:], sf,
                                             stream=ss)

        def decode_only():
            off = 0
            for K, count in ((seg["K_minus"], seg["C_minus"]), (seg["K_plus"], seg["C_plus"])):
                if count:
                    rx.turbo_decode_frames(d_soft[off:], n_tb, sf, count, K, *qpp[K], N_ITER, d_bits=d_bits, bits_mode=om.BITS_PACKED, stream=ss)
                    off += count * (3 * K + 12)

        t_enc_only = timed(torch, enc_only, s, reps)
        t_dem = timed(torch, dematch_only, s, reps)
        t_turbo = timed(torch, decode_only, s, reps)
        new_tx, new_rx = t_enc - t_enc_only, t_dec - t_dem - t_turbo
        emit("A=%6d C=%3d K=%s G=%7d n_tb=%4d | tb_encode %8.3f (encoders alone %8.3f, segment + concat %7.3f) | tb_decode %9.3f (de-match %7.3f, "
             "turbo decode %9.3f, desegment %7.3f) | new kernels / turbo decode = %.4f | tb_ok %d of %d, payload %s" % (
                 A, C, sorted(set(Ks)), G, n_tb, t_enc, t_enc_only, new_tx, t_dec, t_dem, t_turbo, new_rx, (new_tx + new_rx) / t_turbo, ok, n_tb,
                 "equal" if same else "DIFFERS"))
        del d_pay, d_cw, d_soft, d_out, d_llr, d_info, d_coded, d_bits
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="one short pass (an eighth of the transport blocks, 3 repetitions), nothing written")
    ap.add_argument("--case", type=int, default=None, help="run only CASES[I] and write nothing (for a kernel trace)")
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.quick:
        measure(8, 3, lambda t: print(t, flush=True))
        return
    if a.case is not None:
        measure(1, a.reps, lambda t: print(t, flush=True), CASES[a.case:a.case + 1])
        return
    os.makedirs(a.outdir, exist_ok=True)
    lines = ["# Generated by: python3 tools/tb_rate.py"]

    def emit(t):
        print(t, flush=True)
        lines.append(t)
    measure(1, a.reps, emit)
    with open(os.path.join(a.outdir, "tb_rate.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
