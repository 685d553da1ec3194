"""The turbo decoder with early termination by CRC on the GPU (-m gpu): ofdm_turbo_decode_es_frames and
ofdm_tb_decode_es_frames against tests/turbo_es_ref.py (the contract in NumPy float32).  Every comparison is array_equal -- bits,
iteration counts, flags and the float32 LLRs by bit pattern -- and every output sits between poisoned guard bands.  The inputs
come from tests/turbo_es_cases.py, whose operating points tests/test_turbo_es_ref_host.py asserts on the reference alone: the
blocks compared here stop at 1, in between and never, inside one wave.  K is small on purpose: the freeze, exit and CRC logic
does not depend on K beyond the tile classes and the run boundaries, which have a case each."""
import functools

import numpy as np
import pytest

import lte_bits_ref as lb
import tb_cases
import tb_ref
import turbo_cases as tc
import turbo_es_cases as ec
import turbo_es_ref as er
import turbo_ref as tr

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def rx0(om, torch):
    """any receiver handle serves the decoder (it reads LLR buffers, not the handle's numerology)"""
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


class Guarded:
    """nbytes of device memory at .addr = allocation + 64 + off, everything poisoned (or holding `fill`); read() returns the
    payload after asserting that the bytes in front of it and the 64 behind it are still poison"""

    def __init__(self, om, nbytes, off=0, fill=None):
        self.nbytes, self.lo = int(nbytes), GUARD + off
        self.total = self.lo + self.nbytes + GUARD
        host = np.full(self.total, POISON, np.uint8)
        if fill is not None:
            host[self.lo:self.lo + self.nbytes] = np.ascontiguousarray(fill).view(np.uint8).ravel()
        self.buf = om.DeviceBuffer(self.total).upload(host)
        self.addr = self.buf.data_ptr() + self.lo

    def read(self, dtype=np.uint8):
        raw = self.buf.download(np.uint8, self.total)
        assert np.all(raw[:self.lo] == POISON), "%d bytes written IN FRONT of an output" % int((raw[:self.lo] != POISON).sum())
        tail = raw[self.lo + self.nbytes:]
        assert np.all(tail == POISON), "%d bytes written BEHIND an output" % int((tail != POISON).sum())
        return raw[self.lo:self.lo + self.nbytes].copy().view(dtype)

    def untouched(self):
        return bool(np.all(self.read() == POISON))


def dev(om, arr):
    arr = np.ascontiguousarray(arr)
    return om.DeviceBuffer(max(arr.nbytes, 4)).upload(arr)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_es(om, rx, llr_seg, bps, K, kind, lo, hi, packed=False, want=("bits", "llr", "iters", "ok"), stat_stride=0):
    """llr_seg [n_seg][stride] float32 -> (bits [n][K], llr [n][K], iters [n], crc_ok [n]) with n = n_seg * bps, each from a guarded
    buffer or None where not wanted (its buffer is then asserted untouched).  stat_stride > bps: the gaps must stay poison."""
    llr_seg = np.ascontiguousarray(llr_seg, np.float32)
    n_seg, stride = llr_seg.shape
    nb = n_seg * bps
    ss = stat_stride or bps
    g_bits = Guarded(om, nb * (K // 8 if packed else K), 1)
    g_llr = Guarded(om, nb * K * 4)
    g_it, g_ok = Guarded(om, (n_seg - 1) * ss + bps, 3), Guarded(om, (n_seg - 1) * ss + bps, 1)
    rx.turbo_decode_es_frames(dev(om, llr_seg), n_seg, stride, bps, K, *tc.QPP[K], kind, lo, hi,
                              d_bits=g_bits.addr if "bits" in want else None, bits_mode=om.BITS_PACKED if packed else om.BITS_UNPACKED,
                              d_llr_out=g_llr.addr if "llr" in want else None, d_iters=g_it.addr if "iters" in want else None,
                              d_crc_ok=g_ok.addr if "ok" in want else None, stat_stride=stat_stride)
    out = []
    for name, g, dtype in (("bits", g_bits, np.uint8), ("llr", g_llr, np.float32), ("iters", g_it, np.uint8), ("ok", g_ok, np.uint8)):
        if name not in want:
            assert g.untouched(), name
            out.append(None)
            continue
        raw = g.read(dtype)
        if name == "bits":
            raw = np.unpackbits(raw.reshape(nb, K // 8), axis=1, bitorder="big") if packed else raw.reshape(nb, K)
        elif name == "llr":
            raw = raw.reshape(nb, K)
        else:
            rows = np.full(n_seg * ss, POISON, np.uint8)
            rows[:raw.size] = raw
            rows = rows.reshape(n_seg, ss)
            assert np.all(rows[:, bps:] == POISON), "the gap between two segments' %s was written" % name
            raw = rows[:, :bps].reshape(nb)
        out.append(raw)
    return tuple(out)


def same(got, want, what=""):
    """the outputs that are not None equal the reference's, the LLRs by bit pattern"""
    for g, w, name in zip(got, want, ("bits", "llr", "iters", "crc_ok")):
        if g is None:
            continue
        if name == "llr":
            g, w = u32(g), u32(w)
        bad = np.flatnonzero(np.any(np.reshape(g != w, (len(w), -1)), axis=1))
        assert not len(bad), "%s %s differs in blocks %s: got %s, want %s" % (what, name, bad[:8], np.reshape(g, (len(w), -1))[bad[:2], :6],
                                                                         np.reshape(w, (len(w), -1))[bad[:2], :6])


def take(ref, idx):
    return tuple(np.asarray(a)[idx] for a in ref)


# ------------------------------------------------------------------------------------------ stop, freeze, exit
@pytest.mark.parametrize("lo,hi", ec.ITER_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("K", ec.SPREAD_KS)
def test_spread_cases_equal_the_reference(om, rx0, K, lo, hi):
    """17 CRC24B blocks per K, one per segment: blocks that stop at 1, in between and never share a wave; bits in both modes"""
    llr, _ = ec.spread(K)
    ref = ec.spread_ref(K, lo, hi)
    same(gpu_es(om, rx0, llr, 1, K, om.CRC24B, lo, hi), ref, "K=%d (%d, %d)" % (K, lo, hi))
    same(gpu_es(om, rx0, llr, 1, K, om.CRC24B, lo, hi, packed=True, want=("bits", "iters")), ref, "packed")


@pytest.mark.parametrize("K", (40, 72))
def test_frozen_blocks_keep_their_outputs_under_a_long_running_neighbour(om, rx0, K):
    """one wave of 7 noiseless blocks and a noise-only one, at each of the 8 positions: the 7 stop at 1 and equal the fixed
    decoder's n_iter = 1 outputs after the wave has run 6 iterations (a frozen group that kept storing would not)"""
    for pos in range(8):
        llr = ec.neighbour_wave(K, pos)
        got = gpu_es(om, rx0, llr, 1, K, om.CRC24B, 1, ec.MAX_ITER)
        b1, o1 = tr.decode(llr, *tc.QPP[K], 1)
        b6, o6 = tr.decode(llr[pos:pos + 1], *tc.QPP[K], ec.MAX_ITER)
        b1[pos], o1[pos] = b6[0], o6[0]
        iters = np.ones(8, np.uint8)
        iters[pos] = ec.MAX_ITER
        same(got, (b1, o1, iters, (iters == 1).astype(np.uint8)), "pos %d" % pos)


def test_wave_exit_partial_groups_order_and_stride(om, rx0):
    """24 blocks = a wave that stops at 1 between two waves that run to max_iter; 1, 7, 8, 9 and 17 blocks; the same blocks in
    another order and at a seg_stride with poisoned gaps give the same per-block outputs"""
    K = 48
    per = 3 * K + 12
    slow, _ = ec.spread(K)
    never = np.flatnonzero(ec.spread_ref(K, 1, ec.MAX_ITER)[3] == 0)
    assert len(never) >= 4
    fast = ec.noiseless(ec.crc_blocks(K, 8, lb.CRC24B, np.random.default_rng(77)), K)
    llr = np.concatenate([slow[:8], fast, slow[8:16]])
    ref = er.decode_es(llr, *tc.QPP[K], lb.CRC24B, 1, ec.MAX_ITER)
    assert np.all(ref[2][8:16] == 1) and ref[2][:8].max() == ec.MAX_ITER and ref[2][16:].max() == ec.MAX_ITER
    same(gpu_es(om, rx0, llr, 1, K, om.CRC24B, 1, ec.MAX_ITER), ref, "24 blocks")
    for n in tc.DEC_COUNTS:
        same(gpu_es(om, rx0, llr[4:4 + n], 1, K, om.CRC24B, 1, ec.MAX_ITER), take(ref, slice(4, 4 + n)), "%d blocks" % n)
    order = np.random.default_rng(78).permutation(24)
    wide = np.full((6, 4 * per + 37), np.nan, np.float32)    # 6 segments of 4 blocks, NaN-poisoned gaps
    wide[:, :4 * per] = llr[order].reshape(6, 4 * per)
    got = gpu_es(om, rx0, wide, 4, K, om.CRC24B, 1, ec.MAX_ITER)
    same(got, take(ref, order), "permuted, strided")
    again = gpu_es(om, rx0, wide, 4, K, om.CRC24B, 1, ec.MAX_ITER)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("n", (1, 2, 6))
@pytest.mark.parametrize("K", (40, 120, 512))
def test_min_equal_max_is_the_fixed_decoder_on_the_device(om, rx0, K, n):
    llr, _ = ec.spread(K)
    g_bits, g_llr = Guarded(om, ec.SPREAD_BLOCKS * K), Guarded(om, ec.SPREAD_BLOCKS * K * 4)
    rx0.turbo_decode_frames(dev(om, llr), ec.SPREAD_BLOCKS, 3 * K + 12, 1, K, *tc.QPP[K], n, d_bits=g_bits.addr, d_llr_out=g_llr.addr)
    bits, out, iters, _ = gpu_es(om, rx0, llr, 1, K, om.CRC24B, n, n)
    assert np.array_equal(bits.ravel(), g_bits.read()) and np.array_equal(u32(out).ravel(), g_llr.read(np.uint32))
    assert np.all(iters == n)


# ------------------------------------------------------------------------------------------ the CRC
@pytest.mark.parametrize("kind", (lb.CRC24A, lb.CRC24B, lb.CRC16, lb.CRC8), ids=("24A", "24B", "16", "8"))
def test_every_crc_kind_on_blocks_terminated_with_it(om, rx0, kind):
    K, llr, _, ref = ec.kind_case(kind)
    same(gpu_es(om, rx0, llr.reshape(1, -1), 9, K, kind, 1, ec.MAX_ITER), ref, "kind %d" % kind)


def test_crc8_false_passes_and_the_wrong_kind(om, rx0):
    """noise-only LLRs checked with CRC8 pass wrongly where the reference does; CRC24B blocks checked as CRC24A never pass"""
    llr, sent, ref = ec.false_pass()
    got = gpu_es(om, rx0, llr, 1, ec.FALSE_PASS_K, om.CRC8, 1, ec.MAX_ITER)
    same(got, ref, "CRC8")
    assert np.any((got[3] == 1) & np.any(got[0] != sent, axis=1))
    K, llr, _, _ = ec.kind_case(lb.CRC24B)
    ref = er.decode_es(llr, *tc.QPP[K], lb.CRC24A, 1, ec.MAX_ITER)
    got = gpu_es(om, rx0, llr, 1, K, om.CRC24A, 1, ec.MAX_ITER)
    same(got, ref, "24B as 24A")
    assert not got[3].any() and np.all(got[2] == ec.MAX_ITER)


@pytest.mark.parametrize("K", (40, 72, 512))
def test_crc_run_boundaries_single_flipped_bits(om, rx0, K):
    """K / 8 = 5 bytes (empty runs), 9 and 64 bytes over the group's 8 lanes; one wrong hard bit at the block's first bit, on
    both sides of the payload / parity boundary and at the last bit clears crc_ok after iteration 1"""
    ats = (0, K - 25, K - 24, K - 1)
    llr = np.concatenate([ec.flipped_bit(K, at) for at in ats] + [ec.noiseless(ec.crc_blocks(K, 1, lb.CRC24B, np.random.default_rng(5)), K)])
    ref = er.decode_es(llr, *tc.QPP[K], lb.CRC24B, 1, 1)
    assert ref[3].tolist() == [0, 0, 0, 0, 1]
    same(gpu_es(om, rx0, llr, 1, K, om.CRC24B, 1, 1), ref, "flipped bits")
    ref = er.decode_es(llr, *tc.QPP[K], lb.CRC24B, 1, 3)
    same(gpu_es(om, rx0, llr, 1, K, om.CRC24B, 1, 3), ref, "flipped bits, 3 iterations")


def test_the_largest_block(om, rx0):
    """K = 6144 (768 bytes, 96 per lane): 8 noiseless blocks and a noisy one, max_iter 2"""
    llr, ref = ec.big()
    assert ref[2].min() == 1 and ref[2][4] == ec.BIG_MAX_ITER
    same(gpu_es(om, rx0, llr, 1, ec.BIG_K, om.CRC24B, 1, ec.BIG_MAX_ITER), ref, "K=6144")


@functools.lru_cache(maxsize=None)
def edge_reference(K, lo, hi):
    llr = tc.edge_blocks(K)
    return (llr,) + er.decode_es(llr, *tc.QPP[K], lb.CRC24B, lo, hi)


@pytest.mark.parametrize("lo,hi", ((1, 3), (2, 3)))
@pytest.mark.parametrize("K", (40, 56, 72, 120))
def test_edge_values(om, rx0, K, lo, hi):
    """NaN, +-inf, +-0 and subnormals by bit pattern, small integers; all-zero and all-NaN LLRs decide all zeros and stop at
    min_iter with crc_ok = 1"""
    llr, *ref = edge_reference(K, lo, hi)
    got = gpu_es(om, rx0, llr, 1, K, om.CRC24B, lo, hi)
    same(got, ref, "edge")
    assert got[2][2] == lo and got[2][6] == lo and got[3][2] == 1 and got[3][6] == 1 and not got[0][2].any() and not got[0][6].any()


# ------------------------------------------------------------------------------------------ outputs, batch
def test_each_output_alone_and_the_stat_stride(om, rx0):
    K, bps = 64, 5
    llr, _ = ec.spread(K)
    ref = ec.spread_ref(K, 1, ec.MAX_ITER)
    seg = np.full((3, bps * (3 * K + 12) + 7), np.nan, np.float32)
    seg[:, :bps * (3 * K + 12)] = llr[:15].reshape(3, -1)
    want = take(ref, slice(0, 15))
    for names in (("bits",), ("llr",), ("iters",), ("ok",), ("bits", "llr", "iters", "ok")):
        for stat_stride in (0, bps, bps + 3):
            same(gpu_es(om, rx0, seg, bps, K, om.CRC24B, 1, ec.MAX_ITER, want=names, stat_stride=stat_stride), want, str(names))
    gpu_es(om, rx0, seg, bps, K, om.CRC24B, 1, ec.MAX_ITER, want=())       # no pointer at all: a no-op


def test_grid_of_twenty_thousand_blocks(om, rx0):
    """20 000 blocks of K = 40 (2 500 waves), block n of the batch = source block n mod 16: CRC24B blocks around the K = 40
    operating point, so that neighbouring waves leave at different iterations"""
    K = tc.GRID_K
    src, _ = ec.noisy(K, tc.GRID_SRC, ec.SPREAD[K][0], lb.CRC24B, seed=3)
    ref = er.decode_es(src, *tc.QPP[K], lb.CRC24B, 1, 4)
    assert len(set(ref[2].tolist())) >= 3
    pick = np.arange(tc.GRID_BLOCKS) % tc.GRID_SRC
    bps = 10
    seg = np.full((tc.GRID_BLOCKS // bps, bps * (3 * K + 12) + 5), np.nan, np.float32)
    seg[:, :bps * (3 * K + 12)] = src[pick].reshape(tc.GRID_BLOCKS // bps, -1)
    same(gpu_es(om, rx0, seg, bps, K, om.CRC24B, 1, 4), take(ref, pick), "grid")


# ------------------------------------------------------------------------------------------ capture, errors
def test_capturable_after_reserve_and_refused_when_it_would_grow(om, torch):
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)         # a handle of its own: its workspace holds exactly what was reserved
    K, n_seg, bps = 120, 3, 5
    nb = n_seg * bps
    llr, _ = ec.spread(K)
    ref = take(ec.spread_ref(K, 1, ec.MAX_ITER), slice(0, nb))
    rx.reserve_turbo_es(nb, K)
    d_llr = torch.from_numpy(llr[:nb].reshape(n_seg, -1).copy()).cuda()
    big = torch.zeros(4 * nb * (3 * K + 12), dtype=torch.float32, device="cuda")
    outs = dict(bits=torch.zeros(nb * K, dtype=torch.uint8, device="cuda"), llr=torch.zeros(nb * K, dtype=torch.float32, device="cuda"),
                iters=torch.zeros(nb, dtype=torch.uint8, device="cuda"), ok=torch.zeros(nb, dtype=torch.uint8, device="cuda"))
    s = torch.cuda.Stream()

    def call(stream, d=d_llr, n=n_seg):
        rx.turbo_decode_es_frames(d, n, bps * (3 * K + 12), bps, K, *tc.QPP[K], om.CRC24B, 1, ec.MAX_ITER, d_bits=outs["bits"],
                                  d_llr_out=outs["llr"], d_iters=outs["iters"], d_crc_ok=outs["ok"], stream=stream)

    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="reserve_turbo_es"):
            call(torch.cuda.current_stream().cuda_stream, d=big, n=4 * n_seg)
    assert not outs["llr"].any() and not outs["iters"].any()                # capture enqueues nothing
    for _ in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = (outs["bits"].cpu().numpy().reshape(nb, K), outs["llr"].cpu().numpy().reshape(nb, K), outs["iters"].cpu().numpy(),
               outs["ok"].cpu().numpy())
        same(got, ref, "replay")


def test_argument_errors_leave_poisoned_outputs_untouched(om, rx0):
    import ctypes as C
    from ofdm_mi355x import _lib
    K, bps, n_seg = 40, 2, 3
    f1, f2 = tc.QPP[K]
    per = 3 * K + 12
    d_llr = dev(om, np.ones((n_seg, bps * per), np.float32))
    gs = [Guarded(om, n_seg * bps * K), Guarded(om, n_seg * bps * K * 4), Guarded(om, n_seg * bps), Guarded(om, n_seg * bps)]

    def dec(n_seg_=n_seg, stride=bps * per, bps_=bps, K_=K, f1_=f1, f2_=f2, kind=om.CRC24B, lo=1, hi=6, mode=om.BITS_UNPACKED, ss=0):
        out = _lib.TurboEsOut(gs[0].addr, mode, gs[1].addr, gs[2].addr, gs[3].addr, ss)
        rc = om.load().ofdm_turbo_decode_es_frames(rx0._h, d_llr.data_ptr(), n_seg_, stride, bps_, K_, f1_, f2_, kind, lo, hi, C.byref(out), None)
        _lib.check(rc)

    for kw in (dict(K_=44), dict(K_=32), dict(K_=6152), dict(f1_=2), dict(f1_=K), dict(f2_=-1), dict(lo=0), dict(hi=17), dict(lo=4, hi=3),
               dict(kind=4), dict(kind=-1), dict(stride=bps * per - 1), dict(n_seg_=-1), dict(bps_=-1), dict(n_seg_=2 ** 31, bps_=2),
               dict(stride=2 ** 41), dict(mode=om.BITS_NONE), dict(ss=1), dict(ss=-2)):
        with pytest.raises(ValueError):
            dec(**kw)
    out = _lib.TurboEsOut(gs[0].addr, om.BITS_UNPACKED, gs[1].addr, gs[2].addr, gs[3].addr, 0)
    assert om.load().ofdm_turbo_decode_es_frames(None, d_llr.data_ptr(), n_seg, bps * per, bps, K, f1, f2, om.CRC24B, 1, 6, C.byref(out), None) != 0
    for bad in ((4, 20), (-1, 40), (4, 6152)):
        with pytest.raises(ValueError):
            rx0.reserve_turbo_es(*bad)
    dec(n_seg_=0)                                                           # no-ops
    dec(bps_=0)
    rx0.turbo_decode_es_frames(d_llr, n_seg, bps * per, bps, K, f1, f2, om.CRC24B, 1, 6)
    assert all(g.untouched() for g in gs)


# ------------------------------------------------------------------------------------------ transport block
def gpu_tb_es(om, rx, llr, A, Z, G, lo, hi, q=1, rv=0, old=None, want_iters=True):
    """llr [n_tb][stride] -> (payload, tb_ok, cb_ok [n_tb][C], syndrome, soft [n_tb][soft_floats], cb_iters [n_tb][C]), every
    output from a guarded buffer; old: the soft buffer holds it and the call accumulates"""
    llr = np.ascontiguousarray(llr, np.float32)
    n_tb, stride = llr.shape
    qm, qp = tb_cases.pairs(A, Z)
    geo = tb_ref.geometry(A, Z)
    sf, C = geo["soft_floats"], geo["C"]
    g_soft = Guarded(om, n_tb * sf * 4, fill=old)
    g_pay, g_tb, g_cb, g_syn, g_it = Guarded(om, n_tb * A, 1), Guarded(om, n_tb), Guarded(om, n_tb * C), Guarded(om, n_tb * 4), Guarded(om, n_tb * C, 3)
    rx.tb_decode_es_frames(dev(om, llr), n_tb, stride, A, G, qp, g_soft.addr, sf, lo, hi, qpp_minus=qm, Z=Z, q=q, rv=rv,
                           accumulate=old is not None, d_payload=g_pay.addr, d_tb_ok=g_tb.addr, d_cb_ok=g_cb.addr, d_syndrome=g_syn.addr,
                           d_cb_iters=g_it.addr if want_iters else None)
    if not want_iters:
        assert g_it.untouched()
    return (g_pay.read().reshape(n_tb, A), g_tb.read(), g_cb.read().reshape(n_tb, C), g_syn.read(np.uint32),
            g_soft.read(np.float32).reshape(n_tb, sf), g_it.read().reshape(n_tb, C) if want_iters else None)


def same_tb(got, want, what=""):
    for g, w, name in zip(got, want, ("payload", "tb_ok", "cb_ok", "syndrome", "soft", "cb_iters")):
        if g is None:
            continue
        if name == "soft":
            g, w = u32(g), u32(w)
        assert np.array_equal(g, w), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("A,Z,esn0", ((976, 528, -4.0), (80, 64, -4.0), (496, 528, -4.0)), ids=("two-K528", "three-groups", "C1-crc24a"))
def test_transport_block_stops_each_code_block_at_its_own_iteration(om, rx0, A, Z, esn0):
    """full G with noise: two K = 528 blocks with filler; K- and K+ groups (C = 3); C = 1, where CRC24A is the stop check"""
    n_tb = 9
    qm, qp = tb_cases.pairs(A, Z)
    G = tb_cases.full_g(A, Z)
    p = tb_cases.payloads(A, n_tb, seed=21)
    llr = tr.awgn_llrs(tb_ref.encode(p, G, qm, qp, Z=Z), esn0, np.random.default_rng(37000 + A))
    want = er.tb_decode_es(llr, A, G, qm, qp, 1, ec.MAX_ITER, Z=Z)
    print("A=%d Z=%d: cb_iters %s tb_ok %s" % (A, Z, want[5].tolist(), want[1].tolist()))
    assert len(set(want[5].ravel().tolist())) >= 2
    same_tb(gpu_tb_es(om, rx0, llr, A, Z, G, 1, ec.MAX_ITER), want, "(1, 6)")
    same_tb(gpu_tb_es(om, rx0, llr, A, Z, G, 2, 3, want_iters=False), er.tb_decode_es(llr, A, G, qm, qp, 2, 3, Z=Z), "(2, 3)")


def test_harq_rounds_first_round_runs_out_second_round_stops_early(om, rx0):
    """tb_cases.harq_rounds(): round 1 (E < K + 4) ends with every block at max_iter and tb_ok = 0; with rv 2 accumulated every
    tb_ok is 1 and most blocks stop early -- 'most' is the count the reference gives"""
    A, Z, G, q, hi = tb_cases.HARQ_A, tb_cases.HARQ_Z, tb_cases.HARQ_G, tb_cases.HARQ_Q, tb_cases.HARQ_ITERS
    qm, qp = tb_cases.pairs(A, Z)
    p, l0, l2 = tb_cases.harq_rounds()
    want0 = er.tb_decode_es(l0, A, G, qm, qp, 1, hi, Z=Z, q=q, rv=0)
    got0 = gpu_tb_es(om, rx0, l0, A, Z, G, 1, hi, q=q, rv=0)
    same_tb(got0, want0, "round 1")
    assert not got0[1].any() and np.all(got0[5] == hi)
    want1 = er.tb_decode_es(l2, A, G, qm, qp, 1, hi, Z=Z, q=q, rv=2, soft=want0[4])
    got1 = gpu_tb_es(om, rx0, l2, A, Z, G, 1, hi, q=q, rv=2, old=got0[4])
    same_tb(got1, want1, "round 2")
    early = int((want1[5] < hi).sum())
    print("HARQ round 2: %d of %d blocks stop before max_iter, histogram %s" % (early, want1[5].size, np.bincount(want1[5].ravel(), minlength=hi + 1).tolist()))
    assert got1[1].all() and np.array_equal(got1[0], p) and int((got1[5] < hi).sum()) == early and 2 * early > want1[5].size


def test_transport_block_capture_and_errors(om, torch):
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    A, Z, n_tb = 80, 64, 4
    qm, qp = tb_cases.pairs(A, Z)
    G = tb_cases.full_g(A, Z)
    sf = tb_ref.geometry(A, Z)["soft_floats"]
    llr = tr.awgn_llrs(tb_ref.encode(tb_cases.payloads(A, n_tb, seed=22), G, qm, qp, Z=Z), -3.0, np.random.default_rng(38000))
    want = er.tb_decode_es(llr, A, G, qm, qp, 1, ec.MAX_ITER, Z=Z)
    rx.reserve_tb_es(n_tb, A, Z=Z)
    d_l = torch.from_numpy(llr.copy()).cuda()
    d_big = torch.zeros(4 * n_tb * G, dtype=torch.float32, device="cuda")
    soft = torch.zeros(4 * n_tb * sf, dtype=torch.float32, device="cuda")
    pay = torch.zeros(n_tb * A, dtype=torch.uint8, device="cuda")
    its = torch.zeros(n_tb * 3, dtype=torch.uint8, device="cuda")
    tb_ok = torch.full((4 * n_tb,), 9, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        rx.tb_decode_es_frames(d_l, n_tb, G, A, G, qp, soft, sf, 1, ec.MAX_ITER, qpp_minus=qm, Z=Z, d_payload=pay, d_tb_ok=tb_ok, d_cb_iters=its, stream=cs)
        with pytest.raises(ValueError, match="reserve_tb_es"):
            rx.tb_decode_es_frames(d_big, 4 * n_tb, G, A, G, qp, soft, sf, 1, ec.MAX_ITER, qpp_minus=qm, Z=Z, d_tb_ok=tb_ok, stream=cs)
    assert not its.any()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(pay.cpu().numpy().reshape(n_tb, A), want[0]) and np.array_equal(tb_ok.cpu().numpy()[:n_tb], want[1])
    assert np.array_equal(its.cpu().numpy().reshape(n_tb, 3), want[5]) and np.array_equal(u32(soft.cpu().numpy()[:n_tb * sf].reshape(n_tb, sf)), u32(want[4]))
    for kw in (dict(lo=0), dict(lo=3, hi=2), dict(hi=17)):
        a = dict(lo=1, hi=6)
        a.update(kw)
        its.zero_()
        with pytest.raises(ValueError):
            rx.tb_decode_es_frames(d_l, n_tb, G, A, G, qp, soft, sf, a["lo"], a["hi"], qpp_minus=qm, Z=Z, d_cb_iters=its)
        torch.cuda.synchronize()
        assert not its.any()
