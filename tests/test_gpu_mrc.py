"""Receive-diversity combining on the GPU (-m gpu): ofdm_combine_csi_frames and ofdm_rx_demod_frames_mrc against tests/mrc_ref.py
(the contract of include/ofdm_mi355x.h in NumPy float32, pinned by test_mrc_ref_host.py).  Every comparison of llr, sym and weight
is array_equal on the bit patterns, every output sits between poisoned guard bands, and the shapes are those of the
channel-state-weighted LLR tests: odd rows, a tail shorter than one vector, a slice boundary inside a row, the 64-QAM tile of 128
symbols with remainders 1 and 127 -- each with a segment stride that is even and one that is odd in complex items, so that the
16-byte and the per-float store paths both run."""
import numpy as np
import pytest

import csi_ref
import mrc_cases as mc
import mrc_ref
from oracle import ofdm_oracle as orc
from test_gpu_csi import GUARD, Out, cur, demod, same_bits
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

MODS = ("QPSK", "16QAM", "64QAM")
BPS = csi_ref.BPS
SHAPES = [(1, 2), (1, 57), (3, 57), (9, 60), (2, 63), (5, 600), (4, 1200)]          # (rows, row_len)
BRANCHES = [1, 2, 3, 8]
RHO = 0.03
NOISE = (0.004, 0.01, 0.006, 0.02, 0.005, 0.008, 0.003, 0.012)                      # variance of branch b
KEYS = ("llr", "sym", "weight")
assert GUARD == 8


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
def rx0(om):
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


def branches(rng, B, n_seg, rows, row_len, mod):
    """-> z [B][n_seg][rows][row_len] complex64, a [B][n_seg][row_len] float32: the constellation points of a segment through B
    one-tap MMSE equalisers, branch b with the noise variance NOISE[b].  A few symbols sit on decision edges: a zero real or
    imaginary part in every branch makes that coordinate of u exactly 0, the edge of axis bit 0."""
    a = rng.uniform(0.02, 2.0, (B, n_seg, row_len))
    x = orc.map_bits(rng.integers(0, 2, n_seg * rows * row_len * BPS[mod]), mod).reshape(n_seg, rows, row_len)
    w = rng.standard_normal((B, n_seg, rows, row_len)) + 1j * rng.standard_normal((B, n_seg, rows, row_len))
    w *= np.sqrt(np.array(NOISE[:B]) / 2)[:, None, None, None]
    g = a[:, :, None, :]
    z = ((g / (g + RHO)) * (x[None] + w / np.sqrt(g))).astype(np.complex64)
    flat = z.reshape(B, n_seg, -1)
    n = rows * row_len
    flat[:, :, 0 % n].real = 0.0
    flat[:, :, 1 % n].imag = -0.0
    if n > 130:
        flat[:, :, 129].real = -0.0
    return z, a.astype(np.float32)


def layout(z, a, stride, csi_extra=3):
    """the units g = b*n_seg + s in one buffer: sym [B*n_seg][stride] (NaN in the gaps), csi [B*n_seg][row_len + csi_extra]"""
    B, n_seg, rows, row_len = z.shape
    sym = np.full((B * n_seg, stride), complex(np.nan, np.nan), np.complex64)
    sym[:, :rows * row_len] = z.reshape(B * n_seg, -1)
    csi = np.full((B * n_seg, row_len + csi_extra), np.nan, np.float32)
    csi[:, :row_len] = a.reshape(B * n_seg, row_len)
    return sym, csi


def run(torch, rx, sym, csi, B, n_seg, rows, row_len, mod, noise, want=KEYS, base_off=0, rho=RHO):
    """combine_csi_frames on host arrays -> dict of host arrays.  noise: B numbers (given) or an array of B*n_seg doubles
    (OFDM_MRC_NOISE_SEG).  base_off: bytes the symbols are moved off the 16-byte grid."""
    n = rows * row_len
    t = torch.zeros(sym.size * 2 + 4, dtype=torch.float32, device="cuda")
    t[base_off // 4:base_off // 4 + sym.size * 2] = torch.from_numpy(np.ascontiguousarray(sym).view(np.float32).ravel()).cuda()
    d_csi = torch.from_numpy(np.ascontiguousarray(csi)).cuda()
    o = dict(llr=Out(torch, n_seg * n * BPS[mod], torch.float32) if "llr" in want else None,
             sym=Out(torch, n_seg * n * 2, torch.float32) if "sym" in want else None,
             weight=Out(torch, n_seg * n, torch.float32) if "weight" in want else None)
    per_unit = isinstance(noise, np.ndarray)
    d_s2 = torch.from_numpy(np.ascontiguousarray(noise, np.float64)).cuda() if per_unit else None
    rx.combine_csi_frames(t.data_ptr() + base_off, B, n_seg, rows, row_len, sym.shape[1], d_csi, csi.shape[1], rho, mod,
                          noise_var=None if per_unit else noise, d_sigma2=d_s2, d_llr=o["llr"].addr if o["llr"] else None,
                          d_sym_out=o["sym"].addr if o["sym"] else None, d_weight=o["weight"].addr if o["weight"] else None,
                          stream=cur(torch))
    torch.cuda.synchronize()
    return {k: (v.read().copy() if v else None) for k, v in o.items()}


def check(got, ref, what):
    """got: run()'s dict; ref: (llr, sym, weight) of mrc_ref.combine_segments"""
    assert same_bits(got["llr"], ref[0].ravel()), ("llr", what)
    assert same_bits(got["sym"], np.ascontiguousarray(ref[1]).view(np.float32).ravel()), ("sym", what)
    assert same_bits(got["weight"], ref[2].ravel()), ("weight", what)
    for k in KEYS:
        assert np.isfinite(got[k]).all(), (k, what)


def strides(n):
    """(even, odd) segment strides in complex items and the byte offset of the buffer"""
    return ((n + (n & 1), 0), (n + 1 - (n & 1), 8))


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("n_seg", [1, 3])
@pytest.mark.parametrize("B", BRANCHES)
@pytest.mark.parametrize("rows,row_len", SHAPES)
@pytest.mark.parametrize("mod", MODS)
def test_against_the_reference(torch, rx0, mod, rows, row_len, B, n_seg):
    rng = np.random.default_rng(1000 * rows + row_len + 7 * n_seg + BPS[mod] + 100000 * B)
    z, a = branches(rng, B, n_seg, rows, row_len, mod)
    given = list(NOISE[:B])
    per_unit = (np.repeat(np.array(given), n_seg) * rng.uniform(0.8, 1.25, B * n_seg)).astype(np.float64)
    ref_given = mrc_ref.combine_segments(z, a, RHO, mod, given)
    ref_seg = mrc_ref.combine_segments(z, a, RHO, mod, per_unit.reshape(B, n_seg))
    assert ref_given[2].all() and not np.array_equal(ref_given[0], ref_seg[0])
    for stride, base_off in strides(rows * row_len):
        sym, csi = layout(z, a, stride)
        check(run(torch, rx0, sym, csi, B, n_seg, rows, row_len, mod, given, base_off=base_off), ref_given, ("given", stride))
        check(run(torch, rx0, sym, csi, B, n_seg, rows, row_len, mod, per_unit, base_off=base_off), ref_seg, ("seg", stride))


@pytest.mark.parametrize("mod", MODS)
def test_decision_edges(torch, rx0, mod):
    """a = 1, rho = 0 and variances that are powers of two: u = (z0 + z1)/2 exactly, planted on every boundary between two levels
    and on the levels themselves, in both coordinates"""
    bps = BPS[mod]
    lv = csi_ref.levels(bps)[0].astype(np.float32)
    mids = np.unique(np.concatenate([lv, ((lv[:, None] + lv[None, :]) / np.float32(2)).ravel()])).astype(np.float32)
    pts = (mids[:, None] + 1j * mids[None, :]).astype(np.complex64).ravel()
    pts = pts[pts != 0]                                      # 0 + 0j is an erasure, not a symbol
    z = np.stack([pts, pts]).reshape(2, 1, 1, -1)
    a = np.ones((2, 1, pts.size), np.float32)
    ref = mrc_ref.combine_segments(z, a, 0.0, mod, [0.25, 0.25])
    assert same_bits(np.ascontiguousarray(ref[1]).view(np.float32).ravel(), pts.view(np.float32)) and (ref[2] == 8.0).all()
    assert (ref[0] == 0).sum() >= mids.size                                           # ties: d = 0 exactly
    sym, csi = layout(z, a, pts.size + (pts.size & 1))
    check(run(torch, rx0, sym, csi, 2, 1, 1, pts.size, mod, [0.25, 0.25], rho=0.0), ref, "edges")


@pytest.mark.parametrize("mod", MODS)
def test_each_output_alone(torch, rx0, mod):
    rng = np.random.default_rng(5 + BPS[mod])
    B, n_seg, rows, row_len = 3, 3, 3, 600
    z, a = branches(rng, B, n_seg, rows, row_len, mod)
    for stride, base_off in strides(rows * row_len):
        sym, csi = layout(z, a, stride)
        full = run(torch, rx0, sym, csi, B, n_seg, rows, row_len, mod, list(NOISE[:B]), base_off=base_off)
        for k in KEYS:
            one = run(torch, rx0, sym, csi, B, n_seg, rows, row_len, mod, list(NOISE[:B]), want=(k,), base_off=base_off)
            assert same_bits(one[k], full[k]), (k, stride)
    idle = Out(torch, 16, torch.float32)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    nv = [0.1, 0.1]
    rx0.combine_csi_frames(d, 2, 0, 1, 2, 2, d, 2, RHO, mod, nv, d_llr=idle.addr, stream=cur(torch))          # n_seg = 0
    rx0.combine_csi_frames(d, 2, 1, 0, 2, 0, d, 2, RHO, mod, nv, d_llr=idle.addr, stream=cur(torch))          # rows = 0
    rx0.combine_csi_frames(d, 2, 1, 1, 2, 2, d, 2, RHO, mod, nv, stream=cur(torch))                           # no output
    torch.cuda.synchronize()
    assert idle.untouched()


# ------------------------------------------------------------------------------------------ 2. erasures
@pytest.mark.parametrize("mod", MODS)
def test_erasures(torch, rx0, mod):
    rng = np.random.default_rng(77 + BPS[mod])
    B, n_seg, rows, row_len = 3, 2, 5, 57
    n, bps = rows * row_len, BPS[mod]
    z, a = branches(rng, B, n_seg, rows, row_len, mod)
    z[1, 0] = 0                                              # branch 1 of segment 0 found no sync: zero symbols, zero channel
    a[1, 0] = 0
    z[0, 1, 2] = 0                                           # a guard-failed row of branch 0 in segment 1
    for j, v in zip((3, 11, 20, 31), (0.0, np.nan, np.inf, -1.0)):
        a[2, 0, j] = v                                       # entries of branch 2 without an estimate
    zf = z.reshape(B, n_seg, n)
    zf[0, 0, 40], zf[2, 0, 41], zf[1, 1, 42] = complex(np.nan, 0.1), complex(0.1, np.inf), complex(3e38, 0.1)
    zf[:, 1, 50] = [0j, complex(np.nan, np.nan), complex(np.inf, 0)]                    # every branch out of symbol 50 of segment 1
    zf[0, 0, 3], zf[1, 0, 3] = complex(0.2, np.nan), 0j                                 # ... and of symbol 3 of segment 0 (a = 0 in branch 2)
    s2 = np.repeat(np.array(NOISE[:B]), n_seg).reshape(B, n_seg)
    s2[2, 1] = 0.0                                           # sigma2 = 0 for one unit
    ref = mrc_ref.combine_segments(z, a, RHO, mod, s2)
    took = [mrc_ref.combine(z[:, s], a[:, s], RHO, mod, s2[:, s])[3] for s in range(n_seg)]
    assert not took[0][1].any() and not took[1][2].any() and not took[1][0, 2 * row_len:3 * row_len].any()
    assert not took[0][:, 3].any() and not took[1][:, 50].any() and took[0][0, 4] and not took[0][2, 11::row_len].any()
    for stride, base_off in strides(n):
        sym, csi = layout(z, a, stride)
        got = run(torch, rx0, sym, csi, B, n_seg, rows, row_len, mod, s2.ravel(), base_off=base_off)
        check(got, ref, stride)
        llr, w = got["llr"].reshape(n_seg, n, bps), got["weight"].reshape(n_seg, n)
        u = got["sym"].view(np.complex64).reshape(n_seg, n)
        zero = lambda v: not v.view(np.uint32).any()                                                   # noqa: E731
        for s, i in ((0, 3), (1, 50)):
            assert zero(llr[s, i]) and zero(w[s, i:i + 1]) and zero(u[s, i:i + 1].view(np.float32))
        assert llr[0, 4].any() and w[0, 4] > 0 and (w[1, 2 * row_len:3 * row_len] > 0).all()
        # the branches that are left carry the symbol: segment 0 without branch 1, segment 1 without branch 2 -- the same bits
        for s, keep in ((0, [0, 2]), (1, [0, 1])):
            sym2, csi2 = layout(z[keep][:, s:s + 1], a[keep][:, s:s + 1], stride)
            two = run(torch, rx0, sym2, csi2, 2, 1, rows, row_len, mod, s2[keep, s].copy(), base_off=base_off)
            assert same_bits(two["llr"], llr[s].ravel()) and same_bits(two["weight"], w[s]) and same_bits(two["sym"], u[s].view(np.float32))
    # no unit has a usable variance: every output +0
    sym, csi = layout(z, a, n + 1)
    got = run(torch, rx0, sym, csi, B, n_seg, rows, row_len, mod, np.zeros(B * n_seg))
    assert all(not got[k].view(np.uint32).any() for k in KEYS)


# ------------------------------------------------------------------------------------------ 3. the composite call
@pytest.mark.parametrize("N,mod", [(64, "QPSK"), (1024, "64QAM")])
def test_composite_equals_the_separate_calls(om, torch, N, mod):
    cp, Kd = GEOM[N]
    bps = BPS[mod]
    rng = np.random.default_rng(N + bps)
    B, nf = 2, 3
    iq = make_frames(N, mod, B * nf, 12, rng, no_sync=(nf + 1,), late=(2,))            # branch 1 of frame 1 is noise only
    n, fl = iq.shape
    rx, d_iq, nds = demod(om, N, mod, iq)
    n_eq, n_out = n * nds * Kd, nf * nds * Kd

    def outs():
        return dict(llr=Out(torch, n_out * bps, torch.float32), sym=Out(torch, n_out * 2, torch.float32),
                    weight=Out(torch, n_out, torch.float32))

    p_eq, p_tsr = Out(torch, n_eq * 2, torch.float32), Out(torch, n * 4, torch.int32)
    assert rx.demod_frames(d_iq, n, fl, fl, p_eq.addr, d_tsr=p_tsr.addr) == nds
    d_a = Out(torch, n * Kd, torch.float32)
    rx.csi_frames(n, d_a.addr)
    p_s2 = Out(torch, n, torch.float64)
    rx.demap_csi_frames(p_eq.addr, n, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, mod, d_sigma2=p_s2.addr)
    est = p_s2.read().copy()
    tsr = p_tsr.read().reshape(n, 4)
    assert tsr[nf + 1, 3] == 0 and est[nf + 1] == 0.0 and (np.delete(est, nf + 1) > 0).all()
    csi_s2 = Out(torch, n, torch.float64)                                              # what demod_frames_csi reports per frame
    scratch = Out(torch, n_eq * 2, torch.float32)
    assert rx.demod_frames_csi(d_iq, n, fl, fl, scratch.addr, d_sigma2=csi_s2.addr) == nds
    assert np.array_equal(csi_s2.read().view(np.uint64), est.view(np.uint64))
    given = [0.02, 0.03]
    for nv in (None, given):
        sep = outs()
        rx.combine_csi_frames(p_eq.addr, B, nf, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, mod, noise_var=nv,
                              d_sigma2=p_s2.addr if nv is None else None, d_llr=sep["llr"].addr, d_sym_out=sep["sym"].addr,
                              d_weight=sep["weight"].addr)
        c, c_eq, c_tsr, c_s2 = outs(), Out(torch, n_eq * 2, torch.float32), Out(torch, n * 4, torch.int32), Out(torch, n, torch.float64)
        r = rx.demod_frames_mrc(d_iq, B, nf, fl, fl, c_eq.addr, nv, c["llr"].addr, c["sym"].addr, c["weight"].addr, c_s2.addr,
                                c_tsr.addr)
        assert r == nds
        assert same_bits(c_eq.read(), p_eq.read()) and np.array_equal(c_tsr.read(), p_tsr.read())
        want_s2 = est if nv is None else np.repeat(np.array(given), nf)
        assert np.array_equal(c_s2.read().view(np.uint64), want_s2.view(np.uint64)), nv
        for k in KEYS:
            assert same_bits(c[k].read(), sep[k].read()), (k, nv)
            assert np.isfinite(c[k].read()).all()
        # against the reference on the downloaded symbols
        eq = p_eq.read().view(np.complex64).reshape(B, nf, nds, Kd)
        a = d_a.read().reshape(B, nf, Kd)
        ref = mrc_ref.combine_segments(eq, a, rx.csi_rho, mod, want_s2.reshape(B, nf))
        check({k: c[k].read() for k in KEYS}, ref, nv)
        # frame 1: branch 1 is pure noise (no sync) and leaves branch 0's result -- the same bits as branch 0 alone
        alone = outs()
        rx.combine_csi_frames(p_eq.addr + 8 * nds * Kd, 1, 1, nds, Kd, nds * Kd, d_a.addr + 4 * Kd, Kd, rx.csi_rho, mod,
                              noise_var=None if nv is None else given[:1], d_sigma2=p_s2.addr + 8 if nv is None else None,
                              d_llr=alone["llr"].addr, d_sym_out=alone["sym"].addr, d_weight=alone["weight"].addr)
        per = nds * Kd
        for k, m in (("llr", bps), ("sym", 2), ("weight", 1)):
            assert same_bits(alone[k].read()[:per * m], c[k].read()[per * m:2 * per * m]), (k, nv)
        assert c["weight"].read()[per:2 * per].any()
        # frame 2 of branch 0 ends in guard-failed rows: branch 1 carries them
        assert not eq[0, 2, -1].any() and (c["weight"].read().reshape(nf, nds, Kd)[2, -1] > 0).all()
    # sigma2 alone, and nothing wanted: the plain call
    only = Out(torch, n, torch.float64)
    assert rx.demod_frames_mrc(d_iq, B, nf, fl, fl, scratch.addr, d_sigma2=only.addr) == nds
    assert np.array_equal(only.read().view(np.uint64), est.view(np.uint64))
    assert rx.demod_frames_mrc(d_iq, B, nf, fl, fl, scratch.addr) == nds
    assert same_bits(scratch.read(), p_eq.read())
    with pytest.raises(ValueError, match="needs d_eq"):
        rx.demod_frames_mrc(d_iq, B, nf, fl, fl, None, d_llr=scratch.addr)


# ------------------------------------------------------------------------------------------ 4. graph capture, argument errors
def test_graph_capture_equals_eager(om, torch):
    N, mod = 1024, "16QAM"
    cp, Kd = GEOM[N]
    rng = np.random.default_rng(12)
    B, nf = 2, 3
    iq = make_frames(N, mod, B * nf, 8, rng)
    n, fl = iq.shape
    rx = om.RxEngine(8, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    rx.set_max_trials(0)
    nds = rx.data_symbols_per_frame(fl)
    rx.reserve(n)
    rx.reserve_mrc(B, nf - 1, nds, Kd)                       # one frame per branch short of the batch that is captured second
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                llr=torch.zeros(nf * nds * Kd * 4, dtype=torch.float32, device="cuda"),
                sym=torch.zeros(nf * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                weight=torch.zeros(nf * nds * Kd, dtype=torch.float32, device="cuda"),
                sigma2=torch.zeros(n, dtype=torch.float64, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(stream, frames, nv):
        return rx.demod_frames_mrc(d_iq, B, frames, fl, fl, outs["eq"], nv, outs["llr"], outs["sym"], outs["weight"], outs["sigma2"],
                                   stream=stream)

    for nv in (None, [0.02, 0.05]):
        with torch.cuda.stream(s):
            call(s.cuda_stream, nf - 1, nv)
        s.synchronize()
        eager = {k: v.clone() for k, v in outs.items()}
        assert bool((eager["sigma2"][:B * (nf - 1)] > 0).all()) and bool((eager["weight"][:(nf - 1) * nds * Kd] > 0).all())
        for v in outs.values():
            v.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(torch.cuda.current_stream().cuda_stream, nf - 1, nv)
            with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc"):
                call(torch.cuda.current_stream().cuda_stream, nf, nv)   # a larger batch: the workspace would have to grow
        assert not outs["sigma2"].any()                      # capture enqueues nothing
        g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], eager[k]), (k, nv)
        for v in outs.values():
            v.zero_()


def test_argument_errors_leave_the_outputs_untouched(om, torch, rx0):
    d = torch.zeros(256, dtype=torch.float32, device="cuda")
    s2 = torch.zeros(16, dtype=torch.float64, device="cuda")
    o, u, w = Out(torch, 64, torch.float32), Out(torch, 64, torch.float32), Out(torch, 64, torch.float32)
    ok = dict(n_branch=2, n_seg=2, rows=3, row_len=4, seg_stride=12, csi_stride=4, rho=RHO, modulation="QPSK", noise_var=[0.1, 0.2],
              d_sigma2=None)
    for kw in (dict(n_seg=-1), dict(rows=-1), dict(n_branch=0, noise_var=[]), dict(n_branch=9, noise_var=[0.1] * 9), dict(seg_stride=11),
               dict(csi_stride=3), dict(modulation="BPSK"), dict(modulation=3), dict(noise_var=[0.1, 0.0]), dict(noise_var=[-1.0, 0.1]),
               dict(noise_var=[0.1, float("nan")]), dict(noise_var=[float("inf"), 0.1]), dict(rho=-1.0), dict(rho=float("inf")),
               dict(n_seg=1 << 32), dict(n_seg=1 << 19, seg_stride=1 << 30)):
        a = dict(ok, **kw)
        with pytest.raises(ValueError, match="ofdm_combine_csi_frames"):
            rx0.combine_csi_frames(d, a["n_branch"], a["n_seg"], a["rows"], a["row_len"], a["seg_stride"], d, a["csi_stride"], a["rho"],
                                   a["modulation"], a["noise_var"], a["d_sigma2"], o.addr, u.addr, w.addr, stream=cur(torch))
    with pytest.raises(ValueError):
        rx0.combine_csi_frames(None, 2, 2, 3, 4, 12, d, 4, RHO, "QPSK", [0.1, 0.2], d_llr=o.addr)
    with pytest.raises(ValueError, match="exactly one"):
        rx0.combine_csi_frames(d, 2, 2, 3, 4, 12, d, 4, RHO, "QPSK", [0.1, 0.2], s2, d_llr=o.addr)
    with pytest.raises(ValueError):
        rx0.reserve_mrc(2, -1, 1, 1)
    bp = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100, modulation="BPSK")
    with pytest.raises(ValueError, match="ofdm_rx_demod_frames_mrc"):
        bp.demod_frames_mrc(d, 2, 1, 32, 32, d, [0.1, 0.2], d_llr=o.addr)
    with pytest.raises(ValueError, match="ofdm_rx_demod_frames_mrc"):
        rx0.demod_frames_mrc(d, 2, 1, 32, 32, d, [0.1, -0.2], d_llr=o.addr)
    torch.cuda.synchronize()
    assert o.untouched() and u.untouched() and w.untouched()


# ------------------------------------------------------------------------------------------ 5. the link, end to end on the device
def test_chain_decodes_where_one_branch_does_not(om, torch):
    """mrc_cases end to end: turbo_encode_frames -> modulate_frames -> channel (taps and noise seed per branch, into one IQ buffer
    of 2 * 64 frames) -> demod_frames_mrc -> turbo_decode_frames gives every block back, with the noise estimated and with it
    given; branch 0 alone through demod_frames_csi loses at least 8 (15 on the oracle's receiver with the same noise samples)."""
    n, L, B = mc.N_FRAMES, mc.N + mc.CP, mc.N_BRANCH
    txe = om.TxEngine(mc.N, mc.CP, mc.KS, mc.KD, (1, 3), mc.MOD)
    rxe = om.RxEngine(mc.N_SYM, mc.N, mc.CP, mc.KS, (1, 3), mc.KD, mc.SNR_ARG, mc.GATE, modulation=mc.MOD)
    rxe.set_max_trials(0)
    info = mc.info_bits()
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * mc.SEG_BITS)
    txe.turbo_encode_frames(d_info, n, 1, mc.K, mc.F1, mc.F2, d_coded, mc.SEG_BITS)
    fl_tx, fl = mc.N_SYM * L, mc.FRAME_LEN
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(B * n * fl * 8)
    txe.modulate_frames(d_coded, n, mc.N_SYM, d_tx)
    for b in range(B):
        taps = np.asarray(mc.TAPS[b]).astype(np.complex64)
        d_taps = om.DeviceBuffer(taps.nbytes).upload(taps)
        txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx.data_ptr() + b * n * fl * 8, fl, fl, noise_var=mc.NOISE_VAR,
                    seed=mc.SEED_NOISE + b)
    assert rxe.data_symbols_per_frame(fl) == mc.N_DSYM
    d_eq = om.DeviceBuffer(B * n * mc.N_DSYM * mc.KD * 8)
    d_llr = om.DeviceBuffer(n * mc.SEG_BITS * 4)
    d_tsr = om.DeviceBuffer(B * n * 16)
    d_bits = om.DeviceBuffer(n * mc.K)

    def lost_blocks():
        rxe.turbo_decode_frames(d_llr, n, mc.SEG_BITS, 1, mc.K, mc.F1, mc.F2, mc.N_ITER, d_bits=d_bits)
        return int((d_bits.download(np.uint8, n * mc.K).reshape(n, 1, mc.K) != info).any(axis=(1, 2)).sum())

    lost = {}
    for name, nv in (("estimated", None), ("given", [mc.NOISE_VAR] * B)):
        assert rxe.demod_frames_mrc(d_rx, B, n, fl, fl, d_eq, nv, d_llr, d_tsr=d_tsr) == mc.N_DSYM
        print("frames with a sync: %d of %d" % ((d_tsr.download(np.int32, B * n * 4).reshape(B * n, 4)[:, 3] != 0).sum(), B * n))
        lost[name] = lost_blocks()
    assert rxe.demod_frames_csi(d_rx, n, fl, fl, d_eq, d_llr) == mc.N_DSYM
    lost["branch 0 alone"] = lost_blocks()
    print("wrong blocks of %d: %r" % (n, lost))
    assert lost["estimated"] == 0 and lost["given"] == 0
    assert lost["branch 0 alone"] >= 8
