"""Channel-estimate averaging over the sync symbols of a frame on the GPU (-m gpu): ofdm_chan_average_frames,
ofdm_rx_set_chan_average, ofdm_rx_reserve_chan_average and ofdm_rx_chan_spread_frames against tests/chanavg_ref.py (the contract of
include/ofdm_mi355x.h in fp64 NumPy, pinned by test_chanavg_ref_host.py).  The stand-alone call visits every FFT plan with a partly
filled last workgroup, chunk remainders, erasures and every output alone; the composite path is compared averaging on against
averaging off on frames of the device transmitter and channel; the link case runs end to end on the device.
Bars (each printed before it is asserted):
  Hbar    max|a - b| / max|b| < 1e-5 per call, the library's bar for FFT outputs
  gain    the same bar against the gain expression in fp64 on the DEVICE's Hbar
  rot     |u_dev - u_ref| < 1e-5, the zero entries agreeing exactly;  n_used exact
  spread  |sqrt(s_dev) - sqrt(s_ref)| <= 4e-5 max|a_ref|: what 1e-5 on each a_p and on u_p allows through the triangle
          inequality on the root-mean-square deviation"""
import numpy as np
import pytest

import chanavg_cases as ac
import chanavg_ref
import csi_cases as cc
import csi_ref
from test_gpu_chanwin import _link, _lost, demod_all, device_frames, receiver, relerr, run_standalone, upload
from test_gpu_csi import GUARD, Out, cur, same_bits
from test_gpu_soft_frames import GEOM

pytestmark = pytest.mark.gpu

TOL = 1e-5
SNR_LS = ac.snr_lin()
RHO = float(np.float32(1.0 / SNR_LS))
ALL = ("H", "gain", "spread", "n_used", "rot")


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


def engine(om, N, Ks, Kd, synch_dat=ac.SYNCH_DAT):
    return om.RxEngine(8, N, ac.CP[N], Ks, synch_dat, Kd, ac.SNR_ARG, 0.7)


def run_avg(torch, rx, d_iq, n, stride, frame_len, tsr, n_avg, N, Kd, P, want=ALL):
    """chan_average_frames -> dict of host arrays (None for an output not wanted); every output sits between poisoned guard bands
    and starts as poison"""
    d_tsr = upload(torch, np.ascontiguousarray(tsr, np.int32))
    o = dict(H=Out(torch, n * N * 2, torch.float32), gain=Out(torch, n * Kd * 2, torch.float32), spread=Out(torch, n, torch.float32),
             n_used=Out(torch, n, torch.int32), rot=Out(torch, n * P * 2, torch.float32))
    a = {k: (o[k].addr if k in want else None) for k in ALL}
    rx.chan_average_frames(d_iq, n, stride, frame_len, d_tsr, n_avg, a["H"], a["gain"], a["spread"], a["n_used"], a["rot"],
                           stream=cur(torch))
    torch.cuda.synchronize()
    for k in ALL:
        if k not in want:
            assert o[k].untouched(), k
    r = {k: (o[k].read().copy() if k in want else None) for k in ALL}
    for k, shape in (("H", (n, N)), ("gain", (n, Kd)), ("rot", (n, P))):
        if r[k] is not None:
            r[k] = r[k].view(np.complex64).reshape(shape)
    return r


def check_against_reference(got, ref, tsr, N, Ks, Kd, what):
    """the bars of the module's docstring over one call; returns the measured errors"""
    n = len(ref)
    live = [f for f in range(n) if ref[f]["on"]]
    dead = [f for f in range(n) if not ref[f]["on"]]
    assert live, what
    ref_H = np.stack([ref[f]["H"] for f in live])
    a_max = max(float(np.max(np.abs(ap))) for f in live for ap in ref[f]["a"] if ap is not None)
    e_H = relerr(got["H"][live], ref_H)
    want_g = np.stack([chanavg_ref.gain_of(got["H"][f], int(tsr[f][1]), Kd, RHO) for f in live])
    e_g = relerr(got["gain"][live], want_g)
    ref_rot = np.stack([ref[f]["rot"] for f in range(n)])
    e_u = float(np.max(np.abs(got["rot"].astype(np.complex128) - ref_rot)))
    e_s = float(np.max(np.abs(np.sqrt(got["spread"].astype(np.float64)) - np.sqrt([ref[f]["spread"] for f in range(n)]))))
    coh = min(float(c) for f in live for c, ap in zip(ref[f]["coh"], ref[f]["a"]) if ap is not None)
    print("%r: relerr Hbar %.2e gain %.2e, |du| %.2e, |d sqrt(spread)| %.2e (bar %.2e), coherence >= %.2f"
          % (what, e_H, e_g, e_u, e_s, 4e-5 * a_max, coh))
    assert coh > 0.5, what
    assert e_H < TOL and e_g < TOL and e_u < TOL and e_s <= 4e-5 * a_max, what
    assert np.array_equal(got["rot"] == 0, ref_rot == 0), what
    assert list(got["n_used"]) == [ref[f]["n_used"] for f in range(n)], what
    assert not np.signbit(got["spread"]).any() and np.isfinite(got["spread"]).all(), what
    off = np.setdiff1d(np.arange(N), chanavg_ref.bins_p(Ks, N))
    assert not np.ascontiguousarray(got["H"][live][:, off]).view(np.uint32).any(), what
    for f in dead:                                           # no store to Hbar or gain; spread +0, n_used 0, rot all +0
        assert np.isnan(got["H"][f].view(np.float32)).all() and np.isnan(got["gain"][f].view(np.float32)).all(), what
        assert not got["spread"][f:f + 1].view(np.uint32).any() and got["n_used"][f] == 0, what
        assert not got["rot"][f].view(np.uint32).any(), what
    return live


def bits_equal(a, b, live):
    for k in ALL:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if k in ("H", "gain"):
            x, y = x[live], y[live]
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


# ------------------------------------------------------------------------------------------ 1. the stand-alone call
@pytest.mark.parametrize("N,Ks,Kd,n_pat,n_avg", ac.standalone_cases())
def test_standalone_against_the_reference(om, torch, N, Ks, Kd, n_pat, n_avg):
    cp = ac.CP[N]
    rx = engine(om, N, Ks, Kd)
    b = ac.make_batch(N, Ks, Kd, n_pat, seed=N + n_pat + Ks)
    iq, tsr, stride, fl = b["iq"], b["tsr"], b["stride"], b["frame_len"]
    n = iq.shape[0]
    assert n == ac.slots(N) + 1 and stride % 2 == 1 and (tsr[:, 3] == 0).sum() == 1
    assert {int(t) % ac.LINE == 0 for t in b["t0"]} == {True, False}
    P = chanavg_ref.patterns(fl, N, cp, 1, 1, n_avg)
    assert P == (n_pat if n_avg < 0 else min(n_avg, n_pat))
    ref = chanavg_ref.average_frames(iq, fl, tsr, n_avg, N, cp, 1, 1, Ks, Kd, SNR_LS, RHO)
    d_iq = upload(torch, iq)
    got = run_avg(torch, rx, d_iq, n, stride, fl, tsr, n_avg, N, Kd, P)
    what = (N, Ks, n_pat, n_avg)
    live = check_against_reference(got, ref, tsr, N, Ks, Kd, what)
    if b["zeroed"] and b["zeroed"][1] < P:
        zf, zp = b["zeroed"]
        assert got["rot"][zf, zp] == 0 and got["n_used"][zf] == P - 1, what
    if P > 1:                                                # the planted rotation of every frame comes back in rot
        for f in live:
            p = b["p_rot"][f]
            if 0 < p < P and got["rot"][f, p] != 0:
                assert abs(got["rot"][f, p] - np.exp(1j * b["theta"][f])) < 0.5, (what, f)    # noise turns u_p a little
    # a second call, each output alone, a frame alone: the same bits
    bits_equal(run_avg(torch, rx, d_iq, n, stride, fl, tsr, n_avg, N, Kd, P), got, live)
    for k in ALL:
        one = run_avg(torch, rx, d_iq, n, stride, fl, tsr, n_avg, N, Kd, P, want=(k,))
        x, y = np.ascontiguousarray(one[k]), np.ascontiguousarray(got[k])
        if k in ("H", "gain"):
            x, y = x[live], y[live]
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)
    f = live[-1]
    alone = run_avg(torch, rx, d_iq[f:f + 1], 1, stride, fl, tsr[f:f + 1], n_avg, N, Kd, P)
    for k in ALL:
        assert np.array_equal(np.ascontiguousarray(alone[k][0:1]).view(np.uint8), np.ascontiguousarray(got[k][f:f + 1]).view(np.uint8)), (what, k)


@pytest.mark.parametrize("N", [64, 2048])
def test_last_window_cut_by_frame_len(om, torch, N):
    """frame_len one sample short of the last pattern's window: the pattern drops out; exactly at its end: it takes part"""
    cp, Ks, Kd, n_pat = ac.CP[N], N - 2, N - 4, 3
    L = N + cp
    rx = engine(om, N, Ks, Kd)
    b = ac.make_batch(N, Ks, Kd, n_pat, seed=5, late=True)
    iq, tsr, stride = b["iq"], b["tsr"], b["stride"]
    n = iq.shape[0]
    d_iq = upload(torch, iq)
    end0 = int(b["t0"][0]) + 2 * L * (n_pat - 1) + N         # the end of frame 0's last window
    full0 = n_pat - (1 if b["zeroed"] and b["zeroed"][0] == 0 else 0)       # frame 0 may hold the batch's zeroed sync symbol
    seen = set()
    for fl in (end0 - 1, end0, end0 + 1):
        assert chanavg_ref.patterns(fl, N, cp, 1, 1, -1) == n_pat
        ref = chanavg_ref.average_frames(iq, fl, tsr, -1, N, cp, 1, 1, Ks, Kd, SNR_LS, RHO)
        got = run_avg(torch, rx, d_iq, n, stride, fl, tsr, -1, N, Kd, n_pat)
        check_against_reference(got, ref, tsr, N, Ks, Kd, (N, "frame_len", fl - end0))
        seen.add(int(got["n_used"][0]))
        assert got["n_used"][0] == (full0 - 1 if fl < end0 else full0) and (got["rot"][0, n_pat - 1] == 0) == (fl < end0)
    assert seen == {full0 - 1, full0}


def test_hostile_tsr_is_a_row_without_a_sync(om, torch):
    """pattern 0 not inside the frame (a negative start, a start at the frame's end): no store, spread +0, n_used 0"""
    N, Ks, Kd, n_pat = 64, 62, 60, 4
    rx = engine(om, N, Ks, Kd)
    b = ac.make_batch(N, Ks, Kd, n_pat, seed=9)
    tsr = b["tsr"].copy()
    tsr[0, 0], tsr[1, 0], tsr[2, 0] = -1, b["frame_len"] - N + 1, -(1 << 31)
    ref = chanavg_ref.average_frames(b["iq"], b["frame_len"], tsr, -1, N, 16, 1, 1, Ks, Kd, SNR_LS, RHO)
    assert [r["on"] for r in ref[:3]] == [False] * 3
    got = run_avg(torch, rx, upload(torch, b["iq"]), len(tsr), b["stride"], b["frame_len"], tsr, -1, N, Kd, n_pat)
    check_against_reference(got, ref, tsr, N, Ks, Kd, "hostile tsr")


# ------------------------------------------------------------------------------------------ 2. the composite path
def standalone_on(torch, rx, d_rx, n, fl, tsr, n_avg, N, Kd):
    P = chanavg_ref.patterns(fl, N, GEOM[N][0], 1, 3, n_avg)
    return run_avg(torch, rx, d_rx, n, fl, fl, tsr, n_avg, N, Kd, P)


@pytest.mark.parametrize("N,mod", [(64, "16QAM"), (1024, "QPSK")])
def test_averaging_on_against_averaging_off(om, torch, N, mod):
    cp, Kd = GEOM[N]
    n, n_sym, dead = 5, 16, 2                                # four patterns per frame
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, dead, seed=N + 1)
    never, rx = receiver(om, N, mod, n_sym), receiver(om, N, mod, n_sym)
    off = demod_all(om, torch, never, d_rx, n, fl, N, mod)
    live = np.flatnonzero(off["tsr"][:, 3] == 1)
    assert list(off["tsr"][:, 3]) == [1, 1, 0, 1, 1], off["tsr"]
    s2 = Out(torch, n, torch.float64)
    with pytest.raises(ValueError, match="without averaging"):
        rx.chan_spread_frames(1, s2.addr)
    rx.set_chan_average(-1)
    on = demod_all(om, torch, rx, d_rx, n, fl, N, mod)
    assert np.array_equal(on["tsr"], off["tsr"])
    # frame_state = the stand-alone call on the same IQ and the call's tsr, bit for bit; the reference within the bars
    sa = standalone_on(torch, rx, d_rx, n, fl, off["tsr"], -1, N, Kd)
    assert same_bits(on["H"][live].view(np.float32), sa["H"][live].view(np.float32))
    assert same_bits(on["gain"][live].view(np.float32), sa["gain"][live].view(np.float32))
    assert list(sa["n_used"]) == [4, 4, 0, 4, 4]
    iq = d_rx.cpu().numpy().view(np.complex64).reshape(n, fl)
    ref = chanavg_ref.average_frames(iq, fl, off["tsr"], -1, N, cp, 1, 3, N - 2, Kd, SNR_LS, RHO)
    check_against_reference(sa, ref, off["tsr"], N, N - 2, Kd, (N, "composite"))
    assert same_bits(on["H"][dead].view(np.float32), off["H"][dead].view(np.float32))
    assert same_bits(on["gain"][dead].view(np.float32), off["gain"][dead].view(np.float32))
    assert relerr(on["H"][live], off["H"][live].astype(np.complex128)) > 100 * TOL, "the average changed nothing"
    # the equalised symbols: the same FFT outputs times the averaged gains
    g_off, g_on = off["gain"].astype(np.complex128), on["gain"].astype(np.complex128)
    for f in live:
        ok = np.abs(g_off[f]) > 1e-3 * np.max(np.abs(g_off[f]))
        assert ok.sum() > Kd // 2
        want = off["eq"][f].astype(np.complex128)[:, ok] * (g_on[f, ok] / g_off[f, ok])[None, :]
        e = relerr(on["eq"][f][:, ok], want)
        assert e < TOL, (f, e)
    assert not on["eq"][dead].any()
    bins = om.bins_p(Kd, N)
    for f in range(n):
        assert same_bits(on["csi"][f], csi_ref.csi_row(on["H"][f], bins)), f
    # chan_spread_frames: the stand-alone spread widened to double
    rx.chan_spread_frames(n, s2.addr, stream=cur(torch))
    got = s2.read().copy()
    assert np.array_equal(got.view(np.uint64), sa["spread"].astype(np.float64).view(np.uint64))
    assert got[dead] == 0.0 and not np.signbit(got[dead]) and (got[live] > 0).all()
    with pytest.raises(ValueError, match="last ofdm_rx_demod_frames call"):
        rx.chan_spread_frames(n + 1, s2.addr)
    # n_avg = 1: the receiver's own estimate within the bar, the same hard bits
    rx.set_chan_average(1)
    one = demod_all(om, torch, rx, d_rx, n, fl, N, mod)
    e1 = relerr(one["H"][live], off["H"][live].astype(np.complex128))
    print("N=%d: n_avg = 1 against averaging off: relerr H %.2e" % (N, e1))
    assert e1 < TOL and np.array_equal(one["bits"], off["bits"])
    rx.chan_spread_frames(n, s2.addr, stream=cur(torch))
    assert not s2.read().view(np.uint64).any()
    # averaging followed by the delay window = chan_window_frames on the stand-alone Hbar
    pre, post = cp // 4, 3 * cp // 4
    rx.set_chan_average(-1)
    rx.set_chan_window(pre, post)
    both = demod_all(om, torch, rx, d_rx, n, fl, N, mod)
    w_H, w_g, _ = run_standalone(torch, rx, sa["H"], off["tsr"], pre, post, Kd)
    assert same_bits(both["H"][live].view(np.float32), w_H[live].view(np.float32))
    assert same_bits(both["gain"][live].view(np.float32), w_g[live].view(np.float32))
    # switched off again: every output as of a handle that never had it on
    rx.set_chan_window(0, 0)
    rx.set_chan_average(0)
    back = demod_all(om, torch, rx, d_rx, n, fl, N, mod)
    for k in off:
        assert np.array_equal(np.ascontiguousarray(back[k]).view(np.uint8), np.ascontiguousarray(off[k]).view(np.uint8)), k
    with pytest.raises(ValueError, match="without averaging"):
        rx.chan_spread_frames(1, s2.addr)


def test_composites_follow_the_stage(om, torch):
    """demod_frames_csi with averaging on = demod_frames (averaging on), csi_frames and demap_csi_frames called one by one"""
    N, mod = 64, "16QAM"
    cp, Kd = GEOM[N]
    n, n_sym = 4, 12
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, 1, seed=8)
    rx, plain = receiver(om, N, mod, n_sym), receiver(om, N, mod, n_sym)
    rx.set_chan_average(-1)
    nds = rx.data_symbols_per_frame(fl)
    eq, a = Out(torch, n * nds * Kd * 2, torch.float32), Out(torch, n * Kd, torch.float32)
    llr, llr2, llr0 = (Out(torch, n * nds * Kd * 4, torch.float32) for _ in range(3))
    eq2, eq0 = Out(torch, n * nds * Kd * 2, torch.float32), Out(torch, n * nds * Kd * 2, torch.float32)
    assert rx.demod_frames(d_rx, n, fl, fl, eq.addr) == nds
    rx.csi_frames(n, a.addr)
    rx.demap_csi_frames(eq.addr, n, nds, Kd, nds * Kd, a.addr, Kd, rx.csi_rho, mod, llr.addr)
    assert rx.demod_frames_csi(d_rx, n, fl, fl, eq2.addr, llr2.addr) == nds
    assert same_bits(eq2.read(), eq.read()) and same_bits(llr2.read(), llr.read()) and llr.read().any()
    assert plain.demod_frames_csi(d_rx, n, fl, fl, eq0.addr, llr0.addr) == nds
    assert not same_bits(llr0.read(), llr.read())


def test_graph_capture_keeps_the_setting(om, torch):
    N, mod = 1024, "16QAM"
    cp, Kd = GEOM[N]
    n, n_sym = 4, 12
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, 3, seed=13)
    rx = receiver(om, N, mod, n_sym)
    rx.reserve(n)
    rx.reserve_chan_average(n, fl)
    rx.set_chan_average(2)
    nds = rx.data_symbols_per_frame(fl)
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                tsr=torch.zeros(n * 4, dtype=torch.int32, device="cuda"), s2=torch.zeros(n, dtype=torch.float64, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(stream):
        r = rx.demod_frames(d_rx, n, fl, fl, outs["eq"], d_tsr=outs["tsr"], stream=stream)
        rx.chan_spread_frames(n, outs["s2"], stream=stream)
        return r

    with torch.cuda.stream(s):
        assert call(s.cuda_stream) == nds
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["s2"][:3] > 0).all()) and float(eager["s2"][3]) == 0.0 and bool(eager["eq"].any())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert not outs["s2"].any()                              # capture enqueues nothing
    rx.set_chan_average(0)                                   # the graph keeps the setting it was captured with
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k


def test_refusals_leave_the_outputs_untouched(om, torch):
    N, Ks, Kd = 64, 62, 60
    rx = engine(om, N, Ks, Kd)
    fl = 4 * 80
    d = torch.zeros(4 * fl * 2, dtype=torch.float32, device="cuda")
    t = torch.ones(16, dtype=torch.int32, device="cuda")
    o, g, sp = Out(torch, 4 * N * 2, torch.float32), Out(torch, 4 * Kd * 2, torch.float32), Out(torch, 4, torch.float32)
    base = dict(d_iq=d, n_frames=4, frame_stride=fl, frame_len=fl, d_tsr=t, n_avg=-1, d_H_out=o.addr, d_gain_out=g.addr, d_spread=sp.addr)
    for kw in (dict(n_avg=0), dict(n_avg=-2), dict(n_frames=-1), dict(frame_len=-1, frame_stride=-1), dict(n_frames=1 << 31),
               dict(frame_stride=fl - 1), dict(d_iq=None), dict(d_tsr=None), dict(d_H_out=None, d_gain_out=None, d_spread=None)):
        with pytest.raises(ValueError, match="ofdm_chan_average_frames"):
            rx.chan_average_frames(**dict(base, **kw), stream=cur(torch))
    rx.chan_average_frames(None, 0, fl, fl, None, -1)        # no frames: a no-op
    with pytest.raises(ValueError, match="ofdm_rx_set_chan_average"):
        rx.set_chan_average(-2)
    with pytest.raises(ValueError, match="ofdm_rx_reserve_chan_average"):
        rx.reserve_chan_average(-1, fl)
    with pytest.raises(ValueError, match="ofdm_rx_chan_spread_frames"):
        rx.chan_spread_frames(-1, sp.addr)
    two = engine(om, N, Ks, Kd, synch_dat=(2, 3))            # synch_S != 1
    with pytest.raises(ValueError, match="synch_S"):
        two.set_chan_average(1)
    with pytest.raises(ValueError, match="synch_S"):
        two.chan_average_frames(**base, stream=cur(torch))
    with pytest.raises(ValueError, match="synch_S"):
        two.reserve_chan_average(4, fl)
    two.set_chan_average(0)                                  # off is always accepted
    lib = om.load()
    assert lib.ofdm_chan_average_frames(None, d.data_ptr(), 4, fl, fl, t.data_ptr(), -1, o.addr, None, None, None, None, None) == -1
    assert b"null handle" in lib.ofdm_last_error()
    torch.cuda.synchronize()
    assert o.untouched() and g.untouched() and sp.untouched()


# ------------------------------------------------------------------------------------------ 3. the link, end to end on the device
def test_link_end_to_end(om, torch):
    """csi_cases: at 0.175 and 0.2203 demod_frames_csi with averaging on gives every block back where averaging off loses the 15
    and 58 of 64 the oracle's receiver loses on the same noise samples; at 0.30 the average followed by the window (4, 12) loses
    at most 12"""
    n = cc.N_FRAMES
    lost = {}
    for nv in ac.LEVELS + (ac.LEVEL_HIGH,):
        rxe, d_rx, fl, info = _link(om, cc, [cc.TAPS], nv)
        d_eq, d_llr, d_bits = om.DeviceBuffer(n * cc.N_DSYM * cc.KD * 8), om.DeviceBuffer(n * cc.SEG_BITS * 4), om.DeviceBuffer(n * cc.K)
        if nv != ac.LEVEL_HIGH:
            assert rxe.demod_frames_csi(d_rx, n, fl, fl, d_eq, d_llr) == cc.N_DSYM
            lost[(nv, "ls")] = _lost(rxe, om, d_llr, d_bits, cc, info)
        else:
            rxe.set_chan_window(*ac.LINK_WINDOW)
        rxe.set_chan_average(-1)
        assert rxe.demod_frames_csi(d_rx, n, fl, fl, d_eq, d_llr) == cc.N_DSYM
        lost[(nv, "averaged")] = _lost(rxe, om, d_llr, d_bits, cc, info)
        d_s2 = om.DeviceBuffer(n * 8)
        rxe.chan_spread_frames(n, d_s2)
        print("noise %.4f: %r; mean spread %.4f" % (nv, {k[1]: v for k, v in lost.items() if k[0] == nv}, d_s2.download(np.float64, n).mean()))
    assert [lost[(nv, "ls")] for nv in ac.LEVELS] == [15, 58], lost
    assert [lost[(nv, "averaged")] for nv in ac.LEVELS] == [0, 0], lost
    assert lost[(ac.LEVEL_HIGH, "averaged")] <= ac.PAIR_MAX_LOST, lost
