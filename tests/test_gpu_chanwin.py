"""Delay-window channel-estimate denoising on the GPU (-m gpu): ofdm_chan_window_frames, ofdm_rx_set_chan_window and
ofdm_rx_chan_noise_frames against tests/chanwin_ref.py (the contract of include/ofdm_mi355x.h in fp64 NumPy, pinned by
test_chanwin_ref_host.py).  The bar is the one of every FFT-based output of the library: max|a - b| / max|b| < TOL per call.  The
stand-alone call visits every FFT plan with a partly filled last workgroup; the composite path is compared window on against
window off on frames of the device transmitter and channel; the two link cases run end to end on the device."""
import numpy as np
import pytest

import chanwin_cases as wc
import chanwin_ref
import csi_cases as cc
import csi_ref
import mrc_cases as mc
from test_gpu_csi import GUARD, Out, cur, same_bits
from test_gpu_soft_frames import GEOM

pytestmark = pytest.mark.gpu

TOL = 1e-5                                   # TOL of test_gpu_batch.py, conftest.TOL_MAX
SNR = 30.0
RHO = float(np.float32(1.0 / 10.0 ** (SNR / 20.0)))
TAPS = np.array([0.5, 0.0, 0.0, 1.0]) / np.linalg.norm([0.5, 0.0, 0.0, 1.0])


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


def relerr(got, want, floor=0.0):
    """max|got - want| / max|want|.  Where `want` is all zero the error is compared against `floor` = TOL * the scale of the call's
    input instead (floor / TOL takes the place of max|want|).  "All zero" is: nothing in it reaches `floor`.  The reference works on
    the float32-rounded input rows, so where the contract gives exactly zero (a planted tap outside the window) it holds the
    rounding of the input, some 1e-7 of its scale, and never a true zero."""
    scale = float(np.max(np.abs(want)))
    if scale <= floor:
        scale = floor / TOL
    return float(np.max(np.abs(np.asarray(got, np.complex128) - want))) / scale


def engine(om, N, Ks, Kd, cp):
    return om.RxEngine(8, N, cp, Ks, (1, 3), Kd, SNR, 0.7)


def upload(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32) if a.dtype == np.complex64 else a).cuda()


def run_standalone(torch, rx, H, tsr, pre, post, Kd, in_place=False, want=("gain", "tail")):
    """chan_window_frames on host arrays -> (H' [n][N] complex64, gain [n][Kd] complex64 or None, tail [n] float32 or None);
    every output sits between poisoned guard bands and starts as poison"""
    n, N = H.shape
    d_tsr = upload(torch, tsr)
    o_H = Out(torch, n * N * 2, torch.float32)
    o_g = Out(torch, n * Kd * 2, torch.float32) if "gain" in want else None
    o_t = Out(torch, n, torch.float32) if "tail" in want else None
    if in_place:
        o_H.t[GUARD:GUARD + n * N * 2] = upload(torch, H).ravel()
        torch.cuda.synchronize()
        src = o_H.addr
    else:
        d_H = upload(torch, H)
        src = d_H.data_ptr()
    rx.chan_window_frames(src, d_tsr, n, pre, post, o_H.addr, o_g.addr if o_g else None, o_t.addr if o_t else None, stream=cur(torch))
    torch.cuda.synchronize()
    return (o_H.read().copy().view(np.complex64).reshape(n, N), o_g.read().copy().view(np.complex64).reshape(n, Kd) if o_g else None,
            o_t.read().copy() if o_t else None)


# ------------------------------------------------------------------------------------------ 1. the stand-alone call
@pytest.mark.parametrize("N", wc.NFFTS)
def test_standalone_against_the_reference(om, torch, N):
    cp = wc.CP[N]
    for Ks in wc.sync_bin_counts(N):
        Kd = Ks - 2 if Ks < N else N
        rx = engine(om, N, Ks, Kd, cp)
        for pre, post in wc.windows(N):
            for seed in range(3):
                H, tsr = wc.standalone_rows(N, Ks, pre, post, seed)
                n = H.shape[0]
                assert n == wc.slots(N) + 1 and (tsr[:, 3] == 0).sum() == 1
                dead = int(np.flatnonzero(tsr[:, 3] == 0)[0])
                live = np.flatnonzero(tsr[:, 3] == 1)
                ref_H, ref_g, ref_t = chanwin_ref.window_rows(H, tsr, pre, post, Ks, Kd, RHO)
                got_H, got_g, got_t = run_standalone(torch, rx, H, tsr, pre, post, Kd)
                what = (N, Ks, pre, post, seed)
                floor = TOL * float(np.max(np.abs(H)))
                e_H = relerr(got_H[live], ref_H[live], floor)
                e_g = relerr(got_g[live], ref_g[live], floor / RHO)
                e_t = relerr(got_t[live], ref_t[live], floor * float(np.max(np.abs(H))))
                print("N=%d Ks=%d window=(%d,%d) seed=%d: relerr H' %.2e gain %.2e tail %.2e" % (what + (e_H, e_g, e_t)))
                assert e_H < TOL and e_g < TOL and e_t < TOL, what
                # the row without a sync: no store to H' or gain, tail +0; H' is +0 outside the sync bins
                assert np.isnan(got_H[dead].view(np.float32)).all() and np.isnan(got_g[dead].view(np.float32)).all(), what
                assert got_t[dead] == 0.0 and not np.signbit(got_t[dead]), what
                off = np.setdiff1d(np.arange(N), chanwin_ref.bins_p(Ks, N))
                assert not np.ascontiguousarray(got_H[live][:, off]).view(np.uint32).any(), what
                if pre + post == N:
                    assert not got_t.view(np.uint32).any(), what
                # in place, each output alone and a second call: the same bits
                again = run_standalone(torch, rx, H, tsr, pre, post, Kd)
                inpl = run_standalone(torch, rx, H, tsr, pre, post, Kd, in_place=True)
                alone = run_standalone(torch, rx, H, tsr, pre, post, Kd, want=())
                for other in (again, inpl):
                    assert same_bits(other[0][live].view(np.float32), got_H[live].view(np.float32)), what
                    assert same_bits(other[1][live].view(np.float32), got_g[live].view(np.float32)), what
                    assert same_bits(other[2], got_t), what
                assert same_bits(alone[0][live].view(np.float32), got_H[live].view(np.float32)), what
                assert same_bits(inpl[0][dead].view(np.float32), H[dead].view(np.float32)), what      # in place: the row as it was


def test_planted_taps_on_the_device(om, torch):
    """every planted delay of the contract at 64-pt and 2048-pt: H' = H_in on the sync bins or 0, tail = 0 or N/M |tap|^2"""
    amp = complex(0.8, -0.5)
    for N in (64, 2048):
        cp, Ks = wc.CP[N], N - 2
        Kd = Ks - 2
        rx = engine(om, N, Ks, Kd, cp)
        sb = chanwin_ref.bins_p(Ks, N)
        for pre, post in [(cp // 4, 3 * cp // 4), (0, 1), (0, 5)]:
            taps = wc.planted_taps(N, pre, post)
            H = np.stack([wc.planted_row(N, n0, amp) for n0, _ in taps]).astype(np.complex64)
            tsr = np.array([[0, wc.LAGS[i % 3], 0, 1] for i in range(len(taps))], np.int32)
            got_H, _, got_t = run_standalone(torch, rx, H, tsr, pre, post, Kd)
            M = N - pre - post
            for i, (n0, kept) in enumerate(taps):
                want = np.zeros(N, complex)
                if kept:
                    want[sb] = H[i][sb]
                assert np.max(np.abs(got_H[i] - want)) < TOL * abs(amp), (N, pre, post, n0)
                want_t = 0.0 if kept else N / M * abs(amp) ** 2
                assert abs(got_t[i] - want_t) < TOL * N / M * abs(amp) ** 2, (N, pre, post, n0)


# ------------------------------------------------------------------------------------------ 2. the composite path
def device_frames(om, torch, N, mod, n, n_sym, no_sync, seed):
    """frames of the device transmitter through the device channel (taps [0.5, 0, 0, 1] normalised, a little noise); frame
    `no_sync` is noise only -> (d_rx tensor [n][fl] complex64 as float32, fl)"""
    cp, Kd = GEOM[N]
    L = N + cp
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    bits = np.random.default_rng(seed).integers(0, 2, (n, txe.bits_per_frame(n_sym))).astype(np.uint8)
    d_bits = upload(torch, bits)
    fl_tx, fl = n_sym * L, n_sym * L + len(TAPS) - 1
    d_tx = torch.zeros(n, fl_tx * 2, dtype=torch.float32, device="cuda")
    d_rx = torch.zeros(n, fl * 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    txe.modulate_frames(d_bits, n, n_sym, d_tx, stream=cur(torch))
    torch.cuda.synchronize()                                 # torch's default stream is the library's NULL: the handle's own stream
    d_tx[no_sync].zero_()
    torch.cuda.synchronize()
    d_taps = upload(torch, TAPS.astype(np.complex64))
    txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(TAPS), d_rx, fl, fl, noise_var=0.01, seed=seed, stream=cur(torch))
    torch.cuda.synchronize()
    return d_rx, fl


def receiver(om, N, mod, n_sym):
    cp, Kd = GEOM[N]
    rx = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, SNR, 0.7, modulation=mod)
    rx.set_max_trials(0)
    return rx


def demod_all(om, torch, rx, d_rx, n, fl, N, mod):
    """demod_frames + frame_state + csi_frames -> dict of host arrays"""
    cp, Kd = GEOM[N]
    bps = csi_ref.BPS[mod]
    nds = rx.data_symbols_per_frame(fl)
    eq, bits = Out(torch, n * nds * Kd * 2, torch.float32), Out(torch, n * nds * Kd * bps, torch.uint8)
    tsr, a = Out(torch, n * 4, torch.int32), Out(torch, n * Kd, torch.float32)
    assert rx.demod_frames(d_rx, n, fl, fl, eq.addr, bits.addr, om.BITS_UNPACKED, tsr.addr) == nds
    rx.csi_frames(n, a.addr)
    st = [rx.frame_state(f) for f in range(n)]
    return dict(eq=eq.read().copy().view(np.complex64).reshape(n, nds, Kd), bits=bits.read().copy(), tsr=tsr.read().copy().reshape(n, 4),
                csi=a.read().copy().reshape(n, Kd), H=np.stack([s["chan_freq"] for s in st]), gain=np.stack([s["gain"] for s in st]))


@pytest.mark.parametrize("N,mod", [(64, "16QAM"), (1024, "QPSK")])
def test_window_on_against_window_off(om, torch, N, mod):
    cp, Kd = GEOM[N]
    n, n_sym, dead = 5, 8, 2
    pre, post = cp // 4, 3 * cp // 4
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, dead, seed=N)
    never, rx = receiver(om, N, mod, n_sym), receiver(om, N, mod, n_sym)
    off = demod_all(om, torch, never, d_rx, n, fl, N, mod)
    live = np.flatnonzero(off["tsr"][:, 3] == 1)
    assert list(off["tsr"][:, 3]) == [1, 1, 0, 1, 1] and (off["tsr"][live, 1] != 0).any(), off["tsr"]
    with pytest.raises(ValueError, match="without a window"):
        rx.chan_noise_frames(1, Out(torch, 1, torch.float64).addr)
    rx.set_chan_window(pre, post)
    on = demod_all(om, torch, rx, d_rx, n, fl, N, mod)
    assert np.array_equal(on["tsr"], off["tsr"])
    # frame_state against the reference applied to the off-call's estimate; the frame without a sync is as the sync kernel left it
    ref_H, ref_g, ref_t = chanwin_ref.window_rows(off["H"], off["tsr"], pre, post, N - 2, Kd, RHO, off["H"], off["gain"])
    e_H, e_g = relerr(on["H"][live], ref_H[live]), relerr(on["gain"][live], ref_g[live])
    print("N=%d: relerr H' %.2e gain %.2e" % (N, e_H, e_g))
    assert e_H < TOL and e_g < TOL
    assert same_bits(on["H"][dead].view(np.float32), off["H"][dead].view(np.float32))
    assert same_bits(on["gain"][dead].view(np.float32), off["gain"][dead].view(np.float32))
    assert relerr(on["H"][live], off["H"][live].astype(np.complex128)) > 100 * TOL, "the window changed nothing"
    # the equalised symbols: the same FFT outputs times the refined gains
    g_off, g_on = off["gain"].astype(np.complex128), on["gain"].astype(np.complex128)
    for f in live:
        ok = np.abs(g_off[f]) > 1e-3 * np.max(np.abs(g_off[f]))
        assert ok.sum() > Kd // 2
        want = off["eq"][f].astype(np.complex128)[:, ok] * (g_on[f, ok] / g_off[f, ok])[None, :]
        e = relerr(on["eq"][f][:, ok], want)
        assert e < TOL, (f, e)
    assert not on["eq"][dead].any()
    # csi_frames reads the refined estimate, by the header's own rule
    bins = om.bins_p(Kd, N)
    for f in range(n):
        assert same_bits(on["csi"][f], csi_ref.csi_row(on["H"][f], bins)), f
    # chan_noise_frames: the tail of the stand-alone call on the same rows, +0 for the frame without a sync
    sa_H, sa_g, sa_t = run_standalone(torch, rx, off["H"], off["tsr"], pre, post, Kd)
    s2 = Out(torch, n, torch.float64)
    rx.chan_noise_frames(n, s2.addr, stream=cur(torch))
    got = s2.read().copy()
    assert np.array_equal(got.view(np.uint64), sa_t.astype(np.float64).view(np.uint64))
    assert got[dead] == 0.0 and not np.signbit(got[dead]) and (got[live] > 0).all()
    assert relerr(got[live], ref_t[live]) < TOL
    assert same_bits(sa_H[live].view(np.float32), on["H"][live].view(np.float32))
    assert same_bits(sa_g[live].view(np.float32), on["gain"][live].view(np.float32))
    fewer = Out(torch, 2, torch.float64)
    rx.chan_noise_frames(2, fewer.addr)
    assert np.array_equal(fewer.read(), got[:2])
    with pytest.raises(ValueError, match="last ofdm_rx_demod_frames call"):
        rx.chan_noise_frames(n + 1, s2.addr)
    # switched off again: every output as of a handle that never had a window
    rx.set_chan_window(0, 0)
    back = demod_all(om, torch, rx, d_rx, n, fl, N, mod)
    for k in off:
        assert np.array_equal(np.ascontiguousarray(back[k]).view(np.uint8), np.ascontiguousarray(off[k]).view(np.uint8)), k
    with pytest.raises(ValueError, match="without a window"):
        rx.chan_noise_frames(1, s2.addr)


def test_composites_follow_the_window(om, torch):
    """demod_frames_csi with the window on = demod_frames (window on), csi_frames and demap_csi_frames called one by one"""
    N, mod = 64, "16QAM"
    cp, Kd = GEOM[N]
    n, n_sym = 4, 8
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, 1, seed=7)
    rx = receiver(om, N, mod, n_sym)
    rx.set_chan_window(4, 12)
    nds = rx.data_symbols_per_frame(fl)
    eq, a = Out(torch, n * nds * Kd * 2, torch.float32), Out(torch, n * Kd, torch.float32)
    llr, llr2 = Out(torch, n * nds * Kd * 4, torch.float32), Out(torch, n * nds * Kd * 4, torch.float32)
    eq2 = Out(torch, n * nds * Kd * 2, torch.float32)
    assert rx.demod_frames(d_rx, n, fl, fl, eq.addr) == nds
    rx.csi_frames(n, a.addr)
    rx.demap_csi_frames(eq.addr, n, nds, Kd, nds * Kd, a.addr, Kd, rx.csi_rho, mod, llr.addr)
    assert rx.demod_frames_csi(d_rx, n, fl, fl, eq2.addr, llr2.addr) == nds
    assert same_bits(eq2.read(), eq.read()) and same_bits(llr2.read(), llr.read()) and llr.read().any()


def test_graph_capture_equals_eager(om, torch):
    N, mod = 1024, "16QAM"
    cp, Kd = GEOM[N]
    n, n_sym = 4, 8
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, 3, seed=12)
    rx = receiver(om, N, mod, n_sym)
    rx.reserve(n)
    rx.set_chan_window(cp // 4, 3 * cp // 4)
    nds = rx.data_symbols_per_frame(fl)
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                tsr=torch.zeros(n * 4, dtype=torch.int32, device="cuda"), s2=torch.zeros(n, dtype=torch.float64, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(stream):
        r = rx.demod_frames(d_rx, n, fl, fl, outs["eq"], d_tsr=outs["tsr"], stream=stream)
        rx.chan_noise_frames(n, outs["s2"], stream=stream)
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
    rx.set_chan_window(0, 0)                                 # the graph keeps the window it was captured with
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k


def test_argument_errors_leave_the_outputs_untouched(om, torch):
    N, Kd = 64, 60
    rx = engine(om, N, 62, Kd, 16)
    d = torch.zeros(4 * N * 2, dtype=torch.float32, device="cuda")
    t = torch.ones(16, dtype=torch.int32, device="cuda")
    o, g, tl = Out(torch, 4 * N * 2, torch.float32), Out(torch, 4 * Kd * 2, torch.float32), Out(torch, 4, torch.float32)
    for pre, post in [(-1, 4), (0, 0), (4, 0), (4, -1), (60, 5), (0, 65), (1 << 31 - 1, 1)]:
        with pytest.raises(ValueError, match="ofdm_chan_window_frames"):
            rx.chan_window_frames(d, t, 4, pre, post, o.addr, g.addr, tl.addr, stream=cur(torch))
        if (pre, post) != (0, 0):
            with pytest.raises(ValueError, match="ofdm_rx_set_chan_window"):
                rx.set_chan_window(pre, post)
    for kw in (dict(n_rows=-1), dict(n_rows=1 << 31), dict(d_H_in=None), dict(d_tsr=None), dict(d_H_out=None)):
        a = dict(dict(d_H_in=d, d_tsr=t, n_rows=4, d_H_out=o.addr), **kw)
        with pytest.raises(ValueError, match="ofdm_chan_window_frames"):
            rx.chan_window_frames(a["d_H_in"], a["d_tsr"], a["n_rows"], 4, 12, a["d_H_out"], g.addr, tl.addr, stream=cur(torch))
    rx.chan_window_frames(None, None, 0, 4, 12, None)        # no rows: a no-op
    with pytest.raises(ValueError, match="ofdm_rx_chan_noise_frames"):
        rx.chan_noise_frames(-1, tl.addr)
    torch.cuda.synchronize()
    assert o.untouched() and g.untouched() and tl.untouched()


# ------------------------------------------------------------------------------------------ 3. the link, end to end on the device
def _lost(rxe, om, d_llr, d_bits, case, info):
    n = case.N_FRAMES
    rxe.turbo_decode_frames(d_llr, n, case.SEG_BITS, 1, case.K, case.F1, case.F2, case.N_ITER, d_bits=d_bits)
    return int((d_bits.download(np.uint8, n * case.K).reshape(n, 1, case.K) != info).any(axis=(1, 2)).sum())


def _link(om, case, taps_per_branch, noise_var):
    """turbo_encode_frames -> modulate_frames -> channel per branch (seed SEED_NOISE + b) -> (rxe, d_rx, fl, info)"""
    n, L, B = case.N_FRAMES, case.N + case.CP, len(taps_per_branch)
    txe = om.TxEngine(case.N, case.CP, case.KS, case.KD, (1, 3), case.MOD)
    rxe = om.RxEngine(case.N_SYM, case.N, case.CP, case.KS, (1, 3), case.KD, case.SNR_ARG, case.GATE, modulation=case.MOD)
    rxe.set_max_trials(0)
    info = case.info_bits()
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * case.SEG_BITS)
    txe.turbo_encode_frames(d_info, n, 1, case.K, case.F1, case.F2, d_coded, case.SEG_BITS)
    fl_tx, fl = case.N_SYM * L, case.FRAME_LEN
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(B * n * fl * 8)
    txe.modulate_frames(d_coded, n, case.N_SYM, d_tx)
    for b, tp in enumerate(taps_per_branch):
        taps = np.asarray(tp).astype(np.complex64)
        d_taps = om.DeviceBuffer(taps.nbytes).upload(taps)
        txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx.data_ptr() + b * n * fl * 8, fl, fl, noise_var=noise_var,
                    seed=case.SEED_NOISE + b)
    assert rxe.data_symbols_per_frame(fl) == case.N_DSYM
    return rxe, d_rx, fl, info


def test_link_one_branch(om, torch):
    """csi_cases at 0.175 and 0.2203: demod_frames_csi with the window (4, 12) gives every block back; without it the receiver
    loses the 15 of 64 at 0.175 that the oracle's receiver loses on the same noise samples"""
    n = cc.N_FRAMES
    lost = {}
    for nv in wc.CSI_LEVELS:
        rxe, d_rx, fl, info = _link(om, cc, [cc.TAPS], nv)
        d_eq, d_llr, d_bits = om.DeviceBuffer(n * cc.N_DSYM * cc.KD * 8), om.DeviceBuffer(n * cc.SEG_BITS * 4), om.DeviceBuffer(n * cc.K)
        d_used = om.DeviceBuffer(n * 8)
        assert rxe.demod_frames_csi(d_rx, n, fl, fl, d_eq, d_llr, d_n_used=d_used) == cc.N_DSYM
        assert (d_used.download(np.int64, n) == cc.N_DSYM * cc.KD).all(), "every frame should find its sync"
        lost[(nv, "ls")] = _lost(rxe, om, d_llr, d_bits, cc, info)
        rxe.set_chan_window(*wc.LINK_WINDOW)
        assert rxe.demod_frames_csi(d_rx, n, fl, fl, d_eq, d_llr) == cc.N_DSYM
        lost[(nv, "windowed")] = _lost(rxe, om, d_llr, d_bits, cc, info)
        d_s2 = om.DeviceBuffer(n * 8)
        rxe.chan_noise_frames(n, d_s2)
        tail = d_s2.download(np.float64, n)
        print("noise %.4f: LS loses %d of %d, windowed %d; mean tail %.4f" % (nv, lost[(nv, "ls")], n, lost[(nv, "windowed")], tail.mean()))
        if nv == wc.CSI_LEVELS[0]:
            assert wc.TAIL_MEAN_BOUNDS[0] <= tail.mean() <= wc.TAIL_MEAN_BOUNDS[1]
    for nv in wc.CSI_LEVELS:
        assert lost[(nv, "windowed")] == 0, lost
    assert lost[(wc.CSI_LEVELS[0], "ls")] == 15, lost


def test_link_two_branches(om, torch):
    """mrc_cases at 0.40: the combiner over the windowed estimates gives every block back, with the noise given and with the tail
    powers of chan_noise_frames as per-unit variances"""
    n, B, nv = mc.N_FRAMES, mc.N_BRANCH, wc.MRC_LEVEL
    rxe, d_rx, fl, info = _link(om, mc, mc.TAPS, nv)
    d_eq, d_llr = om.DeviceBuffer(B * n * mc.N_DSYM * mc.KD * 8), om.DeviceBuffer(n * mc.SEG_BITS * 4)
    d_bits, d_a, d_s2 = om.DeviceBuffer(n * mc.K), om.DeviceBuffer(B * n * mc.KD * 4), om.DeviceBuffer(B * n * 8)
    lost = {}
    assert rxe.demod_frames_mrc(d_rx, B, n, fl, fl, d_eq, [nv] * B, d_llr) == mc.N_DSYM
    lost["ls, given"] = _lost(rxe, om, d_llr, d_bits, mc, info)
    rxe.set_chan_window(*wc.LINK_WINDOW)
    assert rxe.demod_frames_mrc(d_rx, B, n, fl, fl, d_eq, [nv] * B, d_llr) == mc.N_DSYM
    lost["windowed, given"] = _lost(rxe, om, d_llr, d_bits, mc, info)
    # the sequence of INTEGRATION.md: demod_frames -> csi_frames, chan_noise_frames -> combine_csi_frames(OFDM_MRC_NOISE_SEG)
    assert rxe.demod_frames(d_rx, B * n, fl, fl, d_eq) == mc.N_DSYM
    rxe.csi_frames(B * n, d_a)
    rxe.chan_noise_frames(B * n, d_s2)
    rxe.combine_csi_frames(d_eq, B, n, mc.N_DSYM, mc.KD, mc.N_DSYM * mc.KD, d_a, mc.KD, rxe.csi_rho, mc.MOD, d_sigma2=d_s2, d_llr=d_llr)
    lost["windowed, tail"] = _lost(rxe, om, d_llr, d_bits, mc, info)
    print("noise %.2f, wrong blocks of %d: %r; mean tail %.4f" % (nv, n, lost, d_s2.download(np.float64, B * n).mean()))
    assert lost["windowed, given"] == 0 and lost["windowed, tail"] == 0
    assert lost["ls, given"] >= wc.LS_MIN_LOST
