"""The channel tracked across the sync symbols of a frame on the GPU (-m gpu): ofdm_chan_track_frames, ofdm_rx_demod_frames_track and
ofdm_rx_reserve_chan_track against tests/chantrack_ref.py (the contract of include/ofdm_mi355x.h in fp64 NumPy, pinned by
test_chantrack_ref_host.py).  The stand-alone call visits every FFT plan with a partly filled last workgroup, a full run of data
symbols and a remainder, both modes, the window on and off, erasures and every output alone; the composite call is compared with
the stand-alone one on the tsr it returns; the link case runs end to end on the device.
Bars (each printed before it is asserted):
  eq, H_pat   max|a - b| / max|b| < 1e-5 per output row, the library's bar for FFT outputs; rows the contract makes zero are +0 bits
  csi         max|a - b| / max(b) < 1e-5 per row
  takes       exact
  bits        exactly the oracle's hard decision of the device's own stored eq"""
import numpy as np
import pytest

import chantrack_cases as tc
import chantrack_ref as tr
import csi_ref
from oracle import ofdm_oracle as orc
from test_gpu_chanwin import device_frames, receiver, upload
from test_gpu_csi import Out, cur, same_bits
from test_gpu_soft_frames import GEOM

pytestmark = pytest.mark.gpu

TOL = 1e-5
SNR = tc.snr_lin()
RHO = float(np.float32(1.0 / SNR))
ALL = ("eq", "bits", "csi", "H", "takes")
BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}


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


def engine(om, N, Ks, Kd, synch_dat, mod="QPSK"):
    return om.RxEngine(8, N, tc.CP[N], Ks, synch_dat, Kd, tc.SNR_ARG, 0.7, modulation=mod)


def run_track(om, torch, rx, d_iq, n, stride, fl, tsr, mode, window=(0, 0), want=ALL, packed=False, composite=False):
    """chan_track_frames (or demod_frames_track: tsr is then ignored and the call's own comes back under "tsr") -> dict of host
    arrays (None for an output not wanted); every output sits between poisoned guard bands and starts as poison"""
    c = rx.cfg
    N, Kd, D, bps = c.nfft, c.num_data_bins, c.synch_D, c.modulation
    n_pat = (fl // (N + c.cp_len)) // (c.synch_S + D)
    nds = n_pat * D
    nbits = n * nds * Kd * bps
    o = dict(eq=Out(torch, n * nds * Kd * 2, torch.float32), bits=Out(torch, nbits // 8 if packed else nbits, torch.uint8),
             csi=Out(torch, n * nds * Kd, torch.float32), H=Out(torch, n * n_pat * N * 2, torch.float32),
             takes=Out(torch, n * n_pat, torch.int32))
    a = {k: (o[k].addr if k in want else None) for k in ALL}
    bm = om.BITS_NONE if "bits" not in want else om.BITS_PACKED if packed else om.BITS_UNPACKED
    if composite:
        o_tsr = Out(torch, n * 4, torch.int32)
        rx.set_chan_window(*window)
        ret = rx.demod_frames_track(d_iq, n, stride, fl, mode, a["eq"], a["bits"], bm, a["csi"], a["H"], a["takes"], o_tsr.addr,
                                    stream=cur(torch))
    else:
        d_tsr = upload(torch, np.ascontiguousarray(tsr, np.int32))
        ret = rx.chan_track_frames(d_iq, n, stride, fl, d_tsr, mode, window[0], window[1], a["eq"], a["bits"], bm, a["csi"], a["H"],
                                   a["takes"], stream=cur(torch))
    assert ret == nds
    torch.cuda.synchronize()
    for k in ALL:
        if k not in want:
            assert o[k].untouched(), k
    r = {k: (o[k].read().copy() if k in want else None) for k in ALL}
    if r["eq"] is not None:
        r["eq"] = r["eq"].view(np.complex64).reshape(n, nds, Kd)
    if r["csi"] is not None:
        r["csi"] = r["csi"].reshape(n, nds, Kd)
    if r["H"] is not None:
        r["H"] = r["H"].view(np.complex64).reshape(n, n_pat, N)
    if r["takes"] is not None:
        r["takes"] = r["takes"].reshape(n, n_pat)
    if composite:
        r["tsr"] = o_tsr.read().copy().reshape(n, 4)
    return r


def zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


def row_err(got, want, what):
    """max|got - want| / max|want| of one output row, held to the bar here: a NaN -- an element the device never wrote over its
    poison, or one it computed -- fails the comparison"""
    e = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
    assert e < TOL, (what, e)
    return e


def check_against_reference(got, ref, mod, what):
    """the bars of the module's docstring, asserted row by row over one call; returns the largest errors"""
    worst = dict(eq=0.0, H=0.0, csi=0.0)
    for k in ("eq", "H", "csi"):
        assert np.isfinite(got[k].view(np.float32)).all(), (what, k)
    for f, r in enumerate(ref):
        assert list(got["takes"][f]) == list(r["takes"]), (what, f)
        for p in range(len(r["takes"])):
            if r["takes"][p]:
                worst["H"] = max(worst["H"], row_err(got["H"][f, p], r["H_pat"][p], (what, "H_pat", f, p)))
            else:
                assert zero_bits(got["H"][f, p]), (what, f, p)
        for q in range(r["eq"].shape[0]):
            if r["eq"][q].any():
                worst["eq"] = max(worst["eq"], row_err(got["eq"][f, q], r["eq"][q], (what, "eq", f, q)))
            else:
                assert zero_bits(got["eq"][f, q]), (what, f, q)
            if r["on"]:
                worst["csi"] = max(worst["csi"], row_err(got["csi"][f, q], r["csi"][q], (what, "csi", f, q)))
            else:
                assert zero_bits(got["csi"][f, q]), (what, f, q)
    print("%r: relerr eq %.2e H_pat %.2e csi %.2e" % (what, worst["eq"], worst["H"], worst["csi"]))
    assert np.array_equal(got["bits"], orc.demap_hard(got["eq"].ravel(), mod)), what
    return worst


def same_outputs(a, b, keys=ALL):
    for k in keys:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


# ------------------------------------------------------------------------------------------ 1. the stand-alone call
@pytest.mark.parametrize("N,Ks,Kd,synch_dat,n_pat,n_frames", tc.standalone_cases())
def test_standalone_against_the_reference(om, torch, N, Ks, Kd, synch_dat, n_pat, n_frames):
    cp = tc.CP[N]
    S, D = synch_dat
    rx = engine(om, N, Ks, Kd, synch_dat)
    b = tc.make_batch(N, Ks, Kd, n_pat, seed=N + n_pat + Ks, synch_dat=synch_dat, n_frames=n_frames)
    iq, tsr, stride, fl = b["iq"], b["tsr"], b["stride"], b["frame_len"]
    n = iq.shape[0]
    assert n == (tc.slots(N) + 1 if n_frames is None else n_frames) and stride % 2 == 1 and (tsr[:, 3] == 0).sum() == 1
    with_sync = [f for f in range(n) if tsr[f, 3] == 1]
    if len(with_sync) >= 4:                                  # among the frames WITH a sync: t0 on and off a line, two lags, every erasure
        assert {int(b["t0"][f]) % tc.LINE == 0 for f in with_sync} == {True, False}
        assert len({int(tsr[f, 1]) for f in with_sync}) >= 2 and {k for k, _ in b["planted"].values()} == {"mid", "last", "first"}
    assert n_frames is None or len(with_sync) >= 4
    assert tr.patterns(fl, N, cp, S, D) == n_pat and n_pat * D > tc.RUN      # more than one run per frame
    assert "mid" in [k for k, _ in b["planted"].values()]
    d_iq = upload(torch, iq)
    got = {}
    for name, mode, window in (("linear", tr.LINEAR, (0, 0)), ("hold", tr.HOLD, (0, 0)), ("linear+window", tr.LINEAR, tc.WINDOW)):
        ref = tr.track_frames(iq, fl, tsr, mode, N, cp, S, D, Ks, Kd, SNR, RHO, window)
        got[name] = run_track(om, torch, rx, d_iq, n, stride, fl, tsr, mode, window)
        check_against_reference(got[name], ref, "QPSK", (N, Ks, Kd, synch_dat, n, name))
        for f, (kind, p) in b["planted"].items():
            assert got[name]["takes"][f, p] == 0 and (got[name]["takes"][f].sum() == 0) == (kind == "first"), (name, f, kind)
    assert not np.array_equal(got["linear"]["eq"], got["hold"]["eq"]) and not np.array_equal(got["linear"]["H"], got["linear+window"]["H"])
    same_outputs(got["linear"], got["hold"], ("H", "takes"))
    # a second call, each output alone, a frame alone: the same bits
    g = got["linear"]
    same_outputs(run_track(om, torch, rx, d_iq, n, stride, fl, tsr, tr.LINEAR), g)
    for k in ALL:
        same_outputs(run_track(om, torch, rx, d_iq, n, stride, fl, tsr, tr.LINEAR, want=(k,)), g, (k,))
    f = max(f for f in range(n) if tsr[f, 3] == 1 and f not in b["planted"]) if n > 4 else 0
    alone = run_track(om, torch, rx, d_iq[f:f + 1], 1, stride, fl, tsr[f:f + 1], tr.LINEAR)
    for k in ALL:
        per = g[k].size // n
        assert np.array_equal(np.ascontiguousarray(alone[k]).ravel().view(np.uint8),
                              np.ascontiguousarray(g[k]).ravel()[f * per:(f + 1) * per].view(np.uint8)), k


@pytest.mark.parametrize("N", [64, 2048])
def test_frame_len_cuts_the_last_windows(om, torch, N):
    """frame_len one sample short of, at and past the end of the last sync window (the pattern drops out of / takes part in the
    interpolation) and of the last pattern's guard (its rows are zeros / demodulated)"""
    cp, Ks, Kd, n_pat = tc.CP[N], N - 2, N - 4, 3
    L = N + cp
    rx = engine(om, N, Ks, Kd, (1, 1))
    b = tc.make_batch(N, Ks, Kd, n_pat, seed=5, late=True)
    iq, tsr, stride = b["iq"], b["tsr"], b["stride"]
    n = iq.shape[0]
    d_iq = upload(torch, iq)
    end_sync = int(b["t0"][0]) + 2 * L * (n_pat - 1) + N                     # the end of frame 0's last sync window
    guard = int(b["t0"][0]) + L * (2 * (n_pat - 1) + 1) + N - 1              # the smallest frame_len that demodulates its last pattern
    seen = set()
    for edge, name in ((end_sync, "sync"), (guard, "guard")):
        for fl in (edge - 1, edge, edge + 1):
            assert tr.patterns(fl, N, cp, 1, 1) == n_pat and fl <= stride
            ref = tr.track_frames(iq, fl, tsr, tr.LINEAR, N, cp, 1, 1, Ks, Kd, SNR, RHO)
            got = run_track(om, torch, rx, d_iq, n, stride, fl, tsr, tr.LINEAR)
            check_against_reference(got, ref, "QPSK", (N, name, fl - edge))
            state = (int(got["takes"][0, n_pat - 1]), bool(got["eq"][0, n_pat - 1].any()))
            seen.add(state)
            assert state == ((fl >= end_sync), (fl >= guard)), (name, fl - edge, state)
    assert seen == {(0, False), (1, False), (1, True)}


@pytest.mark.parametrize("mod", ["QPSK", "16QAM", "64QAM"])
def test_bits_of_every_modulation_in_both_formats(om, torch, mod):
    N, Ks, Kd, synch_dat, n_pat = 64, 62, 60, (1, 3), 8
    rx = engine(om, N, Ks, Kd, synch_dat, mod)
    b = tc.make_batch(N, Ks, Kd, n_pat, seed=BPS[mod], synch_dat=synch_dat, mod=mod)
    iq, tsr, stride, fl = b["iq"], b["tsr"], b["stride"], b["frame_len"]
    n = iq.shape[0]
    d_iq = upload(torch, iq)
    ref = tr.track_frames(iq, fl, tsr, tr.LINEAR, N, tc.CP[N], 1, 3, Ks, Kd, SNR, RHO)
    un = run_track(om, torch, rx, d_iq, n, stride, fl, tsr, tr.LINEAR)
    check_against_reference(un, ref, mod, (mod, "unpacked"))
    pk = run_track(om, torch, rx, d_iq, n, stride, fl, tsr, tr.LINEAR, packed=True)
    same_outputs(pk, un, ("eq", "csi", "H", "takes"))
    assert np.array_equal(pk["bits"], np.packbits(un["bits"]))
    alone = run_track(om, torch, rx, d_iq, n, stride, fl, tsr, tr.LINEAR, want=("bits",), packed=True)
    assert np.array_equal(alone["bits"], pk["bits"])
    # QPSK: the bits are the transmitted ones up to the few the noise costs (the dense constellations lose more at the channel's
    # spectral nulls and are held to the rule above only)
    f = [f for f in range(n) if ref[f]["on"] and f not in b["planted"]][0]
    per = n_pat * 3 * Kd * BPS[mod]
    wrong = np.count_nonzero(un["bits"][f * per:(f + 1) * per] != b["bits"][f])
    print("%s: %d of %d bits of frame %d wrong" % (mod, wrong, per, f))
    assert mod != "QPSK" or wrong < per // 10


# ------------------------------------------------------------------------------------------ 2. the composite call
@pytest.mark.parametrize("N,mod", [(64, "16QAM"), (1024, "QPSK")])
def test_composite_equals_the_standalone_call(om, torch, N, mod):
    cp, Kd = GEOM[N]
    n, n_sym, dead = 5, 16, 2                                # four patterns per frame
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, dead, seed=N + 3)
    never, rx = receiver(om, N, mod, n_sym), receiver(om, N, mod, n_sym)
    nds = rx.data_symbols_per_frame(fl)

    def plain(r):
        eq, tsr = Out(torch, n * nds * Kd * 2, torch.float32), Out(torch, n * 4, torch.int32)
        assert r.demod_frames(d_rx, n, fl, fl, eq.addr, d_tsr=tsr.addr, stream=cur(torch)) == nds
        st = [r.frame_state(f) for f in range(n)]
        return dict(eq=eq.read().copy(), tsr=tsr.read().copy().reshape(n, 4), H=np.stack([s["chan_freq"] for s in st]),
                    gain=np.stack([s["gain"] for s in st]))

    off = plain(never)
    assert list(off["tsr"][:, 3]) == [1, 1, 0, 1, 1], off["tsr"]
    iq = d_rx.cpu().numpy().view(np.complex64).reshape(n, fl)
    rx.set_chan_average(-1)                                  # not applied by the call
    for mode, window in ((tr.LINEAR, (0, 0)), (tr.HOLD, (0, 0)), (tr.LINEAR, (cp // 4, 3 * cp // 4))):
        comp = run_track(om, torch, rx, d_rx, n, fl, fl, None, mode, window, composite=True)
        assert np.array_equal(comp["tsr"], off["tsr"])
        sa = run_track(om, torch, rx, d_rx, n, fl, fl, comp["tsr"], mode, window)
        same_outputs(comp, sa)
        ref = tr.track_frames(iq, fl, comp["tsr"], mode, N, cp, 1, 3, N - 2, Kd, SNR, RHO, window)
        check_against_reference(comp, ref, mod, (N, "composite", mode, window))
        assert list(comp["takes"].sum(axis=1)) == [4, 4, 0, 4, 4]
        if window == (0, 0):                                 # the handle's per-frame state is the sync launch's: pattern 0's row
            live = np.flatnonzero(off["tsr"][:, 3] == 1)
            st = np.stack([rx.frame_state(int(f))["chan_freq"] for f in live])
            assert same_bits(st.view(np.float32), off["H"][live].view(np.float32))
            e = float(np.max(np.abs(comp["H"][live, 0] - off["H"][live]))) / float(np.max(np.abs(off["H"][live])))
            print("N=%d: H_pat[0] against the sync launch's row: relerr %.2e" % (N, e))
            assert e < TOL
    # demod_frames afterwards: as of a handle that never made the call
    rx.set_chan_window(0, 0)
    rx.set_chan_average(0)
    back = plain(rx)
    for k in off:
        assert np.array_equal(np.ascontiguousarray(back[k]).view(np.uint8), np.ascontiguousarray(off[k]).view(np.uint8)), k


def test_graph_capture_needs_the_reserve_and_keeps_mode_and_window(om, torch):
    """The FIRST tracking call of the handle is the captured one, so the capture works only because reserve_chan_track sized the
    workspace and loaded the kernels; a batch one frame larger than the reserve, bits without eq (their workspace is not reserved)
    and a handle without ofdm_rx_reserve are refused inside the capture, before anything is enqueued."""
    N, mod = 1024, "16QAM"
    cp, Kd = GEOM[N]
    n, n_sym, n_pat = 5, 12, 3
    d_rx, fl = device_frames(om, torch, N, mod, n, n_sym, 3, seed=14)
    rx, eager_rx, cold = (receiver(om, N, mod, n_sym) for _ in range(3))
    window = (cp // 4, 3 * cp // 4)
    nds = rx.data_symbols_per_frame(fl)

    def buffers():
        return dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                    bits=torch.zeros(n * nds * Kd * 4, dtype=torch.uint8, device="cuda"),
                    csi=torch.zeros(n * nds * Kd, dtype=torch.float32, device="cuda"),
                    takes=torch.zeros(n * n_pat, dtype=torch.int32, device="cuda"), tsr=torch.zeros(n * 4, dtype=torch.int32, device="cuda"))

    def call(r, o, frames, stream, eq=True):
        return r.demod_frames_track(d_rx, frames, fl, fl, om.TRACK_LINEAR, o["eq"] if eq else None, o["bits"], om.BITS_UNPACKED,
                                    o["csi"] if eq else None, None, o["takes"] if eq else None, o["tsr"], stream=stream)

    outs, never = buffers(), buffers()
    rx.reserve(n)
    rx.reserve_chan_track(n - 1, fl)                         # one frame short of the batch that is captured second
    rx.set_chan_window(*window)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                               # the sync search once, eagerly: it touches no tracking workspace
        rx.demod_frames(d_rx, n - 1, fl, fl, d_tsr=never["tsr"], stream=s.cuda_stream)
    s.synchronize()
    never["tsr"].zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cs = torch.cuda.current_stream().cuda_stream
        assert call(rx, outs, n - 1, cs) == nds
        with pytest.raises(ValueError, match="ofdm_rx_reserve_chan_track"):
            call(rx, never, n, cs)                           # a larger batch: the workspace would have to grow
        with pytest.raises(ValueError, match="bits without eq"):
            call(rx, never, n - 1, cs, eq=False)             # the rows' workspace grows on demand only, outside a capture
        with pytest.raises(ValueError, match="call ofdm_rx_reserve first"):
            call(cold, never, n - 1, cs)                     # no frame workspace at all
    assert not any(bool(v.any()) for v in outs.values())     # capture enqueues nothing
    rx.set_chan_window(0, 0)                                 # the graph keeps the window it was captured with
    g.replay()
    torch.cuda.synchronize()
    assert not any(bool(v.any()) for v in never.values()), "a refused call enqueued something"
    want = buffers()
    eager_rx.set_chan_window(*window)
    assert call(eager_rx, want, n - 1, None) == nds
    torch.cuda.synchronize()
    assert want["takes"].cpu().tolist() == [1] * 9 + [0] * 3 + [0] * 3 and bool(want["eq"].any()) and bool(want["bits"].any())
    for k in outs:
        assert torch.equal(outs[k], want[k]), k
    # outside a capture the same calls grow what they need
    rx.set_chan_window(*window)
    assert call(rx, never, n, None) == nds and call(rx, never, n - 1, None, eq=False) == nds
    torch.cuda.synchronize()
    assert torch.equal(never["bits"][:(n - 1) * nds * Kd * 4], want["bits"][:(n - 1) * nds * Kd * 4])


def test_refusals_leave_the_outputs_untouched(om, torch):
    N, Ks, Kd = 64, 62, 60
    rx = engine(om, N, Ks, Kd, (1, 3))
    fl = 8 * 80
    d = torch.zeros(4 * fl * 2, dtype=torch.float32, device="cuda")
    t = torch.ones(16, dtype=torch.int32, device="cuda")
    o, bt, tk = Out(torch, 4 * 6 * Kd * 2, torch.float32), Out(torch, 4 * 6 * Kd * 2, torch.uint8), Out(torch, 8, torch.int32)
    base = dict(d_iq=d, n_frames=4, frame_stride=fl, frame_len=fl, d_tsr=t, mode=om.TRACK_LINEAR, pre=0, post=0, d_eq=o.addr,
                d_bits=bt.addr, bits_mode=om.BITS_UNPACKED, d_takes=tk.addr)
    for kw in (dict(mode=2), dict(mode=-1), dict(pre=-1, post=4), dict(pre=0, post=65), dict(pre=4, post=0), dict(bits_mode=3),
               dict(bits_mode=om.BITS_NONE), dict(n_frames=-1), dict(frame_len=-1, frame_stride=-1), dict(n_frames=1 << 31),
               dict(n_frames=1 << 20, frame_stride=1 << 21), dict(frame_stride=fl - 1), dict(d_iq=None), dict(d_tsr=None),
               dict(d_eq=None, d_bits=None, d_takes=None, bits_mode=om.BITS_NONE)):
        with pytest.raises(ValueError, match="ofdm_chan_track_frames"):
            rx.chan_track_frames(**dict(base, **kw), stream=cur(torch))
    assert rx.chan_track_frames(None, 0, fl, fl, None, d_eq=o.addr) == 6     # no frames: a no-op that returns the row count
    comp = dict(d_iq=d, n_frames=4, frame_stride=fl, frame_len=fl, mode=om.TRACK_LINEAR, d_eq=o.addr, d_bits=bt.addr,
                bits_mode=om.BITS_UNPACKED)
    for kw in (dict(mode=5), dict(bits_mode=om.BITS_NONE), dict(n_frames=-1), dict(frame_stride=fl - 1), dict(d_iq=None),
               dict(d_eq=None, d_bits=None, bits_mode=om.BITS_NONE)):
        with pytest.raises(ValueError, match="ofdm_rx_demod_frames_track"):
            rx.demod_frames_track(**dict(comp, **kw), stream=cur(torch))
    assert rx.demod_frames_track(None, 0, fl, fl, d_eq=o.addr) == 6
    with pytest.raises(ValueError, match="ofdm_rx_reserve_chan_track"):
        rx.reserve_chan_track(-1, fl)
    odd = om.RxEngine(8, N, 16, Ks, (1, 3), 62, tc.SNR_ARG, 0.7)             # num_data_bins % 4 != 0: no packed bits
    with pytest.raises(ValueError, match="packed bits"):
        odd.chan_track_frames(**dict(base, bits_mode=om.BITS_PACKED), stream=cur(torch))
    two = engine(om, N, Ks, Kd, (2, 3))                                      # synch_S != 1
    with pytest.raises(ValueError, match="synch_S"):
        two.chan_track_frames(**base, stream=cur(torch))
    with pytest.raises(ValueError, match="synch_S"):
        two.demod_frames_track(**comp, stream=cur(torch))
    with pytest.raises(ValueError, match="synch_S"):
        two.reserve_chan_track(4, fl)
    torch.cuda.synchronize()
    assert o.untouched() and bt.untouched() and tk.untouched()


# ------------------------------------------------------------------------------------------ 3. end to end
def test_csi_rows_feed_the_weighted_llrs(om, torch):
    """csi with one ROW per segment: demap_csi_frames weighs every symbol with its own interpolated channel power"""
    N, Ks, Kd, synch_dat, n_pat, mod = 64, 62, 60, (1, 3), 4, "16QAM"
    rx = engine(om, N, Ks, Kd, synch_dat, mod)
    b = tc.make_batch(N, Ks, Kd, n_pat, seed=21, synch_dat=synch_dat, mod=mod)
    n, nds = b["iq"].shape[0], n_pat * 3
    d_iq = upload(torch, b["iq"])
    d_tsr = upload(torch, b["tsr"])
    eq, csi = Out(torch, n * nds * Kd * 2, torch.float32), Out(torch, n * nds * Kd, torch.float32)
    llr = Out(torch, n * nds * Kd * 4, torch.float32)
    assert rx.chan_track_frames(d_iq, n, b["stride"], b["frame_len"], d_tsr, d_eq=eq.addr, d_csi=csi.addr, stream=cur(torch)) == nds
    rx.demap_csi_frames(eq.addr, n * nds, 1, Kd, Kd, csi.addr, Kd, rx.csi_rho, mod, llr.addr, stream=cur(torch))
    z, a = eq.read().copy().view(np.complex64).reshape(n * nds, Kd), csi.read().copy().reshape(n * nds, Kd)
    got = llr.read().copy().reshape(n * nds, Kd * 4)
    rho = np.float32(rx.csi_rho)
    for r in range(n * nds):
        assert same_bits(got[r], csi_ref.demap_csi_segment(z[r].reshape(1, Kd), a[r], rho, mod)[0]), r
    assert np.isfinite(got).all() and got.any() and len({a[r].tobytes() for r in range(3)}) == 3


def test_link_end_to_end(om, torch):
    """chantrack_cases.LINK: demod_frames_track gives the transmitted bits of patterns 0-6 back; demod_frames on the same IQ loses
    at least the reference's held count less 10 %"""
    c = tc.LINK
    S, D = c["synch_dat"]
    frames = [tc.link_frame(seed) for seed in c["seeds"]]
    n, fl = len(frames), frames[0]["frame_len"]
    iq = np.stack([fr["x"] for fr in frames]).astype(np.complex64)
    rx = om.RxEngine(S + D, c["N"], c["cp"], c["Ks"], c["synch_dat"], c["Kd"], c["snr_arg"], 0.7, modulation=c["mod"])
    rx.set_max_trials(0)
    d_iq = upload(torch, iq)
    nds = c["n_pat"] * D
    per = nds * c["Kd"] * 2
    bits, held, tsr = (Out(torch, n * per, torch.uint8), Out(torch, n * per, torch.uint8), Out(torch, n * 4, torch.int32))
    assert rx.demod_frames_track(d_iq, n, fl, fl, om.TRACK_LINEAR, d_bits=bits.addr, bits_mode=om.BITS_UNPACKED, d_tsr=tsr.addr,
                                 stream=cur(torch)) == nds
    assert rx.demod_frames(d_iq, n, fl, fl, d_bits=held.addr, bits_mode=om.BITS_UNPACKED, stream=cur(torch)) == nds
    got, hb, t = bits.read().reshape(n, per), held.read().reshape(n, per), tsr.read().reshape(n, 4)
    for f, fr in enumerate(frames):
        lin = int(np.count_nonzero(got[f, :tc.LINK_BITS] != fr["bits"][:tc.LINK_BITS]))
        hel = int(np.count_nonzero(hb[f, :tc.LINK_BITS] != fr["bits"][:tc.LINK_BITS]))
        print("seed %d: tsr %r, bit errors of %d in patterns 0-6: tracked %d, demod_frames %d (reference %d)"
              % (c["seeds"][f], list(t[f]), tc.LINK_BITS, lin, hel, tc.LINK_HELD_LOST[c["seeds"][f]]))
        assert t[f, 3] == 1
        assert lin == 0, (f, lin)
        assert hel >= tc.LINK_HELD_LOST[c["seeds"][f]] * 0.9, (f, hel)
