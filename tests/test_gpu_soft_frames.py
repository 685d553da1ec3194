"""The segmented soft de-mapper (ofdm_demap_frames) and the soft batch receiver (ofdm_rx_demod_frames_soft) on the GPU (-m gpu).

Every segment must carry exactly what ofdm_demap / BitRecovery.work defines for that segment alone: its own sigma, the metrics
of orc.bit_recovery (QPSK) or orc.soft_demap_qam (16/64-QAM) on that segment, and llr = soft0 - soft1 bit for bit.  In the
receiver a segment is one frame's d_eq block, zero rows included; eq, bits and tsr stay those of a plain demod_frames call."""
import numpy as np
import pytest

from conftest import relerr
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

GEOM = {64: (16, 60), 1024: (72, 600), 2048: (144, 1200), 4096: (288, 2400)}       # N: (cp, Kd)
BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}
TOL = 1e-5


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


def cur(torch):
    """the torch stream the test's tensors were written on: the library's calls go behind that work"""
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def sigma_ref(z, mod):
    """sigma = 0.7071*mean(dmin) in fp64 (BitRecovery.py:88,102; the QAM extension's nearest point).  The constellation is the
    library's float32 one (levels m*u rounded to float32): at 64-QAM the fp64 levels differ from those by up to 6e-8, which
    moves a mean distance of 0.04 by 1e-6 -- the metrics check against the fp64 oracle covers that; this check pins the
    per-frame sum."""
    z = np.asarray(z).astype(np.complex64).astype(np.complex128).ravel()
    if mod == "QPSK":
        c = float(np.float32(0.70710678118654752))
        pts = np.array([c + 1j * c, -c + 1j * c, -c - 1j * c, c - 1j * c])
        dmin = np.min(np.abs(z[:, None] - pts[None, :]), axis=1)
    else:
        M = 4 if mod == "16QAM" else 8
        u = np.float32(0.31622776601683794 if mod == "16QAM" else 0.15430334996209191)
        lv = (np.arange(-(M - 1), M, 2).astype(np.float32) * u).astype(np.float64)
        e = [np.min(np.abs(x[:, None] - lv[None, :]), axis=1) for x in (z.real, z.imag)]
        dmin = np.hypot(e[0], e[1])
    return 0.7071067811865476 * np.mean(dmin)


def oracle_soft(z, mod):
    if mod == "QPSK":
        _, s0, s1 = orc.bit_recovery(z)
    else:
        _, s0, s1 = orc.soft_demap_qam(z, mod)
    return s0, s1


def check_segment(z, mod, s0, s1, llr, sig, what=""):
    """one segment's outputs against the oracle on that segment alone (any of s0 / s1 / llr / sig may be None)"""
    r0, r1 = oracle_soft(z, mod)
    if s0 is not None:
        assert relerr(s0, r0) < TOL, (what, "soft0", relerr(s0, r0))
    if s1 is not None:
        assert relerr(s1, r1) < TOL, (what, "soft1", relerr(s1, r1))
    if llr is not None:
        if s0 is not None and s1 is not None:
            assert np.array_equal((np.float32(s0) - np.float32(s1)).view(np.uint32), np.asarray(llr, np.float32).view(np.uint32)), what
        scale = max(np.max(np.abs(r0)), np.max(np.abs(r1)))
        assert np.max(np.abs(np.asarray(llr, np.float64) - (r0 - r1))) <= 2 * TOL * scale, (what, "llr")
    if sig is not None:
        sr = sigma_ref(z, mod)
        assert abs(sig - sr) <= 1e-6 * abs(sr), (what, "sigma", sig, sr)


# ------------------------------------------------------------------------------------------ frames through the receiver
def make_frames(N, mod, n_frames, n_sym, rng, frame_len=None, no_sync=(), late=()):
    """n_frames frames of n_sym symbols through the reference channel with a different noise level per frame (so that every
    frame has its own sigma).  Frames in `no_sync` are noise only; frames in `late` start their sync after 2L + cp, so the last
    pattern fails the guard and its rows are zeros."""
    cp, Kd = GEOM[N]
    L = N + cp
    bps = BPS[mod]
    fl = frame_len or n_sym * L
    out = np.zeros((n_frames, fl), np.complex64)
    for f in range(n_frames):
        noise = 0.01 + 0.03 * f / max(n_frames - 1, 1)
        if f in no_sync:
            out[f] = (0.3 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
            continue
        bits = rng.integers(0, 2, (n_sym // 4) * 3 * Kd * bps).astype(np.uint8)
        tx = orc.channel_apply(orc.tx_modulate(bits, N, cp, N - 2, Kd, n_sym, modulation=mod), orc.REF_TAPS, N)
        lead = 2 * L + cp + 5 if f in late else int(rng.integers(0, cp))
        pre = 0.05 * (rng.standard_normal(lead) + 1j * rng.standard_normal(lead))
        x = np.concatenate([pre, tx])[:fl]
        x = np.concatenate([x, np.zeros(fl - len(x))])
        out[f] = (x + noise * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    return out


def run_receiver(om, N, mod, iq, frame_stride=None, outs=("soft0", "soft1", "llr", "sigma")):
    """-> (plain: eq, bits, tsr of demod_frames), (soft: eq, bits, tsr, soft0, soft1, llr, sigma of demod_frames_soft)"""
    cp, Kd = GEOM[N]
    n_frames, fl = iq.shape
    stride = frame_stride or fl
    n_sym = fl // (N + cp)
    bps = BPS[mod]
    rx = om.RxEngine(max(n_sym, 4), N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    rx.set_max_trials(0)
    nds = rx.data_symbols_per_frame(fl)
    buf = np.zeros((n_frames, stride), np.complex64)
    buf[:, :fl] = iq
    d_iq = om.DeviceBuffer(buf.nbytes).upload(buf)
    n_eq, n_m = n_frames * nds * Kd, n_frames * nds * Kd * bps

    def bufs():
        return dict(eq=om.DeviceBuffer(n_eq * 8), bits=om.DeviceBuffer(n_m), tsr=om.DeviceBuffer(n_frames * 16))

    p = bufs()
    assert rx.demod_frames(d_iq, n_frames, stride, fl, p["eq"], p["bits"], om.BITS_UNPACKED, p["tsr"]) == nds
    s = bufs()
    so = {k: om.DeviceBuffer(max(n_m, 1) * 4) for k in ("soft0", "soft1", "llr") if k in outs}
    sg = om.DeviceBuffer(n_frames * 8) if "sigma" in outs else None
    r = rx.demod_frames_soft(d_iq, n_frames, stride, fl, s["eq"], d_soft0=so.get("soft0"), d_soft1=so.get("soft1"),
                             d_llr=so.get("llr"), d_sigma=sg, d_bits=s["bits"], bits_mode=om.BITS_UNPACKED, d_tsr=s["tsr"])
    assert r == nds

    def get(b):
        return dict(eq=b["eq"].download(np.complex64, n_eq).reshape(n_frames, nds * Kd),
                    bits=b["bits"].download(np.uint8, n_m).reshape(n_frames, -1),
                    tsr=b["tsr"].download(np.int32, n_frames * 4).reshape(n_frames, 4))
    plain, soft = get(p), get(s)
    for k, v in so.items():
        soft[k] = v.download(np.float32, n_m).reshape(n_frames, -1)
    soft["sigma"] = sg.download(np.float64, n_frames) if sg is not None else None
    return plain, soft, nds


def check_frames(plain, soft, mod):
    for k in ("eq", "bits", "tsr"):
        assert np.array_equal(plain[k].view(np.uint8), soft[k].view(np.uint8)), k
    for f in range(plain["eq"].shape[0]):
        z = soft["eq"][f]
        check_segment(z, mod, soft["soft0"][f], soft["soft1"][f], soft["llr"][f], soft["sigma"][f], "frame %d" % f)
        s0, s1 = soft["soft0"][f].astype(np.float64), soft["soft1"][f].astype(np.float64)
        clear = np.abs(s1 - s0) > 1e-4 * np.abs(s0)
        assert np.array_equal(soft["bits"][f][clear], (s1 > s0)[clear].astype(np.uint8)), "frame %d: hard bit vs soft" % f


# ------------------------------------------------------------------------------------------ 1. per-frame parity
CASES = [(64, "QPSK", 19, 16)] + [(N, mod, 3 if N < 4096 else 2, 8) for N in (1024, 2048, 4096) for mod in BPS]


@pytest.mark.parametrize("N,mod,n_frames,n_sym", CASES)
def test_per_frame_parity(om, N, mod, n_frames, n_sym):
    rng = np.random.default_rng(N * 7 + BPS[mod])
    iq = make_frames(N, mod, n_frames, n_sym, rng)
    plain, soft, nds = run_receiver(om, N, mod, iq)
    assert nds > 0 and plain["tsr"][:, 3].all(), "every frame should find its sync"
    assert len(set(np.round(soft["sigma"], 12))) == n_frames, "frames with different noise must get different sigmas"
    check_frames(plain, soft, mod)


@pytest.mark.parametrize("mod", ["QPSK", "64QAM"])
def test_ragged_frame_len_and_stride(om, mod):
    """frame_len not a whole number of symbols, frame_stride > frame_len"""
    N = 1024
    cp, _ = GEOM[N]
    L = N + cp
    rng = np.random.default_rng(5)
    fl = 9 * L + 301
    iq = make_frames(N, mod, 3, 9, rng, frame_len=fl)
    plain, soft, nds = run_receiver(om, N, mod, iq, frame_stride=fl + 77)
    assert nds == 6
    check_frames(plain, soft, mod)


# ------------------------------------------------------------------------------------------ 2. reference pin
def test_reference_bitrecovery_pin(om, golden):
    g = golden("ref_bitrecovery.npz")
    z = np.ascontiguousarray(g["z"], np.complex64)
    n = z.size
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    d_z = om.DeviceBuffer(z.nbytes).upload(z)
    d0, d1, dl = (om.DeviceBuffer(n * 2 * 4) for _ in range(3))
    ds = om.DeviceBuffer(8 * 8)
    rx.demap_frames(d_z, 1, n, n, "QPSK", d0, d1, dl, ds)
    s0, s1 = d0.download(np.float32, 2 * n), d1.download(np.float32, 2 * n)
    assert relerr(s0, g["softbit0"]) < TOL and relerr(s1, g["softbit1"]) < TOL
    assert np.array_equal((s0 - s1).view(np.uint32), dl.download(np.float32, 2 * n).view(np.uint32))
    # uneven segments of the same symbols (a segment = a fresh work() call): as many starts as fit, stride = longest
    cuts = [0, 1, 4, 261, 1700, 1703, 2900, n]
    lens = np.diff(cuts)
    stride = int(lens.max())
    for k, ln in enumerate(lens):
        rx.demap_frames(d_z.data_ptr() + 8 * cuts[k], 1, int(ln), int(ln), "QPSK", d0, d1, dl, ds)
        a0, a1 = d0.download(np.float32, 2 * ln), d1.download(np.float32, 2 * ln)
        check_segment(z[cuts[k]:cuts[k + 1]], "QPSK", a0, a1, dl.download(np.float32, 2 * ln), ds.download(np.float64, 1)[0],
                      "cut %d" % k)
    # the same segments in ONE call, padded to a common stride
    padded = np.zeros((len(lens), stride), np.complex64)
    for k, ln in enumerate(lens):
        padded[k, :ln] = z[cuts[k]:cuts[k + 1]]
    d_p = om.DeviceBuffer(padded.nbytes).upload(padded)
    for k, ln in enumerate(lens):
        rx.demap_frames(d_p.data_ptr() + 8 * k * stride, 1, int(ln), stride, "QPSK", d0, d1, None, ds)
        r0, r1 = oracle_soft(z[cuts[k]:cuts[k + 1]], "QPSK")
        assert relerr(d0.download(np.float32, 2 * ln), r0) < TOL and relerr(d1.download(np.float32, 2 * ln), r1) < TOL


# ------------------------------------------------------------------------------------------ 3. independence, determinism
def _rand_syms(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


@pytest.mark.parametrize("mod", list(BPS))
def test_segment_alone_equals_batch_and_repeats(om, torch, mod):
    rng = np.random.default_rng(31 + BPS[mod])
    n_seg, seg_len, stride = 50, 5003, 5011                  # several slices per segment, odd lengths: every path
    bps = BPS[mod]
    host = np.stack([_rand_syms(rng, stride, 0.2 + 0.05 * s) for s in range(n_seg)])
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    d_sym = torch.from_numpy(host.view(np.float32)).cuda()
    n_m = n_seg * seg_len * bps

    def call(ptr_sym, ns):
        o = [torch.full((ns * seg_len * bps,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
        sg = torch.full((ns,), float("nan"), dtype=torch.float64, device="cuda")
        rx.demap_frames(ptr_sym, ns, seg_len, stride, mod, o[0], o[1], o[2], sg, stream=cur(torch))
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in o] + [sg.cpu().numpy()]

    b1 = call(d_sym, n_seg)
    b2 = call(d_sym, n_seg)
    for x, y in zip(b1, b2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "second call differs"
    assert b1[0].size == n_m
    for s in (0, 17, 49):
        alone = call(d_sym.data_ptr() + 8 * s * stride, 1)
        sl = slice(s * seg_len * bps, (s + 1) * seg_len * bps)
        for x, y in zip(alone[:3], b1[:3]):
            assert np.array_equal(x.view(np.uint32), y[sl].view(np.uint32)), s
        assert alone[3][0] == b1[3][s]
        # the same symbols copied to an address 8 bytes off the 16-byte grid: the scalar paths give the same bits
        t = torch.zeros(seg_len * 2 + 2, dtype=torch.float32, device="cuda")
        t[2:] = torch.from_numpy(host[s, :seg_len].view(np.float32)).cuda()
        shifted = call(t.data_ptr() + 8, 1)
        for x, y in zip(shifted, alone):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), s
        check_segment(host[s, :seg_len], mod, b1[0][sl], b1[1][sl], b1[2][sl], b1[3][s], "segment %d" % s)


# ------------------------------------------------------------------------------------------ 4. no sync, guard-failed rows
@pytest.mark.parametrize("mod", list(BPS))
def test_frames_without_sync_and_guard_failed_rows(om, mod):
    N = 1024
    rng = np.random.default_rng(77 + BPS[mod])
    iq = make_frames(N, mod, 4, 12, rng, no_sync=(1,), late=(2,))
    plain, soft, nds = run_receiver(om, N, mod, iq)
    _, Kd = GEOM[N]
    assert plain["tsr"][1, 3] == 0 and not plain["eq"][1].any(), "frame 1 must have no sync and all-zero rows"
    rows2 = plain["eq"][2].reshape(nds, Kd)
    assert plain["tsr"][2, 3] and not rows2[-1].any() and rows2[0].any(), "frame 2 must end in guard-failed zero rows"
    check_frames(plain, soft, mod)


# ------------------------------------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("mod", list(BPS))
@pytest.mark.parametrize("seg_len", [1, 3, 4, 5, 257])
def test_short_segments_misaligned_and_strided(om, torch, mod, seg_len):
    rng = np.random.default_rng(seg_len * 13 + BPS[mod])
    bps = BPS[mod]
    n_seg, stride = 7, seg_len + 3
    host = np.stack([_rand_syms(rng, stride, 0.3 + 0.1 * s) for s in range(n_seg)])
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    for sym_off, out_off in ((0, 0), (8, 4), (8, 0), (0, 4)):
        base = torch.zeros(host.size * 2 + 4, dtype=torch.float32, device="cuda")
        base[sym_off // 4:sym_off // 4 + host.size * 2] = torch.from_numpy(host.view(np.float32).ravel()).cuda()
        n_m = n_seg * seg_len * bps
        o = [torch.full((n_m + 4,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
        sg = torch.zeros(n_seg, dtype=torch.float64, device="cuda")
        rx.demap_frames(base.data_ptr() + sym_off, n_seg, seg_len, stride, mod, *(x.data_ptr() + out_off for x in o), sg,
                        stream=cur(torch))
        torch.cuda.synchronize()
        k = out_off // 4
        got = [x.cpu().numpy()[k:k + n_m] for x in o]
        for x in o:
            h = x.cpu().numpy()
            assert np.isnan(h[:k]).all() and np.isnan(h[k + n_m:]).all(), "wrote outside its segment"
        for s in range(n_seg):
            sl = slice(s * seg_len * bps, (s + 1) * seg_len * bps)
            check_segment(host[s, :seg_len], mod, got[0][sl], got[1][sl], got[2][sl], sg.cpu().numpy()[s],
                          "seg %d off %d/%d" % (s, sym_off, out_off))


@pytest.mark.parametrize("mod", list(BPS))
def test_each_output_alone(om, torch, mod):
    rng = np.random.default_rng(3)
    bps = BPS[mod]
    n_seg, seg_len = 5, 3000
    host = np.stack([_rand_syms(rng, seg_len, 0.4 + 0.1 * s) for s in range(n_seg)])
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    d = torch.from_numpy(host.view(np.float32)).cuda()
    n_m = n_seg * seg_len * bps
    full = [torch.zeros(n_m, dtype=torch.float32, device="cuda") for _ in range(3)] + [torch.zeros(n_seg, dtype=torch.float64,
                                                                                                    device="cuda")]
    rx.demap_frames(d, n_seg, seg_len, seg_len, mod, *full, stream=cur(torch))
    for i in range(4):
        one = [None] * 4
        one[i] = torch.full_like(full[i], float("nan"))
        rx.demap_frames(d, n_seg, seg_len, seg_len, mod, *one, stream=cur(torch))
        torch.cuda.synchronize()
        assert torch.equal(one[i], full[i]), i
    nothing = torch.full_like(full[0], 7.0)
    rx.demap_frames(d, 0, seg_len, seg_len, mod, nothing, stream=cur(torch))          # n_seg = 0
    rx.demap_frames(d, n_seg, 0, 0, mod, nothing, stream=cur(torch))                  # seg_len = 0
    rx.demap_frames(d, n_seg, seg_len, seg_len, mod, stream=cur(torch))               # no output at all
    torch.cuda.synchronize()
    assert bool((nothing == 7.0).all())


def test_argument_errors(om, torch):
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    o = torch.zeros(64, dtype=torch.float32, device="cuda")
    for args in ((-1, 4, 4, "QPSK"), (1, -4, 4, "QPSK"), (2, 4, 3, "QPSK"), (1, 4, 4, "BPSK"), (1, 4, 4, 3),
                 (1 << 32, 4, 4, "QPSK"), (4, 1 << 41, 1 << 41, "QPSK"), (1 << 20, 8, 1 << 30, "QPSK")):
        with pytest.raises(ValueError):
            rx.demap_frames(d, *args, d_soft0=o)
    with pytest.raises(ValueError):
        rx.demap_frames(None, 1, 4, 4, "QPSK", d_soft0=o)
    with pytest.raises(ValueError):                                         # soft outputs need d_eq
        rx.demod_frames_soft(d, 1, 32, 32, None, d_llr=o)
    with pytest.raises(ValueError):
        rx.demod_frames_soft(d, 1, 16, 32, d, d_llr=o)                      # frame_stride < frame_len
    with pytest.raises(ValueError):
        rx.demod_frames_soft(d, 1, 32, 32, d, d_llr=o, d_bits=o, bits_mode=7)
    bp = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100, modulation="BPSK")
    with pytest.raises(ValueError):
        bp.demod_frames_soft(d, 1, 32, 32, d, d_llr=o)
    assert "ofdm_rx_demod_frames_soft" in om._lib.last_error()


def test_output_beyond_4gib(om, torch):
    """64-QAM llr of 190M symbols = 4.56 GB: segments sampled across the whole array match the oracle"""
    mod, bps = "64QAM", 6
    seg_len, n_seg = 95_000, 2000
    n_m = n_seg * seg_len * bps
    assert n_m * 4 > (1 << 32)
    torch.manual_seed(0)
    sym = (torch.randn(n_seg * seg_len * 2, dtype=torch.float32, device="cuda") * 0.3)
    llr = torch.empty(n_m, dtype=torch.float32, device="cuda")
    sg = torch.empty(n_seg, dtype=torch.float64, device="cuda")
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    rx.demap_frames(sym, n_seg, seg_len, seg_len, mod, d_llr=llr, d_sigma=sg, stream=cur(torch))
    torch.cuda.synchronize()
    sig = sg.cpu().numpy()
    for s in (0, 1, 1883, 1884, n_seg - 1):                                 # segment 1883 crosses 2^32 bytes
        z = sym[s * seg_len * 2:(s + 1) * seg_len * 2].cpu().numpy().view(np.complex64)
        got = llr[s * seg_len * bps:(s + 1) * seg_len * bps].cpu().numpy()
        check_segment(z, mod, None, None, got, sig[s], "segment %d" % s)
    del sym, llr
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 6. graph capture
def test_graph_capture_equals_eager(om, torch):
    N, mod = 1024, "16QAM"
    cp, Kd = GEOM[N]
    rng = np.random.default_rng(12)
    iq = make_frames(N, mod, 6, 8, rng)
    n, fl = iq.shape
    rx = om.RxEngine(8, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    rx.set_max_trials(0)
    nds = rx.data_symbols_per_frame(fl)
    n_m = n * nds * Kd * 4
    rx.reserve(n)
    rx.reserve_soft(n, nds * Kd)
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                bits=torch.zeros(n * nds * Kd // 2, dtype=torch.uint8, device="cuda"),
                tsr=torch.zeros(n * 4, dtype=torch.int32, device="cuda"),
                soft0=torch.zeros(n_m, dtype=torch.float32, device="cuda"),
                soft1=torch.zeros(n_m, dtype=torch.float32, device="cuda"),
                llr=torch.zeros(n_m, dtype=torch.float32, device="cuda"),
                sigma=torch.zeros(n, dtype=torch.float64, device="cuda"))
    s = torch.cuda.Stream()

    def call(stream):
        rx.demod_frames_soft(d_iq, n, fl, fl, outs["eq"], d_soft0=outs["soft0"], d_soft1=outs["soft1"], d_llr=outs["llr"],
                             d_sigma=outs["sigma"], d_bits=outs["bits"], bits_mode=om.BITS_PACKED, d_tsr=outs["tsr"],
                             stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["sigma"] > 0).all())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert not outs["sigma"].any()                                          # capture enqueues nothing
    for _ in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], eager[k]), k
