"""The pilot-aided phase-tracking stage (ofdm_pilot_track_frames) and the receiver that runs it (ofdm_rx_demod_frames_pilots) on
the GPU (-m gpu).  The contract is tests/pilot_ref.py (fp64); the GPU is held against it on the SAME call's d_eq.

Inputs of the end-to-end cases (CASES): chosen on the CPU first.  For every case the fp64 restatement on RxOracle rows (snr 100,
7-sample lead, 240 symbols, the seeds the cases use) de-maps all 180 rows without a single bit error in both modes at the listed noise AND at
twice that noise, while the untracked rows have a bit error rate of 0.41-0.52: ICI grows with the offset, so 64-QAM gets
eps 0.002-0.004, 16-QAM 0.005-0.01, QPSK 0.01.  No row is left out of the comparison: the sync lies inside the first cp samples
and the frame is cp samples longer than its symbols, so every pattern passes the reference's guard (asserted: 0 zero rows)."""
import numpy as np
import pytest

import pilot_ref as pr
from conftest import relerr
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

GEOM = {64: (16, 60), 1024: (72, 600), 2048: (144, 1200), 4096: (288, 2400)}       # N: (cp, K occupied bins)
BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}
TOL = 1e-5
N_SYM = 240


def comb(K, n=7):
    step = (K // 2) // (n + 1)
    return [s * step * m for m in range(1, n + 1) for s in (-1, 1)]


def pilots_of(N):
    return [-21, -7, 7, 21] if N == 64 else comb(GEOM[N][1])


#        N     constellation  eps    noise  frames
CASES = [(64, "QPSK", 0.01, 0.02, 3),
         (64, "16QAM", 0.005, 0.005, 2),
         (64, "64QAM", 0.002, 0.002, 2),
         (1024, "QPSK", 0.01, 0.02, 2),
         (1024, "16QAM", 0.01, 0.01, 2),
         (2048, "64QAM", 0.004, 0.003, 1),
         (4096, "QPSK", 0.01, 0.02, 1),
         (4096, "64QAM", 0.004, 0.003, 1)]


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


def cur(torch):
    return torch.cuda.current_stream().cuda_stream


def pack_msb(bits_rows):
    return np.packbits(np.asarray(bits_rows, np.uint8), axis=-1, bitorder="big")


def receiver(om, N, mod, locs, snr=100):
    cp, K = GEOM[N]
    rx = om.RxEngine(N_SYM, N, cp, N - 2, (1, 3), K, snr, 0.7, modulation=mod)
    rx.set_max_trials(0)
    rx.set_pilots(locs, 1.0)
    return rx


def run_pilots(om, rx, N, mod, locs, iq, mode, bits_mode=None, stride=None, soft=False):
    """demod_frames_pilots on iq [n_frames][fl] -> dict of host arrays"""
    cp, K = GEOM[N]
    Kd = K - len(locs)
    bps = BPS[mod]
    n, fl = iq.shape
    stride = stride or fl
    buf = np.zeros((n, stride), np.complex64)
    buf[:, :fl] = iq
    d_iq = om.DeviceBuffer(buf.nbytes).upload(buf)
    nds = rx.data_symbols_per_frame(fl)
    bits_mode = om.BITS_UNPACKED if bits_mode is None else bits_mode
    nb = n * nds * Kd * bps // (8 if bits_mode == om.BITS_PACKED else 1)
    d = dict(eq=om.DeviceBuffer(n * nds * K * 8), tsr=om.DeviceBuffer(n * 16), data=om.DeviceBuffer(n * nds * Kd * 8),
             bits=om.DeviceBuffer(nb), cpe=om.DeviceBuffer(n * nds * 8), slope=om.DeviceBuffer(n * nds * 4),
             cfo=om.DeviceBuffer(n * 8))
    s = {k: om.DeviceBuffer(n * nds * Kd * bps * 4) for k in ("soft0", "soft1", "llr")} if soft else {}
    sg = om.DeviceBuffer(n * 8) if soft else None
    r = rx.demod_frames_pilots(d_iq, n, stride, fl, d["eq"], mode=mode, d_data=d["data"], d_bits=d["bits"], bits_mode=bits_mode,
                               d_cpe=d["cpe"], d_slope=d["slope"] if mode == pr.CPE_SLOPE else None, d_cfo=d["cfo"],
                               d_soft0=s.get("soft0"), d_soft1=s.get("soft1"), d_llr=s.get("llr"), d_sigma=sg, d_tsr=d["tsr"])
    assert r == nds
    out = dict(nds=nds, d_iq=d_iq, dev=d,
               eq=d["eq"].download(np.complex64, n * nds * K).reshape(n, nds, K),
               tsr=d["tsr"].download(np.int32, n * 4).reshape(n, 4),
               data=d["data"].download(np.complex64, n * nds * Kd).reshape(n, nds, Kd),
               bits=d["bits"].download(np.uint8, nb).reshape(n, nds, -1),
               cpe=d["cpe"].download(np.complex64, n * nds).reshape(n, nds),
               slope=d["slope"].download(np.float32, n * nds).reshape(n, nds) if mode == pr.CPE_SLOPE else None,
               cfo=d["cfo"].download(np.float64, n))
    for k, v in s.items():
        out[k] = v.download(np.float32, n * nds * Kd * bps).reshape(n, -1)
    if soft:
        out["sigma"] = sg.download(np.float64, n)
    return out


def check_against_ref(res, N, mod, locs, mode, packed=False):
    """data / cpe / slope / cfo of one call against the fp64 restatement on that call's d_eq; bits against the stored data"""
    cp, K = GEOM[N]
    ref = pr.track_rows(res["eq"], locs, 1.0, mode)
    figs = dict(data=relerr(res["data"], ref["data"]), cpe=relerr(res["cpe"], ref["cpe"]))
    if mode == pr.CPE_SLOPE:
        figs["slope"] = relerr(res["slope"], ref["slope"])
    n, nds, Kd = res["data"].shape
    for f in range(n):
        want = pr.cfo_estimate(ref["U"][f], ref["usable"][f], 3, N, cp)
        got = res["cfo"][f]
        if np.isnan(want):
            assert np.isnan(got), (f, got)
            continue
        figs["cfo_abs_%d" % f] = abs(got - want)
        figs["cfo_tol_%d" % f] = 1e-6 * abs(want) + 1e-9
    print("pilot parity N=%d %s mode=%d:" % (N, mod, mode), {k: "%.3g" % v for k, v in figs.items()})
    assert figs["data"] < TOL and figs["cpe"] < TOL, figs
    if mode == pr.CPE_SLOPE:
        assert figs["slope"] < TOL, figs
    for f in range(n):
        if "cfo_abs_%d" % f in figs:
            assert figs["cfo_abs_%d" % f] <= figs["cfo_tol_%d" % f], figs
    hb = pr.hard_bits(res["data"], mod).reshape(n, nds, Kd * BPS[mod])
    if packed:
        assert np.array_equal(res["bits"], pack_msb(hb)), "packed bits differ from the hard decision of the stored data"
    else:
        assert np.array_equal(res["bits"], hb), "bits differ from the hard decision of the stored data"
    return hb


_frames = {}


def frames_of(case):
    if case not in _frames:
        N, mod, eps, noise, n = case
        cp, K = GEOM[N]
        fr = [pr.make_frame(N, cp, K, pilots_of(N), mod, N_SYM, eps, noise, seed=1 + f, lead=7) for f in range(n)]
        _frames[case] = (np.stack([x for x, _ in fr]).astype(np.complex64), np.stack([b for _, b in fr]))
    return _frames[case]


# ------------------------------------------------------------------------------------------ 1 + 2: end to end, parity
@pytest.mark.parametrize("mode", [pr.CPE, pr.CPE_SLOPE])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-%s" % (c[0], c[1]))
def test_tracked_bits_equal_transmitted_bits(om, case, mode):
    """Fails without the stage: the plain rows' hard bits are wrong in the later symbols, the tracked bits are the transmitted
    bits on every row."""
    N, mod, eps, noise, n = case
    cp, K = GEOM[N]
    locs = pilots_of(N)
    iq, tx_bits = frames_of(case)
    rx = receiver(om, N, mod, locs)
    res = run_pilots(om, rx, N, mod, locs, iq, mode)
    nds, Kd, bps = res["nds"], K - len(locs), BPS[mod]
    assert nds == 180 and res["tsr"][:, 3].all()
    zero_rows = int((~res["eq"].any(axis=2)).sum())
    assert zero_rows == 0, "every pattern passes the guard with these frames: no row is left out of the comparison"
    hb = check_against_ref(res, N, mod, locs, mode)
    _, _, didx, _ = pr.layout(K, locs)
    plain = pr.hard_bits(res["eq"][:, :, didx], mod).reshape(n, nds, Kd * bps)
    want = tx_bits.reshape(n, nds, Kd * bps)
    late = slice(nds * 3 // 4, nds)
    ber_plain = float((plain[:, late] != want[:, late]).mean())
    print("N=%d %s eps=%g: plain BER of the last quarter %.3f, cfo %s" % (N, mod, eps, ber_plain, res["cfo"]))
    assert ber_plain > 0.1, "the untracked rows should have lost the constellation by the end of the frame"
    assert np.array_equal(hb, want), "tracked bits differ from the transmitted bits: %d errors" % int((hb != want).sum())


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[2]], ids=lambda c: "%d-%s" % (c[0], c[1]))
def test_packed_bits_and_identity_with_plain_call(om, case):
    """d_eq and d_tsr are the plain call's bits; packed bits; the soft outputs are demap_frames over the tracked data"""
    N, mod, eps, noise, n = case
    cp, K = GEOM[N]
    locs = pilots_of(N)
    Kd, bps = K - len(locs), BPS[mod]
    iq, _ = frames_of(case)
    rx = receiver(om, N, mod, locs)
    res = run_pilots(om, rx, N, mod, locs, iq, pr.CPE, bits_mode=om.BITS_PACKED, stride=iq.shape[1] + 33, soft=True)
    check_against_ref(res, N, mod, locs, pr.CPE, packed=True)
    nds = res["nds"]
    d_eq, d_tsr = om.DeviceBuffer(n * nds * K * 8), om.DeviceBuffer(n * 16)
    assert rx.demod_frames(res["d_iq"], n, iq.shape[1] + 33, iq.shape[1], d_eq, None, om.BITS_NONE, d_tsr) == nds
    assert np.array_equal(d_eq.download(np.uint8, n * nds * K * 8), res["dev"]["eq"].download(np.uint8, n * nds * K * 8))
    assert np.array_equal(d_tsr.download(np.int32, n * 4), res["tsr"].ravel())
    nm = n * nds * Kd * bps
    h = {k: om.DeviceBuffer(nm * 4) for k in ("soft0", "soft1", "llr")}
    hs = om.DeviceBuffer(n * 8)
    rx.demap_frames(res["dev"]["data"], n, nds * Kd, nds * Kd, mod, h["soft0"], h["soft1"], h["llr"], hs)
    for k in h:
        assert np.array_equal(h[k].download(np.uint32, nm), res[k].view(np.uint32).ravel()), k
    assert np.array_equal(hs.download(np.float64, n), res["sigma"]) and np.all(res["sigma"] > 0)
    s0, s1 = orc.soft_demap_qam(res["data"][0].ravel(), mod)[1:] if mod != "QPSK" else orc.bit_recovery(res["data"][0].ravel())[1:]
    assert relerr(res["soft0"][0], s0) < TOL and relerr(res["soft1"][0], s1) < TOL


# ------------------------------------------------------------------------------------------ 4: zero rows, frames without sync
@pytest.mark.parametrize("mode", [pr.CPE, pr.CPE_SLOPE])
def test_zero_rows_and_frames_without_sync(om, mode):
    N, mod = 1024, "16QAM"
    cp, K = GEOM[N]
    L = N + cp
    locs = pilots_of(N)
    n_sym = 16
    fl = n_sym * L + cp
    rng = np.random.default_rng(4)
    iq = np.zeros((3, fl), np.complex64)
    iq[0] = pr.make_frame(N, cp, K, locs, mod, n_sym, 0.01, 0.01, seed=8, frame_len=fl)[0]
    iq[1] = 0.3 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))                     # no sync at all
    iq[2] = pr.make_frame(N, cp, K, locs, mod, n_sym, 0.01, 0.01, seed=9, frame_len=fl, lead=2 * L + 2 * cp + 40)[0]   # late sync
    rx = receiver(om, N, mod, locs)
    res = run_pilots(om, rx, N, mod, locs, iq, mode)
    assert res["tsr"][0, 3] and not res["tsr"][1, 3] and res["tsr"][2, 3]
    zero = ~res["eq"].any(axis=2)
    assert not zero[0].any() and zero[1].all() and zero[2, -3:].all() and not zero[2, :-3].any()
    assert not res["data"][zero].any() and not res["cpe"][zero].any(), "zero rows stay zero, their cpe is 0"
    assert np.isfinite(res["data"]).all() and np.isfinite(res["cpe"]).all()
    if mode == pr.CPE_SLOPE:
        assert np.isfinite(res["slope"]).all() and not res["slope"][zero].any()
    assert np.isfinite(res["cfo"][[0, 2]]).all() and np.isnan(res["cfo"][1]), res["cfo"]
    check_against_ref(res, N, mod, locs, mode)


# ------------------------------------------------------------------------------------------ 5: determinism (the stage alone)
def _rows(rng, n, K, locs, scale=1.0):
    """rows that look like equalised symbols: unit-power data, pilots near a common rotation per row"""
    z = (rng.standard_normal((n, K)) + 1j * rng.standard_normal((n, K))) * scale / np.sqrt(2)
    pidx = pr.layout(K, locs)[0]
    ph = rng.uniform(-np.pi, np.pi, n)
    z[:, pidx] = np.exp(1j * ph)[:, None] * (1 + 0.05 * (rng.standard_normal((n, len(locs))) + 1j * rng.standard_normal((n, len(locs)))))
    return z.astype(np.complex64)


def stage(om, torch, rx, d_sym, n_seg, rows, stride, K, n_p, mod, mode, bits_mode, rpp=3, data_off=0):
    Kd, bps = K - n_p, BPS[mod]
    nb = n_seg * rows * Kd * bps // (8 if bits_mode == om.BITS_PACKED else 1)
    data = torch.full((n_seg * rows * Kd * 2 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    bits = torch.full((nb + 8,), 255, dtype=torch.uint8, device="cuda")
    cpe = torch.full((n_seg * rows * 2,), float("nan"), dtype=torch.float32, device="cuda")
    slope = torch.full((n_seg * rows,), float("nan"), dtype=torch.float32, device="cuda")
    cfo = torch.full((n_seg,), 7.0, dtype=torch.float64, device="cuda")
    rx.pilot_track_frames(d_sym, n_seg, rows, stride, rpp, mode, d_data=data.data_ptr() + data_off, d_bits=bits, bits_mode=bits_mode,
                          d_cpe=cpe, d_slope=slope if mode == pr.CPE_SLOPE else None, d_cfo=cfo, stream=cur(torch))
    torch.cuda.synchronize()
    hd = data.cpu().numpy()
    k = data_off // 4
    assert np.isnan(hd[:k]).all() and np.isnan(hd[k + n_seg * rows * Kd * 2:]).all(), "wrote outside data"
    hb = bits.cpu().numpy()
    assert (hb[nb:] == 255).all(), "wrote outside bits"
    return dict(data=hd[k:k + n_seg * rows * Kd * 2].view(np.complex64).reshape(n_seg, rows, Kd), bits=hb[:nb].reshape(n_seg, rows, -1),
                cpe=cpe.cpu().numpy().view(np.complex64).reshape(n_seg, rows), slope=slope.cpu().numpy().reshape(n_seg, rows),
                cfo=cfo.cpu().numpy())


def same_bits(a, b, what):
    for k in ("data", "bits", "cpe", "slope", "cfo"):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


@pytest.mark.parametrize("N,mod,mode", [(64, "QPSK", pr.CPE), (64, "16QAM", pr.CPE_SLOPE), (2048, "64QAM", pr.CPE),
                                        (1024, "16QAM", pr.CPE_SLOPE)])
def test_segment_alone_in_batch_strided_and_repeated(om, torch, N, mod, mode):
    cp, K = GEOM[N]
    locs = pilots_of(N) if N == 64 else comb(K, 8)                    # 16 pilots: (K - 16) * bps is a multiple of 8 for packed bits
    rng = np.random.default_rng(N + mode)
    n_seg, rows = 9, 13
    stride = rows * K + 5                                             # odd stride: segments 1, 3, .. start 8 bytes off the 16-byte grid
    host = np.zeros((n_seg, stride), np.complex64)
    host[:, :rows * K] = _rows(rng, n_seg * rows, K, locs).reshape(n_seg, rows * K)
    rx = receiver(om, N, mod, locs)
    d = torch.from_numpy(host.view(np.float32)).cuda()
    bm = om.BITS_PACKED
    b1 = stage(om, torch, rx, d, n_seg, rows, stride, K, len(locs), mod, mode, bm)
    b2 = stage(om, torch, rx, d, n_seg, rows, stride, K, len(locs), mod, mode, bm)
    same_bits(b1, b2, "second call")
    dense = torch.from_numpy(np.ascontiguousarray(host[:, :rows * K]).view(np.float32)).cuda()
    b3 = stage(om, torch, rx, dense, n_seg, rows, rows * K, K, len(locs), mod, mode, bm)
    same_bits(b1, b3, "dense layout")
    for s in (0, 4, 8):
        alone = stage(om, torch, rx, d.data_ptr() + 8 * s * stride, 1, rows, stride, K, len(locs), mod, mode, bm)
        same_bits({k: v[s:s + 1] for k, v in b1.items()}, alone, "segment %d alone" % s)
        shifted = stage(om, torch, rx, d.data_ptr() + 8 * s * stride, 1, rows, stride, K, len(locs), mod, mode, bm, data_off=8)
        same_bits(alone, shifted, "output 8 bytes off the 16-byte grid")
    ref = pr.track_rows(host[:, :rows * K].reshape(n_seg, rows, K), locs, 1.0, mode)
    assert relerr(b1["data"], ref["data"]) < TOL and relerr(b1["cpe"], ref["cpe"]) < TOL
    hb = pr.hard_bits(b1["data"], mod).reshape(n_seg, rows, -1)
    assert np.array_equal(b1["bits"], pack_msb(hb))
    u = stage(om, torch, rx, d, n_seg, rows, stride, K, len(locs), mod, mode, om.BITS_UNPACKED)
    assert np.array_equal(u["bits"], hb) and np.array_equal(u["data"].view(np.uint8), b1["data"].view(np.uint8))
    for s in range(n_seg):
        want = pr.cfo_estimate(ref["U"][s], ref["usable"][s], 3, N, cp)
        assert abs(b1["cfo"][s] - want) <= 1e-6 * abs(want) + 1e-9, (s, b1["cfo"][s], want)


def test_odd_data_count_and_many_pilots(om, torch):
    """K - n_pilots odd (rows of an odd length start 8 bytes off every other row), more pilots than lanes in a group"""
    N, mod = 64, "16QAM"
    K = 60
    rng = np.random.default_rng(2)
    for locs in ([-21, 7, 21], list(range(-30, 0)) + [1, 2, 3, 5, 8], [-30, 30, 1, -1, 29]):
        rx = receiver(om, N, mod, locs)
        n_seg, rows = 3, 7
        host = _rows(rng, n_seg * rows, K, locs).reshape(n_seg, rows * K)
        d = torch.from_numpy(host.view(np.float32)).cuda()
        for mode in (pr.CPE, pr.CPE_SLOPE):
            r = stage(om, torch, rx, d, n_seg, rows, rows * K, K, len(locs), mod, mode, om.BITS_UNPACKED)
            ref = pr.track_rows(host.reshape(n_seg, rows, K), locs, 1.0, mode)
            assert relerr(r["data"], ref["data"]) < TOL and relerr(r["cpe"], ref["cpe"]) < TOL, (locs, mode)
            if mode == pr.CPE_SLOPE:
                assert relerr(r["slope"], ref["slope"]) < TOL, locs
            assert np.array_equal(r["bits"], pr.hard_bits(r["data"], mod).reshape(n_seg, rows, -1))


# ------------------------------------------------------------------------------------------ 6: errors, edges, size, capture
def test_argument_errors(om, torch):
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100, modulation="QPSK")
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    o = torch.zeros(4096, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):                                         # no pilots set
        rx.pilot_track_frames(d, 1, 2, 120, 3, d_data=o)
    with pytest.raises(ValueError):
        rx.demod_frames_pilots(d, 1, 640, 640, o, d_data=o)
    for bad in ([0], [31], [-31], [7, 7], list(range(1, 31)) * 3):
        with pytest.raises(ValueError):
            rx.set_pilots(bad)
    rx.set_pilots([5])
    with pytest.raises(ValueError):                                         # slope needs two pilots
        rx.pilot_track_frames(d, 1, 2, 120, 3, pr.CPE_SLOPE, d_data=o)
    rx.set_pilots([-21, -7, 7, 21])
    for args in ((-1, 2, 120, 3, 0), (1, -2, 120, 3, 0), (1, 2, 119, 3, 0), (1, 2, 120, 0, 0), (1, 2, 120, 3, 2), (1 << 31, 2, 120, 3, 0),
                 (1 << 20, 1 << 12, 1 << 30, 3, 0)):
        with pytest.raises(ValueError):
            rx.pilot_track_frames(d, *args, d_data=o)
    with pytest.raises(ValueError):                                         # bits without data
        rx.pilot_track_frames(d, 1, 2, 120, 3, d_bits=o, bits_mode=om.BITS_UNPACKED)
    with pytest.raises(ValueError):
        rx.pilot_track_frames(d, 1, 2, 120, 3, d_data=o, d_bits=o, bits_mode=7)
    with pytest.raises(ValueError):                                         # slope output in CPE mode
        rx.pilot_track_frames(d, 1, 2, 120, 3, pr.CPE, d_data=o, d_slope=o)
    with pytest.raises(ValueError):
        rx.pilot_track_frames(None, 1, 2, 120, 3, d_data=o)
    rx.set_pilots([-21, 7, 21])                                             # 57 data entries: 114 bits per row
    with pytest.raises(ValueError):
        rx.pilot_track_frames(d, 1, 2, 120, 3, d_data=o, d_bits=o, bits_mode=om.BITS_PACKED)
    rx.set_pilots([-21, -7, 7, 21])
    with pytest.raises(ValueError):                                         # d_eq is required
        rx.demod_frames_pilots(d, 1, 640, 640, None, d_data=o)
    with pytest.raises(ValueError):
        rx.demod_frames_pilots(d, 1, 320, 640, o, d_data=o)
    with pytest.raises(ValueError):                                         # soft outputs read out->data
        rx.demod_frames_pilots(d, 1, 640, 640, o, d_cpe=o, d_llr=o)
    assert "ofdm_rx_demod_frames_pilots" in om._lib.last_error()
    # no-ops
    keep = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    rx.pilot_track_frames(d, 0, 2, 120, 3, d_data=keep, stream=cur(torch))
    rx.pilot_track_frames(d, 1, 2, 120, 3, stream=cur(torch))
    rx.pilot_track_frames(d, 2, 0, 0, 3, d_data=keep, stream=cur(torch))
    cfo = torch.zeros(2, dtype=torch.float64, device="cuda")
    rx.pilot_track_frames(d, 2, 1, 60, 3, d_cfo=cfo, stream=cur(torch))                # one row per segment: no pair
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all()) and bool(torch.isnan(cfo).all())
    rx.set_pilots([])                                                       # cleared
    with pytest.raises(ValueError):
        rx.pilot_track_frames(d, 1, 2, 120, 3, d_data=o)


def test_output_beyond_4gib(om, torch):
    """64-point rows, 9.7 M of them: 4.66 GB in, 4.35 GB of data out; rows sampled across the array, one across 2^32 bytes"""
    N, mod, K = 64, "QPSK", 60
    locs = pilots_of(N)
    Kd = K - 4
    n_seg, rows = 3236, 3000
    total = n_seg * rows
    assert total * Kd * 8 > (1 << 32)
    torch.manual_seed(0)
    sym = torch.randn(total * K * 2, dtype=torch.float32, device="cuda") * 0.7
    data = torch.empty(total * Kd * 2, dtype=torch.float32, device="cuda")
    bits = torch.empty(total * Kd * 2 // 8, dtype=torch.uint8, device="cuda")
    cpe = torch.empty(total * 2, dtype=torch.float32, device="cuda")
    cfo = torch.empty(n_seg, dtype=torch.float64, device="cuda")
    rx = receiver(om, N, mod, locs)
    rx.pilot_track_frames(sym, n_seg, rows, rows * K, 3, pr.CPE, d_data=data, d_bits=bits, bits_mode=om.BITS_PACKED, d_cpe=cpe,
                          d_cfo=cfo, stream=cur(torch))
    torch.cuda.synchronize()
    cross = (1 << 32) // (Kd * 8)                                     # the row that holds byte 2^32 of data
    for r0 in (0, cross - 1, total // 2, total - 3):
        z = sym[r0 * K * 2:(r0 + 3) * K * 2].cpu().numpy().view(np.complex64).reshape(3, K)
        got = data[r0 * Kd * 2:(r0 + 3) * Kd * 2].cpu().numpy().view(np.complex64).reshape(3, Kd)
        ref = pr.track_rows(z, locs, 1.0, pr.CPE)
        assert relerr(got, ref["data"]) < TOL, r0
        assert relerr(cpe[r0 * 2:(r0 + 3) * 2].cpu().numpy().view(np.complex64), ref["cpe"]) < TOL, r0
        gb = bits[r0 * Kd * 2 // 8:(r0 + 3) * Kd * 2 // 8].cpu().numpy().reshape(3, -1)
        assert np.array_equal(gb, pack_msb(pr.hard_bits(got, mod).reshape(3, -1))), r0
    s = n_seg - 1
    z = sym[s * rows * K * 2:(s + 1) * rows * K * 2].cpu().numpy().view(np.complex64).reshape(rows, K)
    ref = pr.track_rows(z, locs, 1.0, pr.CPE)
    want = pr.cfo_estimate(ref["U"], ref["usable"], 3, N, 16)
    assert abs(cfo[s].item() - want) <= 1e-6 * abs(want) + 1e-9
    del sym, data, bits
    torch.cuda.empty_cache()


def test_graph_capture_equals_eager(om, torch):
    case = CASES[4]
    N, mod = case[0], case[1]
    cp, K = GEOM[N]
    locs = pilots_of(N)
    Kd = K - len(locs)
    iq, _ = frames_of(case)
    n, fl = iq.shape
    rx = receiver(om, N, mod, locs)
    nds = rx.data_symbols_per_frame(fl)
    rx.reserve(n)
    rx.reserve_pilots(n, nds)
    rx.reserve_soft(n, nds * Kd)
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    z = lambda m, dt=torch.float32: torch.zeros(m, dtype=dt, device="cuda")            # noqa: E731
    outs = dict(eq=z(n * nds * K * 2), tsr=z(n * 4, torch.int32), data=z(n * nds * Kd * 2), bits=z(n * nds * Kd * 4 // 8, torch.uint8),
                cpe=z(n * nds * 2), slope=z(n * nds), cfo=z(n, torch.float64), llr=z(n * nds * Kd * 4), sigma=z(n, torch.float64))
    s = torch.cuda.Stream()

    def call(stream):
        rx.demod_frames_pilots(d_iq, n, fl, fl, outs["eq"], mode=pr.CPE_SLOPE, d_data=outs["data"], d_bits=outs["bits"],
                               bits_mode=om.BITS_PACKED, d_cpe=outs["cpe"], d_slope=outs["slope"], d_cfo=outs["cfo"],
                               d_llr=outs["llr"], d_sigma=outs["sigma"], d_tsr=outs["tsr"], stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["sigma"] > 0).all()) and bool((eager["cfo"] > 0).all())
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
