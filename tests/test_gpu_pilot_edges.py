"""The edges of the pilot-aided phase-tracking stage on the GPU (-m gpu): complex pilot values, every lane-group size of
pilot_track_kernel, more pilots than lanes, planted rotations of several radians at the band edge, rows without a usable pilot
sum, the cfo kernel's lane loop and pattern seams, bits at unaligned bases, and a one-sample timing error end to end.

The inputs are tests/pilot_cases.py; what they satisfy on the fp64 restatement alone is asserted in
tests/test_pilot_cases_host.py (no theta wraps, a band edge past pi in every lane-group class, a wrong conjugate or a missing DC
skip moves the data by more than 1e-3).  The bar is the stage's TOL = 1e-5 of tests/test_gpu_pilot_frames.py; the float32
emulation of the contract (pilot_cases.emulate_f32) is within 1.6e-6 of fp64 on every planted case, and so is the device
(data <= 1.5e-6, cpe <= 1.6e-6, slope <= 3.1e-7 on an MI355X: profiles/pilot_edges_gpu.txt)."""
import numpy as np
import pytest

import pilot_cases as pc
import pilot_ref as pr
from conftest import relerr
from test_gpu_pilot_frames import BPS, TOL, cur, om, pack_msb, same_bits, stage, torch  # noqa: F401  (om, torch: fixtures)
from test_pilot_cases_host import ROWS, combos

pytestmark = pytest.mark.gpu

N_SYM = 16
G_BY_ID = pc.BY_ID


def engine(om, geom, mod):
    nfft, cp, K, locs = geom
    rx = om.RxEngine(N_SYM, nfft, cp, nfft - 2, (1, 3), K, 100, 0.7, modulation=mod)
    rx.set_max_trials(0)
    return rx


def dev(torch, z):
    return torch.from_numpy(np.ascontiguousarray(z).view(np.float32).ravel()).cuda()


def stage_at(om, torch, rx, d_sym, n_seg, rows, stride, K, n_p, mod, mode, bits_mode, rpp=3, data_off=0, bits_off=0):
    """stage() of tests/test_gpu_pilot_frames.py with the bits at any byte offset and rows without data (Kd' = 0): poisoned
    outputs, guards on BOTH sides of data and bits."""
    Kd, bps = K - n_p, BPS[mod]
    nb = n_seg * rows * Kd * bps // (8 if bits_mode == om.BITS_PACKED else 1)
    data = torch.full((n_seg * rows * Kd * 2 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    bits = torch.full((nb + 16,), 255, dtype=torch.uint8, device="cuda")
    cpe = torch.full((n_seg * rows * 2 + 2,), float("nan"), dtype=torch.float32, device="cuda")
    slope = torch.full((n_seg * rows + 1,), float("nan"), dtype=torch.float32, device="cuda")
    cfo = torch.full((n_seg + 1,), 7.0, dtype=torch.float64, device="cuda")
    rx.pilot_track_frames(d_sym, n_seg, rows, stride, rpp, mode, d_data=data.data_ptr() + data_off, d_bits=bits.data_ptr() + bits_off,
                          bits_mode=bits_mode, d_cpe=cpe, d_slope=slope if mode == pr.CPE_SLOPE else None, d_cfo=cfo, stream=cur(torch))
    torch.cuda.synchronize()
    hd, hb, hc, hs, hf = (t.cpu().numpy() for t in (data, bits, cpe, slope, cfo))
    k = data_off // 4
    assert np.isnan(hd[:k]).all() and np.isnan(hd[k + n_seg * rows * Kd * 2:]).all(), "wrote outside data"
    assert (hb[:bits_off] == 255).all() and (hb[bits_off + nb:] == 255).all(), "wrote outside bits"
    assert np.isnan(hc[-2:]).all() and np.isnan(hs[-1]) and hf[-1] == 7.0, "wrote outside cpe / slope / cfo"
    if mode != pr.CPE_SLOPE:
        assert np.isnan(hs).all(), "slope written in CPE mode"
    return dict(data=hd[k:k + n_seg * rows * Kd * 2].view(np.complex64).reshape(n_seg, rows, Kd),
                bits=hb[bits_off:bits_off + nb].reshape(n_seg, rows, nb // (n_seg * rows)),
                cpe=hc[:-2].view(np.complex64).reshape(n_seg, rows), slope=hs[:-1].reshape(n_seg, rows), cfo=hf[:-1])


# ------------------------------------------------------------------------------------------ 1 + 2: geometry x mode x pilot value
@pytest.mark.parametrize("geom", pc.GEOMS, ids=pc.geom_id)
def test_planted_rotation_every_geometry(om, torch, geom):
    """3 segments of 7 rows, then one segment of one row (one lane group of the wave has a row, the others none): data, cpe and
    slope against the restatement, bits against the stored data AND the planted bits, slope and cpe against what was planted.
    Every constellation one bit per byte, and packed wherever Kd' bps % 8 == 0."""
    nfft, cp, K, locs = geom
    d = pc.describe(geom)
    Kd, n_p = d["Kd"], len(locs)
    for mod, mode, pv in combos(geom):
        rx = engine(om, geom, mod)
        rx.set_pilots(locs, pv)
        z, sym, bits, phi, tau = pc.planted_rows(geom, mod, pv, ROWS, seed=K + mode, mode=mode)
        ref = pr.track_rows(z, locs, pv, mode)
        d_z = dev(torch, z)
        layouts = [om.BITS_UNPACKED] + ([om.BITS_PACKED] if Kd and Kd * BPS[mod] % 8 == 0 else [])
        for bm in layouts:
            a = stage_at(om, torch, rx, d_z, 3, 7, 7 * K, K, n_p, mod, mode, bm)
            b = stage_at(om, torch, rx, d_z.data_ptr() + 21 * K * 8, 1, 1, K, K, n_p, mod, mode, bm)
            got = {k: np.concatenate([a[k].reshape((21,) + a[k].shape[2:]), b[k].reshape((1,) + b[k].shape[2:])]) for k in ("data", "bits", "cpe", "slope")}
            figs = dict(cpe=relerr(got["cpe"], ref["cpe"]))
            if d["symmetric"]:
                figs["cpe_planted"] = float(np.max(np.abs(got["cpe"] - np.exp(1j * phi))))
            if Kd:
                figs["data"] = relerr(got["data"], ref["data"])
            if mode == pr.CPE_SLOPE:
                figs["slope"] = relerr(got["slope"], ref["slope"])
                figs["slope_planted"] = float(np.max(np.abs(got["slope"] - tau)) / np.max(np.abs(tau)))
            print("pilot edges %s G=%d %s mode=%d pv=%s bits=%d:" % (pc.geom_id(geom), d["G"], mod, mode, pv, bm), {k: "%.3g" % v for k, v in figs.items()})
            assert max(figs.values()) < TOL, figs
            assert np.isfinite(got["cpe"]).all() and np.isnan(b["cfo"]).all()            # one row: no pair
            if not Kd:
                assert got["bits"].size == 0 and got["data"].size == 0                     # stage_at saw both buffers all poison
                continue
            hb = pr.hard_bits(got["data"], mod).reshape(ROWS, Kd * BPS[mod])
            assert np.array_equal(hb, bits), "stored data do not de-map to the planted bits: %d errors" % int((hb != bits).sum())
            assert np.array_equal(got["bits"], pack_msb(hb) if bm == om.BITS_PACKED else hb), "bits differ from the hard decision of the stored data"


# ------------------------------------------------------------------------------------------ 2: bits and data at unaligned bases
@pytest.mark.parametrize("gid", ["N64-K8-p2_1", "N64-K16-p2_5", "N64-K60-p4_21", "N128-K100-p8_40", "N2048-K1200-p200_600", "N64-K60-p59_30"])
def test_unaligned_bits_and_data(om, torch, gid):
    """one bit per byte with d_bits 1, 2 and 3 bytes past a 4-byte boundary and the data 8 bytes off the 16-byte grid: the same
    bytes as the aligned call"""
    geom = G_BY_ID[gid]
    nfft, cp, K, locs = geom
    for i, mod in enumerate(pc.MODS):
        pv, mode = pc.PVS[i], pr.CPE_SLOPE
        rx = engine(om, geom, mod)
        rx.set_pilots(locs, pv)
        z, sym, bits, _, _ = pc.planted_rows(geom, mod, pv, ROWS - 1, seed=3 + i, mode=mode)
        d_z = dev(torch, z)
        base = stage_at(om, torch, rx, d_z, 3, 7, 7 * K, K, len(locs), mod, mode, om.BITS_UNPACKED)
        assert np.array_equal(base["bits"].reshape(ROWS - 1, -1), bits)
        whole = stage(om, torch, rx, d_z, 3, 7, 7 * K, K, len(locs), mod, mode, om.BITS_UNPACKED)   # the existing harness agrees
        same_bits(base, whole, "stage()")
        for off in (1, 2, 3):
            for data_off in (0, 8):
                moved = stage_at(om, torch, rx, d_z, 3, 7, 7 * K, K, len(locs), mod, mode, om.BITS_UNPACKED, data_off=data_off, bits_off=off)
                same_bits(base, moved, "bits at +%d, data at +%d" % (off, data_off))


# ------------------------------------------------------------------------------------------ 3: rows without a usable U
@pytest.mark.parametrize("mode", [pr.CPE, pr.CPE_SLOPE])
@pytest.mark.parametrize("gid", ["N64-K8-p2_1", "N64-K60-p4_21", "N128-K100-p8_40", "N256-K152-p8_60", "N2048-K1200-p200_600",
                                 "N64-K60-p60_30"])
def test_unusable_rows(om, torch, gid, mode):
    """NaN, +-Inf, cancelling, overflowing and underflowing pilot entries in the first and last row, at the cfo kernel's lane
    seam (s = 63, 64, 65), in the middle of a lane group's walk: those rows are copied (c = 1), cpe 0, slope 0; every other row
    is the same bits as without them; the cfo sum skips them.  The last geometry has no data entries: cpe and cfo alone."""
    geom = G_BY_ID[gid]
    nfft, cp, K, locs = geom
    mod, pv, rows = "16QAM", pc.PVS[mode], 130
    pidx, pk, didx, dk = pr.layout(K, locs)
    z, plain, kinds = pc.unusable_rows(geom, rows, seed=mode, pilot_value=pv, phase_step=0.9)
    spoiled = np.zeros(rows, bool)
    spoiled[list(kinds)] = True
    rx = engine(om, geom, mod)
    rx.set_pilots(locs, pv)
    got = stage_at(om, torch, rx, dev(torch, z), 1, rows, rows * K, K, len(locs), mod, mode, om.BITS_UNPACKED, rpp=5)
    clean = stage_at(om, torch, rx, dev(torch, plain), 1, rows, rows * K, K, len(locs), mod, mode, om.BITS_UNPACKED, rpp=5)
    g = {k: got[k][0] for k in ("data", "bits", "cpe", "slope")}
    assert np.array_equal(g["data"][spoiled], z[spoiled][:, didx]), "an unusable row is copied: c = 1"
    assert not g["cpe"][spoiled].any() and (mode == pr.CPE or not g["slope"][spoiled].any())
    if len(didx):
        assert np.array_equal(g["bits"][spoiled], pr.hard_bits(z[spoiled][:, didx], mod).reshape(int(spoiled.sum()), -1))
    for k in ("data", "bits", "cpe") + (("slope",) if mode == pr.CPE_SLOPE else ()):
        assert np.array_equal(np.ascontiguousarray(g[k][~spoiled]).view(np.uint8), np.ascontiguousarray(clean[k][0][~spoiled]).view(np.uint8)), \
            "%s of a usable row depends on an unusable one" % k
        assert np.isfinite(g[k].astype(np.complex128)).all(), "%s: a non-finite value in a row whose data were finite" % k
    ref = pr.track_rows(z, locs, pv, mode)
    assert np.array_equal(ref["usable"], ~spoiled)
    assert relerr(g["data"], ref["data"]) < TOL and relerr(g["cpe"], ref["cpe"]) < TOL
    if mode == pr.CPE_SLOPE:
        assert relerr(g["slope"], ref["slope"]) < TOL
    want = pr.cfo_estimate(ref["U"], ref["usable"], 5, nfft, cp)
    assert abs(got["cfo"][0] - want) <= 1e-6 * abs(want) + 1e-9, (got["cfo"][0], want)
    assert got["cfo"][0] != clean["cfo"][0]


# ------------------------------------------------------------------------------------------ 4: the cfo kernel's geometry
@pytest.mark.parametrize("rows", [130, 65])
def test_cfo_geometry(om, torch, rows):
    """the lane loop (s += 64) and its seam, rows_per_pattern 1 (no pair: NaN), 2, 5 and `rows`; segment 0 has unusable rows at
    s = 63, 64, 65 (rows 63 and 64 close patterns of 2 and 5 as well), segment 1 has every pair broken (NaN), segment 2 is whole"""
    geom = G_BY_ID["N64-K60-p4_21"]
    nfft, cp, K, locs = geom
    pv, mod = pc.PVS[0], "QPSK"
    pidx = pr.layout(K, locs)[0]
    last = [63, 64] if rows == 65 else [63, 64, 65, 127]
    z0 = pc.unusable_rows(geom, rows, 1, pv, phase_step=0.9, chosen=last)[0]
    z1 = pc.unusable_rows(geom, rows, 2, pv, phase_step=0.9, chosen=list(range(1, rows, 2)))[0]
    z2 = pc.random_rows(np.random.default_rng(3), rows, K, locs, pv, phase_step=-1.3)
    z = np.stack([z0, z1, z2])
    ref = pr.track_rows(z, locs, pv)
    assert ref["usable"][2].all() and not ref["usable"][0][last].any() and ref["usable"][0].sum() == rows - len(last)
    rx = engine(om, geom, mod)
    rx.set_pilots(locs, pv)
    d_z = dev(torch, z)
    for rpp in (1, 2, 5, rows):
        got = stage(om, torch, rx, d_z, 3, rows, rows * K, K, len(locs), mod, pr.CPE, om.BITS_UNPACKED, rpp=rpp)
        alone = stage(om, torch, rx, d_z.data_ptr() + 2 * rows * K * 8, 1, rows, rows * K, K, len(locs), mod, pr.CPE, om.BITS_UNPACKED, rpp=rpp)
        assert got["cfo"][2:].tobytes() == alone["cfo"].tobytes(), "a whole segment's cfo depends on its neighbours"
        for s in range(3):
            want = pr.cfo_estimate(ref["U"][s], ref["usable"][s], rpp, nfft, cp)
            print("cfo rows=%d rpp=%d segment %d: got %.12g want %.12g" % (rows, rpp, s, got["cfo"][s], want))
            if rpp == 1 or s == 1:
                assert np.isnan(want) and np.isnan(got["cfo"][s]), (rpp, s, got["cfo"][s])
            else:
                assert abs(got["cfo"][s] - want) <= 1e-6 * abs(want) + 1e-9, (rpp, s, got["cfo"][s], want)
    full = pr.cfo_estimate(ref["U"][2], ref["usable"][2], rows, nfft, cp)
    assert abs(full + 1.3 / (2 * np.pi * (nfft + cp) / nfft)) < 0.01                         # the planted step


# ------------------------------------------------------------------------------------------ 5: alone, batched, strided, repeated
@pytest.mark.parametrize("gid,mod,mode", [("N64-K8-p2_1", "16QAM", pr.CPE_SLOPE), ("N128-K100-p8_40", "QPSK", pr.CPE),
                                          ("N128-K100-p8_40", "16QAM", pr.CPE_SLOPE), ("N2048-K1200-p200_600", "64QAM", pr.CPE_SLOPE)])
def test_edge_geometries_alone_in_batch_strided_and_repeated(om, torch, gid, mod, mode):
    """the determinism sentence of the header at a small lane group, at G = 64 with a walk of 5 rows (13 rows per segment: a
    walk crosses segments) and with 200 pilots"""
    geom = G_BY_ID[gid]
    nfft, cp, K, locs = geom
    pv, n_p = pc.PVS[1], len(locs)
    rng = np.random.default_rng(K + mode)
    n_seg, rows = 9, 13
    stride = rows * K + 5                                             # odd stride: segments 1, 3, .. start 8 bytes off the 16-byte grid
    host = np.zeros((n_seg, stride), np.complex64)
    host[:, :rows * K] = pc.random_rows(rng, n_seg * rows, K, locs, pv).reshape(n_seg, rows * K)
    rx = engine(om, geom, mod)
    rx.set_pilots(locs, pv)
    d = dev(torch, host)
    bm = om.BITS_PACKED
    b1 = stage(om, torch, rx, d, n_seg, rows, stride, K, n_p, mod, mode, bm)
    b2 = stage(om, torch, rx, d, n_seg, rows, stride, K, n_p, mod, mode, bm)
    same_bits(b1, b2, "second call")
    dense = dev(torch, host[:, :rows * K])
    same_bits(b1, stage(om, torch, rx, dense, n_seg, rows, rows * K, K, n_p, mod, mode, bm), "dense layout")
    for s in (0, 4, 8):
        alone = stage(om, torch, rx, d.data_ptr() + 8 * s * stride, 1, rows, stride, K, n_p, mod, mode, bm)
        same_bits({k: v[s:s + 1] for k, v in b1.items()}, alone, "segment %d alone" % s)
        shifted = stage(om, torch, rx, d.data_ptr() + 8 * s * stride, 1, rows, stride, K, n_p, mod, mode, bm, data_off=8)
        same_bits(alone, shifted, "output 8 bytes off the 16-byte grid")
    ref = pr.track_rows(host[:, :rows * K].reshape(n_seg, rows, K), locs, pv, mode)
    assert relerr(b1["data"], ref["data"]) < TOL and relerr(b1["cpe"], ref["cpe"]) < TOL
    if mode == pr.CPE_SLOPE:
        assert relerr(b1["slope"], ref["slope"]) < TOL
    hb = pr.hard_bits(b1["data"], mod).reshape(n_seg, rows, -1)
    assert np.array_equal(b1["bits"], pack_msb(hb))
    u = stage(om, torch, rx, d, n_seg, rows, stride, K, n_p, mod, mode, om.BITS_UNPACKED)
    assert np.array_equal(u["bits"], hb) and np.array_equal(u["data"].view(np.uint8), b1["data"].view(np.uint8))


# ------------------------------------------------------------------------------------------ 6: end to end, a timing error
@pytest.mark.parametrize("case", pc.E2E, ids=lambda c: "%d-%s" % (c[0], c[4]))
def test_timing_error_end_to_end(om, case):
    """demod_frames_pilots on frames with the pilot value 0.6 - 0.8j whose rows carry a slope of up to a one-sample timing error:
    tracked bits are the transmitted bits, parity with the restatement on the same call's d_eq, and the conjugate pilot value on
    the receiver loses the bits"""
    nfft, cp, K, locs, mod, eps, noise = case
    Kd, bps = K - len(locs), BPS[mod]
    iq, tx_bits = pc.e2e_frames(case)
    n, fl = iq.shape
    rx = engine(om, (nfft, cp, K, locs), mod)
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    nds = rx.data_symbols_per_frame(fl)
    assert nds == 12

    def run(pv):
        rx.set_pilots(locs, pv)
        d = dict(eq=om.DeviceBuffer(n * nds * K * 8), tsr=om.DeviceBuffer(n * 16), data=om.DeviceBuffer(n * nds * Kd * 8),
                 bits=om.DeviceBuffer(n * nds * Kd * bps), cpe=om.DeviceBuffer(n * nds * 8), slope=om.DeviceBuffer(n * nds * 4),
                 cfo=om.DeviceBuffer(n * 8))
        r = rx.demod_frames_pilots(d_iq, n, fl, fl, d["eq"], mode=pr.CPE_SLOPE, d_data=d["data"], d_bits=d["bits"], bits_mode=om.BITS_UNPACKED,
                                   d_cpe=d["cpe"], d_slope=d["slope"], d_cfo=d["cfo"], d_tsr=d["tsr"])
        assert r == nds
        return dict(eq=d["eq"].download(np.complex64, n * nds * K).reshape(n, nds, K), tsr=d["tsr"].download(np.int32, n * 4).reshape(n, 4),
                    data=d["data"].download(np.complex64, n * nds * Kd).reshape(n, nds, Kd),
                    bits=d["bits"].download(np.uint8, n * nds * Kd * bps).reshape(n, nds * Kd * bps),
                    cpe=d["cpe"].download(np.complex64, n * nds).reshape(n, nds), slope=d["slope"].download(np.float32, n * nds).reshape(n, nds),
                    cfo=d["cfo"].download(np.float64, n))

    res = run(pc.E2E_PV)
    assert res["tsr"][:, 3].all() and res["eq"].any(axis=2).all(), "both frames synchronise and no row is left out"
    ref = pr.track_rows(res["eq"], locs, pc.E2E_PV, pr.CPE_SLOPE)
    figs = {k: relerr(res[k], ref[k]) for k in ("data", "cpe", "slope")}
    print("pilot edges end to end N=%d %s:" % (nfft, mod), {k: "%.3g" % v for k, v in figs.items()}, "max |slope| N / 2 pi = %.3f" % (
        np.max(np.abs(res["slope"])) * nfft / (2 * np.pi)))
    assert max(figs.values()) < TOL, figs
    for f in range(n):
        want = pr.cfo_estimate(ref["U"][f], ref["usable"][f], 3, nfft, cp)
        assert abs(res["cfo"][f] - want) <= 1e-6 * abs(want) + 1e-9, (f, res["cfo"][f], want)
    assert np.array_equal(res["bits"], pr.hard_bits(res["data"], mod).reshape(n, -1))
    assert np.array_equal(res["bits"], tx_bits), "tracked bits differ from the transmitted bits: %d errors" % int((res["bits"] != tx_bits).sum())
    assert np.max(np.abs(res["slope"])) > 0.9 * 2 * np.pi / nfft
    wrong = run(np.conj(pc.E2E_PV))
    assert np.array_equal(wrong["eq"].view(np.uint8), res["eq"].view(np.uint8))
    assert (wrong["bits"] != tx_bits).mean() > 0.2, "the case cannot see a wrong conjugate"
