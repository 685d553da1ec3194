"""The pilot-stage edge cases on the CPU (tests/pilot_cases.py): the geometry table reaches every path of pilot_track_kernel it
is meant to reach -- with the work split read out of csrc/ofdm_launch.hpp, so that a changed formula turns this file red instead
of quietly moving the coverage --, the planted rows satisfy on the fp64 restatement ALONE what the GPU test
(tests/test_gpu_pilot_edges.py) relies on, the inputs can see a wrong conjugate and a missing DC skip, and the spoiled rows are
the unusable ones."""
import os
import re

import numpy as np
import pytest

import pilot_cases as pc
import pilot_ref as pr
from conftest import ROOT, relerr

CSRC = os.path.join(ROOT, "lte-gnu-radio-code_amd", "csrc")
TOL = 1e-5                                                            # the GPU bar of the stage (tests/test_gpu_pilot_frames.py)
ROWS = 22                                                             # 3 segments of 7 rows and a call of one row
SLOPED = [g for g in pc.GEOMS if len(g[3]) >= 2]


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------ the work split of the sources
def test_work_split_restates_the_sources():
    hpp = source("ofdm_launch.hpp")
    assert re.search(r"inline int pilot_group_log2\(int Kd\) \{\s*int g = 1;\s*while \(g < 6 && \(1 << g\) < \(Kd \+ 1\) / 2\) \+\+g;\s*"
                     r"return g;\s*\}", hpp), "pilot_group_log2 changed: restate it in pilot_cases.group_log2"
    assert ("inline int pilot_rows_per_group(int K, int g_log2) { return std::max(1, 4096 / (K * 8 * (64 >> g_log2))); }" in hpp), \
        "pilot_rows_per_group changed: restate it in pilot_cases.rows_per_group"
    stages = source("capi_rx_stages.hip")
    assert "a.g_log2 = pilot_group_log2(a.Kd);" in stages and "a.rows_per_group = pilot_rows_per_group(a.K, a.g_log2);" in stages
    assert "a.Kd = d.Kd - h->n_pilots;" in stages                     # the group size follows the DATA entries of a row
    kern = source("rx_pilot.hip")
    assert "constexpr int UNR = 2;" in kern and "for (int q0 = 0; q0 < npairs; q0 += G * UNR)" in kern
    assert "for (int p0 = 0; p0 < a.n_pilots; p0 += G)" in kern
    assert [pc.group_log2(k) for k in (0, 1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 4096)] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6, 6]
    assert [pc.rows_per_group(k, 6) for k in (100, 152, 170, 171, 300)] == [5, 3, 3, 2, 1]


def test_table_reaches_every_path():
    d = [pc.describe(g) for g in pc.GEOMS]
    assert len(set(pc.geom_id(g) for g in pc.GEOMS)) == len(pc.GEOMS)
    assert {x["g_log2"] for x in d} == {1, 2, 3, 4, 5, 6}
    g64 = [x for x in d if x["G"] == 64]
    assert {x["rows_per_group"] for x in g64} >= {1, 3, 5}
    assert {x["nfft"] for x in d} >= {64, 128, 256, 512, 1024, 2048}
    many = [x for x in g64 if x["n_pilots"] > 64]
    assert any(x["pilot_trips"] == 4 and x["last_trip"] == 8 for x in many), "four pilot trips at G = 64, the last of 8"
    assert any(x["Kd"] == 0 for x in d) and any(x["Kd"] == 1 and x["n_pilots"] >= 2 for x in d) and any(x["n_pilots"] == 1 for x in d)
    assert any(x["load_batches"] == 3 for x in d) and any(x["load_batches"] == 2 for x in d)
    assert any(x["Kd"] % 4 == 2 and x["Kd"] * 4 % 8 == 0 for x in d), "16-QAM packed: the last even lane stores one byte"
    assert any(x["Kd"] % 2 == 1 for x in d), "an odd row: the last lane has one output"
    assert any(not x["symmetric"] and x["n_pilots"] >= 2 for x in d)
    # a geometry of every lane-group size can be tried with packed bits in some constellation
    for gl in range(1, 7):
        assert any(x["g_log2"] == gl and x["Kd"] and any(x["Kd"] * b % 8 == 0 for b in (2, 4, 6)) for x in d), gl
    nfft, cp, K, locs = pc.BY_ID["N1024-K600-p16_128"]
    assert K >= 600 and max(abs(x) for x in locs) <= K // 4
    # the rules of ofdm_rx_set_pilots
    for nfft, cp, K, locs in pc.GEOMS:
        assert K % 2 == 0 and 2 <= K <= nfft and len(set(locs)) == len(locs) <= K
        assert all(x != 0 and abs(x) <= K // 2 for x in locs)
    assert abs(pc.PVS[1]) != 1 and all(v.imag != 0 for v in pc.PVS)


# ------------------------------------------------------------------------------------------ planted rows on the reference alone
def combos(geom):
    """(constellation, mode, pilot value) of a geometry as the GPU test runs them: every constellation in every mode the
    pilot count allows, the pilot values in turn (each twice, each mode with all three where both modes run)"""
    modes = (pr.CPE, pr.CPE_SLOPE) if len(geom[3]) >= 2 else (pr.CPE,)
    return [(mod, mode, pc.PVS[i % 3]) for i, (mod, mode) in enumerate((a, b) for a in pc.MODS for b in modes)]


def band_edge(z, geom, pv, ref):
    """max |delta + tau k| over the data entries, delta and tau as the restatement measures them"""
    pidx, pk, didx, dk = pr.layout(geom[2], geom[3])
    if not len(dk):
        return 0.0, 0.0
    theta = np.angle(z[:, pidx].astype(np.complex128) * np.conj(pv) * np.conj(ref["cpe"])[:, None])
    delta = theta.mean(axis=1) - ref["slope"] * pk.mean()
    return float(np.max(np.abs(delta[:, None] + ref["slope"][:, None] * dk))), float(np.max(np.abs(theta)))


@pytest.mark.parametrize("geom", pc.GEOMS, ids=pc.geom_id)
def test_planted_rows_on_the_reference(geom):
    nfft, cp, K, locs = geom
    pidx, pk, didx, dk = pr.layout(K, locs)
    for mod, mode, pv in combos(geom):
        z, sym, bits, phi, tau = pc.planted_rows(geom, mod, pv, ROWS, seed=K + mode, mode=mode)
        assert z.dtype == np.complex64 and np.all(np.abs(phi) < np.pi)
        assert np.max(np.abs(z[:, pidx] * np.exp(-1j * (phi[:, None] + tau[:, None] * pk)) - pv)) < 1e-6 * abs(pv)
        ref = pr.track_rows(z, locs, pv, mode)
        assert ref["usable"].all()
        edge, theta = band_edge(z, geom, pv, ref)
        assert theta <= np.pi - 0.3, "theta wraps"
        if len(didx):
            assert relerr(ref["data"], sym) < 1e-6
            assert np.array_equal(pr.hard_bits(ref["data"], mod).reshape(ROWS, -1), bits)
        if pc.describe(geom)["symmetric"]:
            assert np.max(np.abs(ref["cpe"] - np.exp(1j * phi))) < 1e-6
        # the inputs see a wrong conjugate: in the data, or -- without data -- in cpe
        bad = pr.track_rows(z, locs, np.conj(pv), mode)
        what = "data" if len(didx) else "cpe"
        assert relerr(bad[what], ref[what]) > 1e-3, "a wrong conjugate would pass"
        emu = pc.emulate_f32(z, locs, pv, mode)
        figs = {k: relerr(emu[k], ref[k]) for k in (("data",) if len(didx) else ()) + ("cpe",)}
        if mode == pr.CPE_SLOPE:
            assert np.max(np.abs(tau)) == pc.tau_max(K, locs) > 0
            assert np.max(np.abs(ref["slope"] - tau)) <= 1e-6 * np.max(np.abs(tau))
            figs["slope"] = relerr(emu["slope"], ref["slope"])
            if len(didx):                                             # .. and a missing DC skip: k = i - K/2 for every list index i
                nodc = pr.track_rows(z, locs, pv, mode, data_offsets=didx - K // 2)
                assert relerr(nodc["data"], ref["data"]) > 1e-3, "a missing DC skip would pass"
        else:
            assert not tau.any()
        print("%s %s mode=%d: band edge %.2f rad, max|theta| %.2f, float32 emulation against fp64:" % (pc.geom_id(geom), mod, mode, edge, theta),
              {k: "%.2g" % v for k, v in figs.items()})
        assert max(figs.values()) < TOL / 4, "the float32 contract itself leaves no margin under the GPU bar"


def test_every_group_size_has_a_band_edge_past_pi():
    seen = {}
    for geom in SLOPED:
        nfft, cp, K, locs = geom
        for mod, mode, pv in combos(geom):
            if mode != pr.CPE_SLOPE or K == len(locs):
                continue
            z = pc.planted_rows(geom, mod, pv, ROWS, seed=K + mode, mode=mode)[0]
            edge = band_edge(z, geom, pv, pr.track_rows(z, locs, pv, mode))[0]
            gl = pc.describe(geom)["g_log2"]
            seen[gl] = max(seen.get(gl, 0.0), edge)
    assert sorted(seen) == [1, 2, 3, 4, 5, 6] and all(v > np.pi for v in seen.values()), seen
    assert max(seen.values()) > 1.5 * np.pi                          # more than three quarters of a revolution somewhere


# ------------------------------------------------------------------------------------------ rows without a usable U
@pytest.mark.parametrize("geom", [pc.BY_ID[i] for i in ("N64-K2-p1_1", "N64-K8-p2_1", "N64-K60-p4_21", "N128-K100-p8_40", "N256-K152-p8_60",
                                                        "N2048-K1200-p200_600", "N64-K60-p60_30")], ids=pc.geom_id)
def test_unusable_rows_are_the_planted_ones(geom):
    nfft, cp, K, locs = geom
    pidx, pk, didx, dk = pr.layout(K, locs)
    rows = 130
    for seed, pv in enumerate(pc.PVS):
        z, plain, kinds = pc.unusable_rows(geom, rows, seed, pv, phase_step=0.9)
        assert set(kinds.values()) == set(pc.KINDS) and {0, 63, 64, 65, rows - 1} <= set(kinds)
        d = pc.describe(geom)
        if d["rows_per_group"] > 1:
            assert any(r % d["rows_per_group"] == d["rows_per_group"] // 2 and r - 1 not in kinds and r + 1 not in kinds for r in kinds)
        else:
            assert any(0 < r < rows - 1 and r - 1 not in kinds and r + 1 not in kinds for r in kinds)
        spoiled = np.zeros(rows, bool)
        spoiled[list(kinds)] = True
        assert np.array_equal(z[~spoiled], plain[~spoiled]) and np.array_equal(z[:, didx], plain[:, didx]) and np.isfinite(z[:, didx]).all()
        for mode in ((pr.CPE, pr.CPE_SLOPE) if len(locs) >= 2 else (pr.CPE,)):
            ref = pr.track_rows(z, locs, pv, mode)
            assert np.array_equal(ref["usable"], ~spoiled), (kinds, np.nonzero(ref["usable"] == spoiled)[0])
            assert pr.track_rows(plain, locs, pv, mode)["usable"].all()
            assert np.array_equal(ref["data"][spoiled], z[spoiled][:, didx]) and not ref["cpe"][spoiled].any() and not ref["slope"][spoiled].any()
            assert np.isfinite(ref["data"]).all() and np.isfinite(ref["cpe"]).all() and np.isfinite(ref["U"]).all()
        # cfo: the pairs with a spoiled row are skipped -- the estimate is the one of the usable pairs alone, and finite
        ref = pr.track_rows(z, locs, pv)
        full = pr.track_rows(plain, locs, pv)
        for rpp in (2, 5, rows):
            got = pr.cfo_estimate(ref["U"], ref["usable"], rpp, nfft, cp)
            want = pr.cfo_estimate(full["U"], ~spoiled, rpp, nfft, cp)
            assert np.isfinite(got) and got == want
            assert abs(got - 0.9 / (2 * np.pi * (nfft + cp) / nfft)) < 0.02          # the planted step per row
        assert np.isnan(pr.cfo_estimate(ref["U"], ref["usable"], 1, nfft, cp))


def test_usable_is_decided_in_float32():
    """|U| = 1e25 and 1e-30 are ordinary numbers in fp64; the contract squares in float32"""
    locs = [-21, -7, 7, 21]
    z = np.ones((4, 60), np.complex64)
    z[1, pr.layout(60, locs)[0]] = 1e25
    z[2, pr.layout(60, locs)[0]] = 1e-30
    z[3, pr.layout(60, locs)[0]] = 1e-15                              # |U|^2 = 1.6e-29: small, and usable
    r = pr.track_rows(z, locs)
    assert r["usable"].tolist() == [True, False, False, True]
    assert np.array_equal(r["data"][1], z[1, pr.layout(60, locs)[2]]) and r["cpe"][1] == 0 and r["U"][2] == 0
    assert abs(r["cpe"][3] - 1) < 1e-12


# ------------------------------------------------------------------------------------------ the end-to-end frames
@pytest.mark.parametrize("case", pc.E2E, ids=lambda c: "%d-%s" % (c[0], c[4]))
def test_e2e_frames_on_the_reference(case):
    """On rows of the fp64 receiver: tracked bits are the transmitted bits in slope mode (and at twice the noise), not with the
    conjugate pilot value on the receiver, not in CPE mode (the slope stays in), and the slope returned is the planted one."""
    nfft, cp, K, locs, mod, eps, noise = case
    iq, bits = pc.e2e_frames(case)
    for f in range(pc.E2E_FRAMES):
        z = pr.oracle_rows(iq[f], nfft, cp, K, pc.E2E_SYM)
        assert z.shape == (12, K) and z.any(axis=1).all()
        r = pr.track_rows(z, locs, pc.E2E_PV, pr.CPE_SLOPE)
        assert np.array_equal(pr.hard_bits(r["data"], mod), bits[f])
        assert np.max(np.abs(r["slope"])) > 0.9 * 2 * np.pi / nfft
        wrong = pr.track_rows(z, locs, np.conj(pc.E2E_PV), pr.CPE_SLOPE)
        assert (pr.hard_bits(wrong["data"], mod) != bits[f]).mean() > 0.2
        assert (pr.hard_bits(pr.track_rows(z, locs, pc.E2E_PV)["data"], mod) != bits[f]).mean() > 0.05
    loud, lbits = pr.make_frame(nfft, cp, K, locs, mod, pc.E2E_SYM, eps, 2 * noise, seed=11, pilot_value=pc.E2E_PV,
                                row_slope=np.linspace(-1, 1, 12) * 2 * np.pi / nfft)
    r = pr.track_rows(pr.oracle_rows(loud, nfft, cp, K, pc.E2E_SYM), locs, pc.E2E_PV, pr.CPE_SLOPE)
    assert np.array_equal(pr.hard_bits(r["data"], mod), lbits)
