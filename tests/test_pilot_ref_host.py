"""The pilot tracking stage without a GPU: the fp64 restatement (tests/pilot_ref.py) on rows of the fp64 receiver oracle, and the
C ABI of the stage (symbols, struct layout, argument errors that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pilot_ref as pr
from conftest import ROOT
from oracle import ofdm_oracle as orc

NEW = ("ofdm_rx_set_pilots", "ofdm_rx_reserve_pilots", "ofdm_pilot_track_frames", "ofdm_rx_demod_frames_pilots")
N, CP, K, LOCS = 64, 16, 60, [-21, -7, 7, 21]


def rows_of(mod="QPSK", n_sym=16, eps=0.0, noise=0.0, seed=3, **kw):
    iq, bits = pr.make_frame(N, CP, K, LOCS, mod, n_sym, eps, noise, seed, **kw)
    return pr.oracle_rows(iq, N, CP, K, n_sym), bits


def test_layout_is_the_transmitters_grid():
    """the data entries of a received row are the transmitter's symbols in order; the pilot entries carry the pilot value"""
    pidx, pk, didx, dk = pr.layout(K, LOCS)
    assert pk.tolist() == sorted(LOCS) and len(didx) == K - 4
    sym = (np.arange(K - 4) + 1) * (1 + 0.5j)
    grid = orc.tx_stage_grid(sym, N, K - 4, LOCS, 2 - 1j)[0]
    row = grid[orc.bins_p(K, N)]
    assert np.array_equal(row[didx], sym) and np.all(row[pidx] == 2 - 1j)


def test_no_offset_no_noise_changes_nothing():
    z, bits = rows_of("16QAM")
    r = pr.track_rows(z, LOCS)
    assert r["usable"].all() and np.max(np.abs(r["cpe"] - 1)) < 1e-12
    _, _, didx, _ = pr.layout(K, LOCS)
    assert np.max(np.abs(r["data"] - z[:, didx])) < 1e-12
    assert np.array_equal(pr.hard_bits(r["data"], "16QAM"), bits)


def test_known_rotation_per_row_is_measured_and_removed():
    n_data = 12
    phi = np.linspace(-3.0, 3.0, n_data)
    z0, bits = rows_of("16QAM")
    z1, _ = rows_of("16QAM", row_phase=phi)
    r = pr.track_rows(z1, LOCS)
    assert np.max(np.abs(r["cpe"] - np.exp(1j * phi))) < 1e-9
    _, _, didx, _ = pr.layout(K, LOCS)
    assert np.max(np.abs(r["data"] - z0[:, didx])) < 1e-9
    assert np.array_equal(pr.hard_bits(r["data"], "16QAM"), bits)
    # a pilot value other than 1 measures the same rotation
    z2, _ = rows_of("16QAM", row_phase=phi, pilot_value=0.6 - 0.8j)
    assert np.max(np.abs(pr.track_rows(z2, LOCS, 0.6 - 0.8j)["cpe"] - np.exp(1j * phi))) < 1e-9


def test_known_slope_is_measured_and_removed():
    n_data = 12
    tau = np.linspace(-0.02, 0.03, n_data)                         # radians per bin; |tau k| < 1 rad over the 30 bins a side
    phi = np.linspace(1.0, -2.0, n_data)
    z0, bits = rows_of("64QAM")
    z1, _ = rows_of("64QAM", row_phase=phi, row_slope=tau)
    r = pr.track_rows(z1, LOCS, mode=pr.CPE_SLOPE)
    assert np.max(np.abs(r["slope"] - tau)) < 1e-9
    _, _, didx, _ = pr.layout(K, LOCS)
    assert np.max(np.abs(r["data"] - z0[:, didx])) < 1e-9
    assert np.array_equal(pr.hard_bits(r["data"], "64QAM"), bits)
    # CPE alone leaves the slope in: the outer bins are off by tau * 30
    assert np.max(np.abs(pr.track_rows(z1, LOCS)["data"] - z0[:, didx])) > 0.1


def test_rows_without_a_usable_pilot_sum():
    z, _ = rows_of()
    z[2] = 0
    z[5, pr.layout(K, LOCS)[0]] = [1, -1, 1j, -1j]                  # pilots cancel: U = 0
    for mode in (pr.CPE, pr.CPE_SLOPE):
        r = pr.track_rows(z, LOCS, mode=mode)
        assert not r["usable"][[2, 5]].any() and r["usable"].sum() == len(z) - 2
        assert not r["data"][2].any() and r["cpe"][2] == 0 and r["cpe"][5] == 0 and r["slope"][5] == 0
        assert np.array_equal(r["data"][5], z[5, pr.layout(K, LOCS)[2]])           # c = 1: not rotated
    r = pr.track_rows(z, LOCS)
    assert np.isfinite(pr.cfo_estimate(r["U"], r["usable"], 3, N, CP))
    assert np.isnan(pr.cfo_estimate(r["U"][:1], r["usable"][:1], 3, N, CP))
    assert np.isnan(pr.cfo_estimate(r["U"], r["usable"], 1, N, CP))              # one row per pattern: no pair


# (N, cp, K, pilots, constellation, eps, noise) -> measured max |cfo - eps| over the seeds 1, 2, 3 (240 symbols, fp64 path)
CFO_CASES = [
    ((64, 16, 60, LOCS, "QPSK", 0.01, 0.02), 2.7e-4),
    ((64, 16, 60, LOCS, "16QAM", 0.005, 0.005), 6.4e-5),
    ((64, 16, 60, LOCS, "QPSK", 0.0, 0.02), 1.0e-4),
    ((1024, 72, 600, [s * 37 * m for m in range(1, 8) for s in (-1, 1)], "16QAM", 0.01, 0.01), 6.9e-5),
]


@pytest.mark.parametrize("case,measured", CFO_CASES, ids=lambda c: "-".join(str(x) for x in (c[0], c[4], c[5])) if isinstance(c, tuple) else None)
def test_cfo_returns_the_injected_offset(case, measured):
    """The estimate is noise- and ICI-limited, not arithmetic: its error on the fp64 path was measured for these seeds and noise
    levels (the figure beside each case: the largest |cfo - eps| of seeds 1, 2, 3) and the assertion is three times that.
    Tracked bits are the transmitted bits in every case."""
    n, cp, k, locs, mod, eps, noise = case
    worst = 0.0
    for seed in (1, 2, 3):
        iq, bits = pr.make_frame(n, cp, k, locs, mod, 240, eps, noise, seed)
        z = pr.oracle_rows(iq, n, cp, k, 240)
        assert z.any(axis=1).all()
        r = pr.track_rows(z, locs)
        assert np.array_equal(pr.hard_bits(r["data"], mod), bits)
        est = pr.cfo_estimate(r["U"], r["usable"], 3, n, cp)
        worst = max(worst, abs(est - eps))
    print("cfo error, worst of three seeds: %.3g (recorded %.3g)" % (worst, measured))
    assert worst <= 3 * measured


# ------------------------------------------------------------------------------------------ C ABI without a device
def _lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load(), L


def test_pilot_symbols_are_exported_and_bound():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.PROTOTYPES
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(ofdm_[a-z0-9_]+)\s*\(", code)) <= set(L.PROTOTYPES)
    assert lib.ofdm_abi_version() == 1
    assert (L.PILOT_CPE, L.PILOT_CPE_SLOPE) == (0, 1) and re.search(r"OFDM_PILOT_CPE = 0, OFDM_PILOT_CPE_SLOPE = 1", hdr)


def test_pilot_out_struct_matches_the_header():
    _, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    body = re.search(r"typedef struct ofdm_pilot_out \{(.*?)\} ofdm_pilot_out;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in L.PilotOut._fields_] == ["data", "bits", "bits_mode", "cpe", "slope", "cfo"]
    assert C.sizeof(L.PilotOut) == 6 * C.sizeof(C.c_void_p)


def test_argument_errors_need_no_device():
    """A null handle is rejected by name; what the arguments alone decide is checked before the handle is read, so a stand-in
    handle that is never dereferenced is enough."""
    lib, L = _lib()
    buf = (C.c_float * 64)()
    loc = (C.c_int32 * 4)(-21, -7, 7, 21)
    out = L.PilotOut()
    out.data = C.addressof(buf)
    for call, name in ((lambda: lib.ofdm_rx_set_pilots(None, loc, 4, 1.0, 0.0), "ofdm_rx_set_pilots"),
                       (lambda: lib.ofdm_rx_reserve_pilots(None, 4, 100), "ofdm_rx_reserve_pilots"),
                       (lambda: lib.ofdm_pilot_track_frames(None, buf, 1, 2, 120, 3, 0, C.byref(out), None), "ofdm_pilot_track_frames"),
                       (lambda: lib.ofdm_rx_demod_frames_pilots(None, buf, 1, 32, 32, buf, None, 0, C.byref(out), None, None),
                        "ofdm_rx_demod_frames_pilots")):
        assert call() == L.OFDM_ERR_INVALID
        assert name in lib.ofdm_last_error().decode()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.ofdm_rx_set_pilots(dummy, None, 4, 1.0, 0.0) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_set_pilots(dummy, loc, -1, 1.0, 0.0) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_reserve_pilots(dummy, -1, 4) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_reserve_pilots(dummy, 4, -1) == L.OFDM_ERR_INVALID
    for n_seg, rows, stride, rpp, mode in ((-1, 2, 120, 3, 0), (1, -2, 120, 3, 0), (1, 2, 120, 0, 0), (1, 2, 120, 3, 2), (1, 2, 120, 3, -1)):
        assert lib.ofdm_pilot_track_frames(dummy, buf, n_seg, rows, stride, rpp, mode, C.byref(out), None) == L.OFDM_ERR_INVALID
        assert "ofdm_pilot_track_frames" in lib.ofdm_last_error().decode()
    bad = L.PilotOut()
    bad.bits = C.addressof(buf)                                     # bits without data
    bad.bits_mode = L.BITS_UNPACKED
    assert lib.ofdm_pilot_track_frames(dummy, buf, 1, 2, 120, 3, 0, C.byref(bad), None) == L.OFDM_ERR_INVALID
    assert "data" in lib.ofdm_last_error().decode()
    bad.data = C.addressof(buf)
    bad.bits_mode = 7
    assert lib.ofdm_pilot_track_frames(dummy, buf, 1, 2, 120, 3, 0, C.byref(bad), None) == L.OFDM_ERR_INVALID
    out.slope = C.addressof(buf)                                    # slope output in CPE mode
    assert lib.ofdm_pilot_track_frames(dummy, buf, 1, 2, 120, 3, L.PILOT_CPE, C.byref(out), None) == L.OFDM_ERR_INVALID
    out.slope = None
    # the receiver: d_eq is required, bad layout
    assert lib.ofdm_rx_demod_frames_pilots(dummy, buf, 1, 32, 32, None, None, 0, C.byref(out), None, None) == L.OFDM_ERR_INVALID
    assert "d_eq" in lib.ofdm_last_error().decode()
    assert lib.ofdm_rx_demod_frames_pilots(dummy, buf, 1, 16, 32, buf, None, 0, C.byref(out), None, None) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_demod_frames_pilots(dummy, None, 1, 32, 32, buf, None, 0, C.byref(out), None, None) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_demod_frames_pilots(dummy, buf, -1, 32, 32, buf, None, 0, C.byref(out), None, None) == L.OFDM_ERR_INVALID
