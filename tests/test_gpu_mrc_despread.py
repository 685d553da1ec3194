"""Receive diversity for DFT-spread OFDM on the GPU (-m gpu): ofdm_combine_despread_frames and ofdm_rx_demod_frames_mrc_despread
against tests/mrc_despread_ref.py (the contract of include/ofdm_mi355x.h restated in NumPy, pinned by
test_mrc_despread_ref_host.py).  comb is held bit for bit to the float32 restatement, sym to the suite's 1e-5 bar against fp64 on
those float32 values, beta and weight to one float32 ulp, llr and bits bit for bit to the contract's function of the device's own
stored sym and the row's weight.  Every output sits between poisoned guard bands.

Sizes: M = 12 (64 rows per workgroup), 60 (16), 64 (the smallest padded LDS layout), 75 (odd radices only), 1200 (one row per
workgroup in the small register class) and 2400 (the large class); B = 1, 2, 3, 8 (both remainders of the branch rounds, and the
most); rows = 1 and rows_per_group + 1 (a second workgroup per segment, with one row)."""
import ctypes as C
import math

import numpy as np
import pytest

import mrc_despread_ref as ref
from conftest import TOL_MAX, relerr
from oracle import ofdm_oracle as orc
from test_gpu_csi import Out, cur, demod, same_bits
from test_gpu_dft_spread import bits_of, put
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

MODS = ("QPSK", "16QAM", "64QAM")
BPS = ref.BPS
SIZES = (12, 60, 64, 75, 1200, 2400)
BRANCHES = (1, 2, 3, 8)
RHO = 0.03
WANT_ALL = ("sym", "llr", "bits", "beta", "weight", "comb")


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


def units(rng, B, n_seg, rows, M, mod, extra=0, csi_extra=3):
    """-> sym [B*n_seg][rows*M + extra] complex64 (NaN in the gap), csi [B*n_seg][M + csi_extra] float32 (NaN in the gap), sigma2
    [B*n_seg]: the same spread constellation rows per segment through B channels and one-tap MMSE equalisers, unit g = b*n_seg + s"""
    n = rows * M
    sym = np.full((B * n_seg, n + extra), complex(np.nan, np.nan), np.complex64)
    csi = np.full((B * n_seg, M + csi_extra), np.nan, np.float32)
    sig = np.zeros(B * n_seg)
    for s in range(n_seg):
        x = np.fft.fft(orc.map_bits(rng.integers(0, 2, n * BPS[mod]), mod).reshape(rows, M), axis=1) / math.sqrt(M)
        for b in range(B):
            g = b * n_seg + s
            a = rng.uniform(0.02, 2.0, M)
            sig[g] = (0.02, 0.05, 0.1)[(b + s) % 3]
            w = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))) * math.sqrt(sig[g] / 2)
            sym[g, :n] = ((a / (a + RHO)) * (x + w / np.sqrt(a))).ravel()
            csi[g, :M] = a
    return sym, csi, sig


def run(om, torch, rx, sym, csi, B, rows, M, mod, noise, want=WANT_ALL, base_off=0, rho=RHO, bits_mode=None):
    """combine_despread_frames on host arrays -> dict of host arrays.  noise: ("given", [B]) or ("seg", [B*n_seg])"""
    n_seg, bps = sym.shape[0] // B, BPS[mod]
    bits_mode = om.BITS_UNPACKED if bits_mode is None else bits_mode
    t, addr = put(torch, sym, base_off)
    d_csi = torch.from_numpy(np.ascontiguousarray(csi)).cuda()
    n = n_seg * rows * M
    nbits = n * bps if bits_mode == om.BITS_UNPACKED else n * bps // 8
    size = dict(sym=(2 * n, torch.float32), llr=(n * bps, torch.float32), bits=(nbits, torch.uint8), beta=(n_seg * rows, torch.float32),
                weight=(n_seg * rows, torch.float32), comb=(2 * n, torch.float32))
    o = {k: (Out(torch, *size[k]) if k in want else None) for k in WANT_ALL}
    d_sig = torch.from_numpy(np.asarray(noise[1], np.float64)).cuda() if noise[0] == "seg" else None
    rx.combine_despread_frames(addr, B, n_seg, rows, M, sym.shape[1], d_csi, csi.shape[1], rho, mod,
                               noise_var=list(noise[1]) if noise[0] == "given" else None, d_sigma2=d_sig,
                               d_sym_out=o["sym"] and o["sym"].addr, d_llr=o["llr"] and o["llr"].addr, d_bits=o["bits"] and o["bits"].addr,
                               bits_mode=bits_mode if "bits" in want else om.BITS_NONE, d_beta=o["beta"] and o["beta"].addr,
                               d_weight=o["weight"] and o["weight"].addr, d_comb=o["comb"] and o["comb"].addr, stream=cur(torch))
    torch.cuda.synchronize()
    return {k: (v.read().copy() if v else None) for k, v in o.items()}


def unit_sigma2(noise, B, n_seg):
    s2 = np.asarray(noise[1], np.float64)
    return np.repeat(s2, n_seg) if noise[0] == "given" else s2


def restated(sym, csi, B, rows, M, noise, rho=RHO):
    n_seg, n = sym.shape[0] // B, rows * M
    s2 = unit_sigma2(noise, B, n_seg)
    return [ref.combine_despread_segment(np.stack([sym[b * n_seg + s, :n].reshape(rows, M) for b in range(B)]),
                                         np.stack([csi[b * n_seg + s, :M] for b in range(B)]), rho, [s2[b * n_seg + s] for b in range(B)])
            for s in range(n_seg)]


def check_against_contract(got, sym, csi, B, rows, M, mod, noise, rho=RHO, packed=False):
    """-> the restated segments"""
    n_seg, n, bps = sym.shape[0] // B, rows * M, BPS[mod]
    segs = restated(sym, csi, B, rows, M, noise, rho)
    dev_sym = got["sym"].view(np.complex64).reshape(n_seg, rows, M)
    dev_comb = got["comb"].view(np.complex64).reshape(n_seg, rows, M)
    beta, weight = got["beta"].reshape(n_seg, rows), got["weight"].reshape(n_seg, rows)
    llr = got["llr"].reshape(n_seg, rows, M * bps)
    for s, seg in enumerate(segs):
        assert np.array_equal(bits_of(dev_comb[s]), bits_of(seg["comb"])), ("comb", s)                    # bit for bit
        e = relerr(dev_sym[s], seg["sym"]) if seg["sym"].any() else float(np.max(np.abs(dev_sym[s])))
        assert e < TOL_MAX, ("sym", s, e)
        for r in range(rows):
            for k, dev, want in (("beta", beta[s, r], seg["beta32"][r]), ("weight", weight[s, r], seg["weight32"][r])):
                assert abs(float(dev) - float(want)) <= float(np.spacing(np.float32(want))), (k, s, r, dev, want)
                assert (dev == 0) == (want == 0), (k, s, r)
            want_llr, hb = ref.outputs_from(dev_sym[s, r], weight[s, r], mod)
            assert same_bits(llr[s, r], want_llr), ("llr", s, r)
            at = (s * rows + r) * M * bps
            if packed:
                assert np.array_equal(got["bits"][at // 8:(at + M * bps) // 8], ref.pack_bits(hb)), ("bits", s, r)
            else:
                assert np.array_equal(got["bits"][at:at + M * bps], hb), ("bits", s, r)
            if not seg["usable"][r]:
                assert not bits_of(dev_sym[s, r]).any() and not bits_of(llr[s, r]).any(), ("+0", s, r)
    for k in ("sym", "llr", "beta", "weight", "comb"):
        assert np.isfinite(got[k]).all(), k
    return segs


# ------------------------------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("mod", MODS)
def test_stage_against_the_contract(om, torch, rx0, mod, M):
    rpg = om.dft_plan_info(M)[2]
    rng = np.random.default_rng(M + BPS[mod])
    for B in BRANCHES:
        n_seg = 3 if B in (2, 8) else 1
        for rows in (1, rpg + 1):
            # dense and 16-byte aligned, against an odd stride on an 8-byte base: there the branches' (and segments') bases
            # alternate between 8- and 16-byte alignment
            dense, csi, sig = units(rng, B, n_seg, rows, M, mod, extra=0)
            odd = np.full((B * n_seg, rows * M + 1), complex(np.nan, np.nan), np.complex64)
            odd[:, :rows * M] = dense
            noise = ("seg", sig) if B in (2, 8) else ("given", sig[::n_seg])
            a = run(om, torch, rx0, dense, csi, B, rows, M, mod, noise, base_off=0)
            b = run(om, torch, rx0, odd, csi, B, rows, M, mod, noise, base_off=8)
            check_against_contract(a, dense, csi, B, rows, M, mod, noise)
            for k in WANT_ALL:
                assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (k, B, rows)
            assert (a["beta"] > 0).all() and (a["weight"] > 0).all() and a["llr"].any()


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("mod", MODS)
def test_packed_bits(om, torch, rx0, mod, M):
    """B = 3, two segments of rows_per_group + 1 rows on an odd stride: packed where a row's bits fill bytes, refused where not"""
    rpg = om.dft_plan_info(M)[2]
    rng = np.random.default_rng(3 * M + BPS[mod])
    B, n_seg, rows = 3, 2, rpg + 1
    sym, csi, sig = units(rng, B, n_seg, rows, M, mod, extra=1)
    noise = ("seg", sig)
    if M * BPS[mod] % 8 != 0:                                # M = 75 with QPSK and 64-QAM
        with pytest.raises(ValueError, match="packed bits"):
            run(om, torch, rx0, sym, csi, B, rows, M, mod, noise, base_off=8, bits_mode=om.BITS_PACKED)
        return
    got = run(om, torch, rx0, sym, csi, B, rows, M, mod, noise, base_off=8, bits_mode=om.BITS_PACKED)
    check_against_contract(got, sym, csi, B, rows, M, mod, noise, packed=True)


@pytest.mark.parametrize("mod", MODS)
def test_outputs_alone_segments_alone_rows_moved_and_repeats(om, torch, rx0, mod):
    rng = np.random.default_rng(5 + BPS[mod])
    B, n_seg, rows, M = 3, 3, 19, 60                         # 16 rows per group: two groups per segment
    n, bps = rows * M, BPS[mod]
    sym, csi, sig = units(rng, B, n_seg, rows, M, mod, extra=1)
    noise = ("seg", sig)
    full = run(om, torch, rx0, sym, csi, B, rows, M, mod, noise, base_off=8)
    again = run(om, torch, rx0, sym, csi, B, rows, M, mod, noise, base_off=8)
    per = dict(sym=2 * n, llr=n * bps, bits=n * bps, beta=rows, weight=rows, comb=2 * n)
    for k in WANT_ALL:
        assert np.array_equal(again[k].view(np.uint8), full[k].view(np.uint8)), k                         # every call the same bits
        one = run(om, torch, rx0, sym, csi, B, rows, M, mod, noise, want=(k,), base_off=8)
        assert np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), k                           # every output alone
    for s in range(n_seg):                                   # a segment alone, dense and aligned
        pick = [b * n_seg + s for b in range(B)]
        alone = run(om, torch, rx0, np.ascontiguousarray(sym[pick, :n]), csi[pick], B, rows, M, mod, ("seg", sig[pick]))
        for k in WANT_ALL:
            assert np.array_equal(alone[k].view(np.uint8), full[k][s * per[k]:(s + 1) * per[k]].view(np.uint8)), (k, s)
    # rows moved within their segment (to other places in the group, to the other group): every row keeps its bits
    shift = 5
    moved = sym.copy()
    moved[:, :n] = np.roll(sym[:, :n].reshape(B * n_seg, rows, M), shift, axis=1).reshape(B * n_seg, n)
    got = run(om, torch, rx0, moved, csi, B, rows, M, mod, noise, base_off=8)
    for k, width in (("beta", 1), ("weight", 1), ("sym", 2 * M), ("llr", M * bps), ("comb", 2 * M), ("bits", M * bps)):
        a = full[k].reshape(n_seg, rows, width)
        b = got[k].reshape(n_seg, rows, width)
        assert np.array_equal(np.roll(a, shift, axis=1).view(np.uint8), b.view(np.uint8)), k


@pytest.mark.parametrize("M", [60, 2400])
def test_comb_through_the_plain_inverse_is_the_row_before_scaling(om, torch, rx0, M):
    rng = np.random.default_rng(M)
    B, n_seg, rows = 2, 2, 3
    sym, csi, sig = units(rng, B, n_seg, rows, M, "16QAM")
    got = run(om, torch, rx0, sym, csi, B, rows, M, "16QAM", ("seg", sig))
    t, addr = put(torch, got["comb"].view(np.complex64))
    x = Out(torch, n_seg * rows * M * 2, torch.float32)
    rx0.dft_despread_frames(addr, n_seg, rows, M, rows * M, None, 0, 0.0, "16QAM", d_sym_out=x.addr, stream=cur(torch))
    plain = x.read().view(np.complex64).reshape(n_seg * rows, M)
    dev = got["sym"].view(np.complex64).reshape(n_seg * rows, M)
    scaled = plain.astype(np.complex128) / got["beta"].astype(np.float64)[:, None]
    assert relerr(dev, scaled) < TOL_MAX


# ------------------------------------------------------------------------------------------ 2. planted cases
@pytest.mark.parametrize("mod", MODS)
def test_planted_entries_symbols_and_rows(om, torch, rx0, mod):
    rng = np.random.default_rng(77 + BPS[mod])
    B, n_seg, rows, M = 3, 1, 6, 60
    n, bps = rows * M, BPS[mod]
    sym, csi, sig = units(rng, B, n_seg, rows, M, mod, extra=1)
    for j, a in zip((3, 11, 20, 41), (0.0, -1.0, np.nan, np.inf)):      # branch 1: unusable entries
        csi[1, j] = a
    csi[:, 30] = (0.0, np.nan, -2.0)                                      # entry 30: unusable in every branch
    for i, z in zip((5, 70, 140), (complex(np.nan, 0.1), complex(0.1, np.inf), complex(-np.inf, np.nan))):
        sym[2, i] = z                                                     # branch 2: non-finite symbols in usable entries
    sym[1, 2 * M:3 * M] = 0                                               # branch 1 misses row 2
    sym[:, 4 * M:5 * M] = 0                                               # row 4 has nothing in any branch
    noise = ("seg", sig)
    got = run(om, torch, rx0, sym, csi, B, rows, M, mod, noise)
    seg = check_against_contract(got, sym, csi, B, rows, M, mod, noise)[0]
    comb = got["comb"].view(np.complex64).reshape(rows, M)
    dsym = got["sym"].view(np.complex64).reshape(rows, M)
    assert not bits_of(comb[:, 30]).any() and (seg["A"][:, 30] == 0).all()
    assert comb[0, 3] != 0 and comb[0, 5] != 0 and not seg["took"][1, 0, 3] and not seg["took"][2, 0, 5]
    # row 2: the beta of branches 0 and 2, other than its neighbours'
    pick = [0, 2]
    others = run(om, torch, rx0, np.ascontiguousarray(sym[pick]), csi[pick], 2, rows, M, mod, ("seg", sig[pick]))
    for k in ("beta", "weight"):
        assert got[k][2] == others[k][2] and got[k][2] < got[k][1] and got[k][2] < got[k][3] and got[k][2] > 0
    assert np.array_equal(bits_of(dsym[2]), bits_of(others["sym"].view(np.complex64).reshape(rows, M)[2]))
    # row 4: an erasure, +0 everywhere, the bits of a zero symbol
    assert seg["erased"][4] and got["beta"][4] == 0 and got["weight"][4] == 0 and not bits_of(dsym[4]).any()
    assert not bits_of(got["llr"].reshape(rows, -1)[4]).any() and not bits_of(comb[4]).any()
    assert np.array_equal(got["bits"].reshape(rows, -1)[4], np.tile(orc.demap_hard(np.zeros(1, np.complex64), mod), M))
    assert dsym[[0, 1, 2, 3, 5]].all() and (got["beta"][[0, 1, 2, 3, 5]] > 0).all()


def test_planted_variances_and_ranges(om, torch, rx0):
    mod = "16QAM"
    rng = np.random.default_rng(78)
    B, n_seg, rows, M = 3, 2, 3, 60
    sym, csi, sig = units(rng, B, n_seg, rows, M, mod)
    base = run(om, torch, rx0, sym, csi, B, rows, M, mod, ("seg", sig))
    pick = [0, 1, 4, 5]                                                   # branches 0 and 2
    others = run(om, torch, rx0, np.ascontiguousarray(sym[pick]), csi[pick], 2, rows, M, mod, ("seg", sig[pick]))
    for bad in (0.0, np.nan, np.inf, -0.5):
        s2 = sig.copy()
        s2[2] = bad                                                       # branch 1 of segment 0: the others carry
        got = run(om, torch, rx0, sym, csi, B, rows, M, mod, ("seg", s2))
        check_against_contract(got, sym, csi, B, rows, M, mod, ("seg", s2))
        for k in WANT_ALL:
            half = got[k].size // 2
            assert np.array_equal(got[k][:half].view(np.uint8), others[k][:half].view(np.uint8)), (k, bad)
            assert np.array_equal(got[k][half:].view(np.uint8), base[k][half:].view(np.uint8)), (k, bad)
        s2[[0, 2, 4]] = bad                                               # every branch of segment 0: every row erased
        got = run(om, torch, rx0, sym, csi, B, rows, M, mod, ("seg", s2))
        check_against_contract(got, sym, csi, B, rows, M, mod, ("seg", s2))
        for k in ("sym", "llr", "beta", "weight", "comb"):
            half = got[k].size // 2
            assert not bits_of(got[k][:half]).any() and got[k][half:].any(), (k, bad)
    # a / sigma2 = 1e30: usable, beta = 1, a finite weight
    big = np.full_like(csi, 1e10)
    got = run(om, torch, rx0, sym, big, B, rows, M, mod, ("given", [1e-20] * B))
    check_against_contract(got, sym, big, B, rows, M, mod, ("given", [1e-20] * B))
    assert (got["beta"] == 1).all() and (got["weight"] > 1e29).all() and got["sym"].any()
    # The weight cannot overflow: w = sum b / sum e <= max A, a finite float32.  float(1/beta) can -- t = 1e-40 is a float32
    # denormal, beta = 1e-40: the rows are not usable and sym is +0 although every symbol was combined
    tiny = np.full_like(csi, 1e-30)
    got = run(om, torch, rx0, sym, tiny, B, rows, M, mod, ("given", [1e10] * B), rho=0.0)
    segs = check_against_contract(got, sym, tiny, B, rows, M, mod, ("given", [1e10] * B), rho=0.0)
    assert all((s["A"] > 0).all() and not s["usable"].any() for s in segs)
    assert got["comb"].any() and not bits_of(got["sym"]).any() and not bits_of(got["beta"]).any() and not bits_of(got["weight"]).any()


# ------------------------------------------------------------------------------------------ 3. refusals
def test_argument_errors_leave_the_outputs_untouched(om, torch, rx0):
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    sig = torch.ones(8, dtype=torch.float64, device="cuda")
    o = {k: Out(torch, 512, torch.uint8 if k == "bits" else torch.float32) for k in WANT_ALL}
    ok = dict(n_branch=2, n_seg=2, rows=3, M=12, seg_stride=36, csi_stride=12, rho=RHO, modulation="QPSK", noise_var=[0.1, 0.2],
              sigma2=None, bits_mode=om.BITS_UNPACKED)

    def call(a, sym=d):
        rx0.combine_despread_frames(sym, a["n_branch"], a["n_seg"], a["rows"], a["M"], a["seg_stride"], d, a["csi_stride"], a["rho"],
                                    a["modulation"], noise_var=a["noise_var"], d_sigma2=a["sigma2"], d_sym_out=o["sym"].addr,
                                    d_llr=o["llr"].addr, d_bits=o["bits"].addr, bits_mode=a["bits_mode"], d_beta=o["beta"].addr,
                                    d_weight=o["weight"].addr, d_comb=o["comb"].addr, stream=cur(torch))

    bad = (dict(M=7), dict(M=0), dict(M=4100), dict(n_seg=-1), dict(rows=-1), dict(n_branch=0, noise_var=[]),
           dict(n_branch=9, noise_var=[0.1] * 9), dict(seg_stride=35), dict(csi_stride=11), dict(modulation="BPSK"), dict(modulation=3),
           dict(noise_var=[0.1, 0.0]), dict(noise_var=[-1.0, 0.1]), dict(noise_var=[0.1, float("nan")]), dict(noise_var=[float("inf"), 0.1]),
           dict(rho=-1.0), dict(rho=float("inf")), dict(bits_mode=om.BITS_NONE), dict(bits_mode=7),
           dict(M=75, seg_stride=225, csi_stride=75, bits_mode=om.BITS_PACKED), dict(n_seg=1 << 32), dict(n_seg=1 << 19, seg_stride=1 << 30),
           dict(n_seg=1 << 19, csi_stride=1 << 30),
           dict(n_branch=1, noise_var=[0.1], n_seg=1 << 31, rows=1, seg_stride=12))   # more than 2^31 - 1 workgroups
    for kw in bad:
        with pytest.raises(ValueError, match="ofdm_combine_despread_frames"):
            call(dict(ok, **kw))
    with pytest.raises(ValueError, match="no pointer"):
        rx0.combine_despread_frames(d, 2, 2, 3, 12, 36, d, 12, RHO, "QPSK", noise_var=[0.1, 0.2], stream=cur(torch))
    with pytest.raises(ValueError, match="null d_sym or d_csi"):
        call(ok, sym=None)
    with pytest.raises(ValueError, match="exactly one"):
        rx0.combine_despread_frames(d, 2, 2, 3, 12, 36, d, 12, RHO, "QPSK", noise_var=[0.1, 0.2], d_sigma2=sig, d_llr=o["llr"].addr)
    # OFDM_MRC_NOISE_EST, which the engine never passes: refused by both calls
    from ofdm_mi355x import _lib
    out = _lib.MrcDespreadOut(llr=o["llr"].addr, sym=o["sym"].addr)
    two = (C.c_double * 2)(0.1, 0.2)
    lib, h, p = rx0.lib, rx0._h, d.data_ptr()
    assert lib.ofdm_combine_despread_frames(h, p, 2, 2, 3, 12, 36, p, 12, RHO, 2, om.MRC_NOISE_EST, two, sig.data_ptr(), om.BITS_NONE,
                                            C.byref(out), None) == -1
    assert b"OFDM_MRC_NOISE_EST" in lib.ofdm_last_error()
    assert lib.ofdm_rx_demod_frames_mrc_despread(h, p, 2, 1, 32, 32, p, None, om.MRC_NOISE_EST, two, None, om.BITS_NONE, C.byref(out),
                                                 None) == -1
    assert b"OFDM_MRC_NOISE_EST" in lib.ofdm_last_error() and b"ofdm_rx_demod_frames_mrc_despread" in lib.ofdm_last_error()
    with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc_despread"):
        rx0.reserve_mrc_despread(7, 2, 1)
    with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc_despread"):
        rx0.reserve_mrc_despread(60, 9, 1)
    bp = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100, modulation="BPSK")
    with pytest.raises(ValueError, match="ofdm_rx_demod_frames_mrc_despread"):
        bp.demod_frames_mrc_despread(d, 2, 1, 32, 32, d, noise_var=[0.1, 0.2], d_llr=o["llr"].addr)
    with pytest.raises(ValueError, match="ofdm_rx_demod_frames_mrc_despread"):
        rx0.demod_frames_mrc_despread(d, 2, 1, 32, 32, d, noise_var=[0.1, -0.2], d_llr=o["llr"].addr)
    with pytest.raises(ValueError, match="needs d_eq"):
        rx0.demod_frames_mrc_despread(d, 2, 1, 32, 32, None, noise_var=[0.1, 0.2], d_llr=o["llr"].addr)
    with pytest.raises(ValueError, match="no pointer"):
        rx0.demod_frames_mrc_despread(d, 2, 1, 32, 32, d, noise_var=[0.1, 0.2])
    call(dict(ok, n_seg=0))                                   # zero counts: no-ops
    call(dict(ok, rows=0, seg_stride=0))
    torch.cuda.synchronize()
    assert all(o[k].untouched() for k in WANT_ALL)


# ------------------------------------------------------------------------------------------ 4. the composite call
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
        return dict(sym=Out(torch, n_out * 2, torch.float32), llr=Out(torch, n_out * bps, torch.float32), bits=Out(torch, n_out * bps, torch.uint8),
                    beta=Out(torch, nf * nds, torch.float32), weight=Out(torch, nf * nds, torch.float32), comb=Out(torch, n_out * 2, torch.float32))

    p_eq, p_tsr = Out(torch, n_eq * 2, torch.float32), Out(torch, n * 4, torch.int32)
    assert rx.demod_frames(d_iq, n, fl, fl, p_eq.addr, d_tsr=p_tsr.addr) == nds
    d_a = Out(torch, n * Kd, torch.float32)
    rx.csi_frames(n, d_a.addr)
    assert p_tsr.read().reshape(n, 4)[nf + 1, 3] == 0
    sig = np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.06])
    d_sig = torch.from_numpy(sig).cuda()
    for noise in (("given", [0.02, 0.03]), ("seg", sig)):
        nv, ds = (noise[1], None) if noise[0] == "given" else (None, d_sig)
        a, b = outs(), outs()
        rx.combine_despread_frames(p_eq.addr, B, nf, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, mod, nv, ds, a["sym"].addr, a["llr"].addr,
                                   a["bits"].addr, om.BITS_UNPACKED, a["beta"].addr, a["weight"].addr, a["comb"].addr)
        c_eq, c_tsr = Out(torch, n_eq * 2, torch.float32), Out(torch, n * 4, torch.int32)
        r = rx.demod_frames_mrc_despread(d_iq, B, nf, fl, fl, c_eq.addr, nv, ds, b["sym"].addr, b["llr"].addr, b["bits"].addr,
                                         om.BITS_UNPACKED, b["beta"].addr, b["weight"].addr, b["comb"].addr, d_tsr=c_tsr.addr)
        assert r == nds
        assert np.array_equal(bits_of(p_eq.read()), bits_of(c_eq.read())) and np.array_equal(p_tsr.read(), c_tsr.read())
        for k in a:
            assert np.array_equal(a[k].read().view(np.uint8), b[k].read().view(np.uint8)), (k, noise[0])
        # the contract on the downloaded rows
        eq = p_eq.read().view(np.complex64).reshape(n, nds * Kd)
        csi = d_a.read().reshape(n, Kd)
        got = {k: v.read().copy() for k, v in b.items()}
        segs = check_against_contract(got, eq, csi, B, nds, Kd, mod, noise, rho=rx.csi_rho)
        # frame 1: branch 1 found no sync and takes no part; frame 2 of branch 0 ends in guard-failed rows: branch 1 carries them
        assert not segs[1]["took"][1].any() and segs[1]["took"][0].all() and (got["beta"].reshape(nf, nds)[1] > 0).all()
        assert not eq.reshape(B, nf, nds, Kd)[0, 2, -1].any() and got["beta"].reshape(nf, nds)[2, -1] > 0
        assert got["beta"].reshape(nf, nds)[2, -1] < got["beta"].reshape(nf, nds)[2, 0]


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
    rx.reserve_mrc_despread(Kd, B, nf - 1)                   # one frame per branch short of the batch that is captured second
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                sym=torch.zeros(nf * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                llr=torch.zeros(nf * nds * Kd * 4, dtype=torch.float32, device="cuda"),
                weight=torch.zeros(nf * nds, dtype=torch.float32, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(stream, frames):
        return rx.demod_frames_mrc_despread(d_iq, B, frames, fl, fl, outs["eq"], noise_var=[0.02, 0.05], d_sym_out=outs["sym"],
                                            d_llr=outs["llr"], d_weight=outs["weight"], stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream, nf - 1)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["weight"][:(nf - 1) * nds] > 0).all()) and bool(eager["llr"].any())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                      # a linear capture: one stream, no parallel branches
        call(torch.cuda.current_stream().cuda_stream, nf - 1)
        with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc_despread"):
            call(torch.cuda.current_stream().cuda_stream, nf)  # a larger batch: the workspace would have to grow
        with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc_despread"):
            rx.combine_despread_frames(outs["eq"], 1, 1, 1, 300, 300, outs["eq"], 300, 0.03, mod, noise_var=[0.1], d_sym_out=outs["sym"],
                                       stream=torch.cuda.current_stream().cuda_stream)  # a plan the handle does not hold
    assert not outs["weight"].any()                          # capture enqueues nothing
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k


# ------------------------------------------------------------------------------------------ 5. the link, end to end on the device
def test_link_case_decodes_where_neither_branch_does(om, torch):
    """mrc_despread_cases end to end: turbo_encode_frames -> modulate_frames_spread -> channel (taps and noise seed per branch,
    into one IQ buffer of 2 * 64 frames) -> demod_frames_mrc_despread -> turbo_decode_frames gives every block back; each branch
    alone through demod_frames_despread with the noise given loses blocks (27 and 55 on the oracle's receiver)."""
    import mrc_despread_cases as dc
    n, L, B = dc.N_FRAMES, dc.N + dc.CP, dc.N_BRANCH
    txe = om.TxEngine(dc.N, dc.CP, dc.KS, dc.KD, (1, 3), dc.MOD)
    rxe = om.RxEngine(dc.N_SYM, dc.N, dc.CP, dc.KS, (1, 3), dc.KD, dc.SNR_ARG, dc.GATE, modulation=dc.MOD)
    rxe.set_max_trials(0)
    info = dc.info_bits()
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * dc.SEG_BITS)
    txe.turbo_encode_frames(d_info, n, 1, dc.K, dc.F1, dc.F2, d_coded, dc.SEG_BITS)
    fl_tx, fl = dc.N_SYM * L, dc.FRAME_LEN
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(B * n * fl * 8)
    assert txe.modulate_frames_spread(d_coded, n, dc.N_SYM, d_tx) == n * dc.N_SYM
    for b in range(B):
        taps = np.asarray(dc.TAPS[b]).astype(np.complex64)
        d_taps = om.DeviceBuffer(taps.nbytes).upload(taps)
        txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx.data_ptr() + b * n * fl * 8, fl, fl, noise_var=dc.NOISE_VAR,
                    seed=dc.SEED_NOISE + b)
    assert rxe.data_symbols_per_frame(fl) == dc.N_DSYM
    d_eq = om.DeviceBuffer(B * n * dc.N_DSYM * dc.KD * 8)
    d_llr = om.DeviceBuffer(n * dc.SEG_BITS * 4)
    d_beta = om.DeviceBuffer(n * dc.N_DSYM * 4)
    d_bits = om.DeviceBuffer(n * dc.K)

    def lost():
        rxe.turbo_decode_frames(d_llr, n, dc.SEG_BITS, 1, dc.K, dc.F1, dc.F2, dc.N_ITER, d_bits=d_bits)
        return int((d_bits.download(np.uint8, n * dc.K).reshape(n, 1, dc.K) != info).any(axis=(1, 2)).sum())

    assert rxe.demod_frames_mrc_despread(d_rx, B, n, fl, fl, d_eq, noise_var=[dc.NOISE_VAR] * B, d_llr=d_llr, d_beta=d_beta) == dc.N_DSYM
    assert (d_beta.download(np.float32, n * dc.N_DSYM) > 0).all(), "every frame should find its sync"
    res = {"combined": lost()}
    for b in range(B):
        assert rxe.demod_frames_despread(d_rx.data_ptr() + b * n * fl * 8, n, fl, fl, d_eq, d_llr=d_llr,
                                         noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=dc.NOISE_VAR) == dc.N_DSYM
        res["branch %d alone" % b] = lost()
    print("blocks lost of %d: %r" % (n, res))
    assert res["combined"] == 0
    assert res["branch 0 alone"] >= 1 and res["branch 1 alone"] >= 1
