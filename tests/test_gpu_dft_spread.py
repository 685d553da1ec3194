"""DFT-spread OFDM on the GPU (-m gpu): ofdm_tx_dft_spread, ofdm_dft_despread_frames and the two composite calls against
tests/dft_spread_ref.py (the contract of include/ofdm_mi355x.h in fp64 NumPy, pinned by test_dft_spread_ref_host.py).  Transforms
are held to the suite's 1e-5 bar, beta and weight to one float32 ulp, llr and bits bit for bit to the contract's function of the
device's own stored sym and weight.  Every output sits between poisoned guard bands.

Sizes: the list the feature was specified with, plus M = 64 (the smallest size with the padded LDS layout, 16 rows per
workgroup) and M = 2048 (padded layout with a radix-2 last pass): the list itself reaches the padded layout only at 4096."""
import math

import numpy as np
import pytest

import dft_spread_ref as ref
from conftest import TOL_MAX, relerr
from oracle import ofdm_oracle as orc
from test_gpu_csi import Out, cur, demod, same_bits
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

MODS = ("QPSK", "16QAM", "64QAM")
BPS = ref.BPS
SIZES = [1, 2, 3, 4, 5, 6, 8, 9, 12, 15, 16, 25, 27, 36, 60, 64, 75, 96, 125, 243, 300, 600, 625, 1200, 1296, 2048, 2187, 2400, 3125,
         4050, 4096]
SHAPES = [(1, 12), (3, 60), (9, 60), (2, 75), (5, 600), (4, 1200)]                   # (rows, M)
RHO = 0.03


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
def tx0(om):
    return om.TxEngine(64, 16, 62, 60, (1, 3), "QPSK")


@pytest.fixture(scope="module")
def rx0(om):
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def put(torch, x, base_off=0):
    """host complex64 array -> (tensor that owns it, device address), the data base_off bytes off the 16-byte grid"""
    v = np.ascontiguousarray(x).view(np.float32).ravel()
    t = torch.zeros(v.size + 4, dtype=torch.float32, device="cuda")
    t[base_off // 4:base_off // 4 + v.size] = torch.from_numpy(v).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + base_off


def bits_of(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. the transforms alone
@pytest.mark.parametrize("M", SIZES)
def test_transforms_against_fp64(om, torch, tx0, rx0, M):
    n_pass, radix8, rpg = om.dft_plan_info(M)
    rng = np.random.default_rng(M)
    for n_rows in (1, rpg + 1):
        x = crandn(rng, n_rows, M)
        want = {"fwd": ref.spread(x), "inv": ref.inverse(x)}
        first = {}
        for base_off in (0, 8):
            for in_place in (False, True):
                for call in (0, 1):
                    for d in ("fwd", "inv"):
                        t, addr = put(torch, x, base_off)
                        o = Out(torch, n_rows * M * 2, torch.float32)
                        dst = addr if in_place else o.addr
                        if d == "fwd":
                            tx0.dft_spread(addr, n_rows, M, dst, stream=cur(torch))
                        else:
                            rx0.dft_despread_frames(addr, 1, n_rows, M, n_rows * M, None, 0, 0.0, "QPSK", d_sym_out=dst, stream=cur(torch))
                        torch.cuda.synchronize()
                        if in_place:
                            assert o.untouched()
                            got = t.cpu().numpy()[base_off // 4:base_off // 4 + n_rows * M * 2].view(np.complex64).reshape(n_rows, M)
                        else:
                            got = o.read().view(np.complex64).reshape(n_rows, M)
                        assert relerr(got, want[d]) < TOL_MAX, (d, n_rows, base_off, in_place, relerr(got, want[d]))
                        key = (d, n_rows)
                        first.setdefault(key, got.copy())
                        assert np.array_equal(bits_of(got), bits_of(first[key])), (d, n_rows, base_off, in_place, call)


def test_transform_arguments(om, torch, tx0, rx0):
    d = torch.zeros(256, dtype=torch.float32, device="cuda")
    o = Out(torch, 64, torch.float32)
    for M in (0, 7, 14, 4097, 4100, -4):
        assert not om.dft_size_ok(M)
        with pytest.raises(ValueError, match="ofdm_tx_dft_spread"):
            tx0.dft_spread(d, 1, M, o.addr, stream=cur(torch))
        with pytest.raises(ValueError, match="ofdm_tx_reserve_spread"):
            tx0.reserve_spread(M)
        with pytest.raises(ValueError, match="ofdm_rx_reserve_despread"):
            rx0.reserve_despread(M)
    with pytest.raises(ValueError, match="negative"):
        tx0.dft_spread(d, -1, 12, o.addr, stream=cur(torch))
    tx0.dft_spread(d, 0, 12, o.addr, stream=cur(torch))                                  # a no-op
    for M in (2, 3, 4, 5, 6, 8, 9, 10, 12, 15):                                          # more plans than a handle keeps
        tx0.reserve_spread(M)
    x = crandn(np.random.default_rng(1), 3, 2)
    t, addr = put(torch, x)
    g = Out(torch, 12, torch.float32)
    tx0.dft_spread(addr, 3, 2, g.addr, stream=cur(torch))                                # M = 2 had made room: built again
    assert relerr(g.read().view(np.complex64).reshape(3, 2), ref.spread(x)) < TOL_MAX
    torch.cuda.synchronize()
    assert o.untouched()


# ------------------------------------------------------------------------------------------ 2. the despread contract
def segments(rng, n_seg, rows, M, mod, extra=0, csi_extra=3, noise=(0.002, 0.005, 0.01)):
    """-> sym [n_seg][rows*M + extra] complex64 (NaN in the gap), csi [n_seg][M + csi_extra] float32 (NaN in the gap), sigma2
    [n_seg]: spread constellation rows through a one-tap MMSE equaliser"""
    n = rows * M
    sym = np.full((n_seg, n + extra), complex(np.nan, np.nan), np.complex64)
    csi = np.full((n_seg, M + csi_extra), np.nan, np.float32)
    sig = np.zeros(n_seg)
    for s in range(n_seg):
        a = rng.uniform(0.02, 2.0, M)
        x = ref.spread(orc.map_bits(rng.integers(0, 2, n * BPS[mod]), mod).reshape(rows, M))
        sig[s] = noise[s % 3]
        w = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))) * math.sqrt(sig[s] / 2)
        sym[s, :n] = ((a / (a + RHO)) * (x + w / np.sqrt(a))).ravel()
        csi[s, :M] = a
    return sym, csi, sig


WANT_ALL = ("sym", "llr", "bits", "beta", "weight")


def run(om, torch, rx, sym, csi, rows, M, mod, noise=("rho", None), want=WANT_ALL, base_off=0, rho=RHO, bits_mode=None):
    """dft_despread_frames on host arrays -> dict of host arrays.  noise: ("rho", None), ("given", var) or ("seg", [n_seg])"""
    n_seg, bps = sym.shape[0], BPS[mod]
    bits_mode = om.BITS_UNPACKED if bits_mode is None else bits_mode
    t, addr = put(torch, sym, base_off)
    d_csi = None if csi is None else torch.from_numpy(np.ascontiguousarray(csi)).cuda()
    n = n_seg * rows * M
    nbits = n * bps if bits_mode == om.BITS_UNPACKED else n * bps // 8
    size = dict(sym=(2 * n, torch.float32), llr=(n * bps, torch.float32), bits=(nbits, torch.uint8), beta=(n_seg, torch.float32),
                weight=(n_seg, torch.float32))
    o = {k: (Out(torch, *size[k]) if k in want else None) for k in WANT_ALL}
    d_sig = torch.from_numpy(np.asarray(noise[1], np.float64)).cuda() if noise[0] == "seg" else None
    mode = dict(rho=om.DESPREAD_NOISE_RHO, given=om.DESPREAD_NOISE_GIVEN, seg=om.DESPREAD_NOISE_SEG)[noise[0]]
    rx.dft_despread_frames(addr, n_seg, rows, M, sym.shape[1], d_csi, 0 if csi is None else csi.shape[1], rho, mod,
                           d_sym_out=o["sym"] and o["sym"].addr, d_llr=o["llr"] and o["llr"].addr, d_bits=o["bits"] and o["bits"].addr,
                           bits_mode=bits_mode if "bits" in want else om.BITS_NONE, d_beta=o["beta"] and o["beta"].addr,
                           d_weight=o["weight"] and o["weight"].addr, noise_mode=mode,
                           noise_var=noise[1] if noise[0] == "given" else 0.0, d_sigma2=d_sig, stream=cur(torch))
    torch.cuda.synchronize()
    return {k: (v.read().copy() if v else None) for k, v in o.items()}


def sigma2_of(noise, s, rho=RHO):
    return float(np.float32(rho)) if noise[0] == "rho" else float(noise[1]) if noise[0] == "given" else float(noise[1][s])


def check_against_contract(got, sym, csi, rows, M, mod, noise, rho=RHO, packed=False):
    n_seg, n, bps = sym.shape[0], rows * M, BPS[mod]
    dev_sym = got["sym"].view(np.complex64).reshape(n_seg, n)
    want_sym = np.zeros((n_seg, n), np.complex128)
    for s in range(n_seg):
        u, wt, _ = ref.despread_segment(sym[s, :n].reshape(rows, M), None if csi is None else csi[s, :M], rho, sigma2_of(noise, s, rho))
        want_sym[s] = u.ravel()
        for k, key in (("beta", "beta32"), ("weight", "weight32")):
            assert abs(float(got[k][s]) - float(wt[key])) <= float(np.spacing(np.float32(wt[key]))), (k, s, got[k][s], wt[key])
        llr, hb = ref.outputs_from(dev_sym[s], got["weight"][s], mod)
        assert same_bits(got["llr"][s * n * bps:(s + 1) * n * bps], llr), s
        mine = ref.pack_bits(hb) if packed else hb
        assert np.array_equal(got["bits"][s * mine.size:(s + 1) * mine.size], mine), s
    e = relerr(dev_sym, want_sym)
    assert e < TOL_MAX, e
    for k in ("sym", "llr", "beta", "weight"):
        assert np.isfinite(got[k]).all(), k


@pytest.mark.parametrize("rows,M", SHAPES)
@pytest.mark.parametrize("mod", MODS)
def test_despread_against_the_contract(om, torch, rx0, mod, rows, M):
    rng = np.random.default_rng(1000 * rows + M + BPS[mod])
    for n_seg in (1, 3):
        for extra, base_off in ((0, 0), (1, 8)):             # dense and 16-byte aligned; odd stride and 8-byte alignment only
            sym, csi, sig = segments(rng, n_seg, rows, M, mod, extra=extra)
            for noise in (("rho", None), ("given", 0.004), ("seg", sig)):
                got = run(om, torch, rx0, sym, csi, rows, M, mod, noise, base_off=base_off)
                check_against_contract(got, sym, csi, rows, M, mod, noise)
                assert (got["beta"] > 0).all() and (got["weight"] > 0).all() and got["llr"].any()
    if M * BPS[mod] % 8 == 0:
        got = run(om, torch, rx0, sym, csi, rows, M, mod, ("seg", sig), base_off=8, bits_mode=om.BITS_PACKED)
        check_against_contract(got, sym, csi, rows, M, mod, ("seg", sig), packed=True)
    # the same segment alone, moved and dense: the same bits
    full = run(om, torch, rx0, sym, csi, rows, M, mod, ("seg", sig), base_off=8)
    n = rows * M
    for s in range(sym.shape[0]):
        alone = run(om, torch, rx0, np.ascontiguousarray(sym[s:s + 1, :n]), csi[s:s + 1], rows, M, mod, ("seg", sig[s:s + 1]))
        for k, per in (("sym", 2 * n), ("llr", n * BPS[mod]), ("bits", n * BPS[mod]), ("beta", 1), ("weight", 1)):
            assert np.array_equal(alone[k].view(np.uint8), full[k][s * per:(s + 1) * per].view(np.uint8)), (k, s)


@pytest.mark.parametrize("mod", MODS)
def test_each_output_alone_and_in_place(om, torch, rx0, mod):
    rng = np.random.default_rng(5 + BPS[mod])
    rows, M = 3, 60
    sym, csi, sig = segments(rng, 3, rows, M, mod)
    full = run(om, torch, rx0, sym, csi, rows, M, mod, ("given", 0.01))
    for k in WANT_ALL:
        one = run(om, torch, rx0, sym, csi, rows, M, mod, ("given", 0.01), want=(k,))
        assert np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), k
    t, addr = put(torch, sym)
    d_csi = torch.from_numpy(csi).cuda()
    rx0.dft_despread_frames(addr, 3, rows, M, rows * M, d_csi, csi.shape[1], RHO, mod, d_sym_out=addr, noise_mode=om.DESPREAD_NOISE_GIVEN,
                            noise_var=0.01, stream=cur(torch))
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(t.cpu().numpy()[:sym.size * 2]), bits_of(full["sym"]))


@pytest.mark.parametrize("rows,M", SHAPES)
def test_without_channel_state_it_is_the_inverse_of_the_precoder(om, torch, tx0, rx0, rows, M):
    rng = np.random.default_rng(rows + M)
    x = orc.map_bits(rng.integers(0, 2, 2 * rows * M * 4), "16QAM").astype(np.complex64).reshape(2, rows * M)
    t, addr = put(torch, x)
    z = Out(torch, x.size * 2, torch.float32)
    tx0.dft_spread(addr, 2 * rows, M, z.addr, stream=cur(torch))
    spread = z.read().view(np.complex64).reshape(2, rows * M)
    assert relerr(spread, ref.spread(x.reshape(-1, M)).reshape(2, -1)) < TOL_MAX
    got = run(om, torch, rx0, spread, None, rows, M, "16QAM", ("given", float("nan")))      # the noise mode is ignored
    assert (got["beta"] == 1).all() and (got["weight"] == 1).all()
    assert relerr(got["sym"].view(np.complex64).reshape(2, -1), x) < TOL_MAX
    assert np.array_equal(got["bits"], orc.demap_hard(got["sym"].view(np.complex64), "16QAM"))
    check_against_contract(got, spread, None, rows, M, "16QAM", ("given", 1.0))


# ------------------------------------------------------------------------------------------ 3. planted cases
@pytest.mark.parametrize("mod", MODS)
def test_planted_cases(om, torch, rx0, mod):
    rng = np.random.default_rng(77 + BPS[mod])
    rows, M = 5, 60
    n, bps = rows * M, BPS[mod]
    sym, csi, sig = segments(rng, 6, rows, M, mod, extra=1)
    for j, a in zip((3, 11, 20), (0.0, np.nan, -1.0)):       # segment 0: unusable entries
        csi[0, j] = a
    for i, z in zip((5, 70, 140), (complex(np.nan, 0.1), complex(0.1, np.inf), complex(-np.inf, np.nan))):
        sym[1, i] = z                                        # segment 1: non-finite symbols in usable entries
    sym[2, 2 * M:3 * M] = 0                                  # segment 2: a zero row
    csi[3, :M] = 0                                           # segment 3: every entry unusable
    sig[4] = 1e300                                           # segment 4: the weight underflows float32, the symbols stay
    sig[5] = np.inf                                          # segment 5: nu is not finite
    noise = ("seg", sig)
    got = run(om, torch, rx0, sym, csi, rows, M, mod, noise)
    check_against_contract(got, sym, csi, rows, M, mod, noise)
    dsym = got["sym"].view(np.complex64).reshape(6, rows, M)
    llr = got["llr"].reshape(6, rows, M * bps)
    hb = got["bits"].reshape(6, rows, M * bps)
    zero_bits = np.tile(orc.demap_hard(np.zeros(1, np.complex64), mod), M)

    def erased(s, r):
        pz = not bits_of(dsym[s, r]).any() and not bits_of(llr[s, r]).any()                 # +0, sign included
        return pz and np.array_equal(hb[s, r], zero_bits)

    # masked entries are left out of the transform: the same as zeros in their place
    z0 = sym[0:1].copy()
    for j in (3, 11, 20):
        z0[0, j:n:M] = 0
    c0 = csi[0:1].copy()
    same = run(om, torch, rx0, z0, c0, rows, M, mod, ("seg", sig[0:1]))
    assert np.array_equal(bits_of(same["sym"]), bits_of(got["sym"][:2 * n]))
    assert erased(2, 2) and dsym[2, 1].any() and llr[2, 3].any()
    assert all(erased(3, r) for r in range(rows)) and got["beta"][3] == 0 and got["weight"][3] == 0
    assert got["weight"][4] == 0 and got["beta"][4] > 0 and dsym[4].all() and not bits_of(llr[4]).any()
    assert all(erased(5, r) for r in range(rows)) and got["beta"][5] == 0 and got["weight"][5] == 0
    assert got["beta"][1] > 0 and dsym[1].all()


def test_argument_errors_leave_the_outputs_untouched(om, torch, rx0):
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    sig = torch.ones(4, dtype=torch.float64, device="cuda")
    o = {k: Out(torch, 512, torch.uint8 if k == "bits" else torch.float32) for k in WANT_ALL}
    ok = dict(n_seg=2, rows=3, M=12, seg_stride=36, csi=d, csi_stride=12, rho=RHO, modulation="QPSK", noise_mode=om.DESPREAD_NOISE_RHO,
              noise_var=0.0, sigma2=None, bits_mode=om.BITS_UNPACKED)
    bad = (dict(M=7), dict(M=0), dict(M=4100), dict(n_seg=-1), dict(rows=-1), dict(seg_stride=35), dict(csi_stride=11),
           dict(modulation="BPSK"), dict(modulation=3), dict(noise_mode=3), dict(noise_mode=-1),
           dict(noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=0.0), dict(noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=float("nan")),
           dict(noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=float("inf")), dict(noise_mode=om.DESPREAD_NOISE_SEG),
           dict(rho=-1.0), dict(rho=float("inf")), dict(bits_mode=om.BITS_NONE), dict(bits_mode=7),
           dict(M=75, seg_stride=225, csi_stride=75, bits_mode=om.BITS_PACKED), dict(n_seg=1 << 32), dict(n_seg=1 << 20, seg_stride=1 << 30))
    for kw in bad:
        a = dict(ok, **kw)
        with pytest.raises(ValueError, match="ofdm_dft_despread_frames"):
            rx0.dft_despread_frames(d, a["n_seg"], a["rows"], a["M"], a["seg_stride"], a["csi"], a["csi_stride"], a["rho"], a["modulation"],
                                    d_sym_out=o["sym"].addr, d_llr=o["llr"].addr, d_bits=o["bits"].addr, bits_mode=a["bits_mode"],
                                    d_beta=o["beta"].addr, d_weight=o["weight"].addr, noise_mode=a["noise_mode"], noise_var=a["noise_var"],
                                    d_sigma2=a["sigma2"], stream=cur(torch))
    with pytest.raises(ValueError, match="no pointer"):
        rx0.dft_despread_frames(d, 2, 3, 12, 36, d, 12, RHO, "QPSK", stream=cur(torch))
    with pytest.raises(ValueError, match="seg_stride == rows"):
        rx0.dft_despread_frames(d, 2, 3, 12, 37, d, 12, RHO, "QPSK", d_sym_out=d, stream=cur(torch))
    with pytest.raises(ValueError, match="null d_sym"):
        rx0.dft_despread_frames(None, 2, 3, 12, 36, d, 12, RHO, "QPSK", d_sym_out=o["sym"].addr, stream=cur(torch))
    rx0.dft_despread_frames(d, 0, 3, 12, 36, d, 12, RHO, "QPSK", d_sym_out=o["sym"].addr, stream=cur(torch))     # zero counts: no-ops
    rx0.dft_despread_frames(d, 2, 0, 12, 0, d, 12, RHO, "QPSK", d_sym_out=o["sym"].addr, stream=cur(torch))
    rx0.dft_despread_frames(d, 2, 3, 12, 36, d, 12, RHO, "QPSK", d_beta=o["beta"].addr, noise_mode=om.DESPREAD_NOISE_SEG, d_sigma2=sig,
                            stream=cur(torch))                                                                    # the one good call
    bp = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100, modulation="BPSK")
    with pytest.raises(ValueError, match="ofdm_rx_demod_frames_despread"):
        bp.demod_frames_despread(d, 1, 32, 32, d, d_llr=o["llr"].addr)
    with pytest.raises(ValueError, match="needs d_eq"):
        rx0.demod_frames_despread(d, 1, 32, 32, None, d_llr=o["llr"].addr)
    torch.cuda.synchronize()
    assert all(o[k].untouched() for k in ("sym", "llr", "bits", "weight"))
    assert np.isfinite(o["beta"].read()[:2]).all()


# ------------------------------------------------------------------------------------------ 4. the composite calls
@pytest.mark.parametrize("N,mod,pilots", [(64, "QPSK", ()), (64, "16QAM", (-25, -15, -5, 5, 15, 25)), (1024, "64QAM", ())])
def test_modulate_frames_spread_equals_the_stage_calls(om, torch, N, mod, pilots):
    cp, K = GEOM[N]
    Kd, bps, L = K - len(pilots), BPS[mod], N + cp
    n_frames, n_sym = 3, 8
    rows = n_frames * 6
    tx = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    if pilots:
        tx.set_pilots(pilots, 1.0)
    rng = np.random.default_rng(N + bps)
    bits = rng.integers(0, 2, rows * Kd * bps).astype(np.uint8)
    d_bits = torch.from_numpy(bits).cuda()
    comp = Out(torch, n_frames * n_sym * L * 2, torch.float32)
    assert tx.modulate_frames_spread(d_bits, n_frames, n_sym, comp.addr, stream=cur(torch)) == n_frames * n_sym
    sym, grid = Out(torch, rows * Kd * 2, torch.float32), Out(torch, rows * N * 2, torch.float32)
    time, chain = Out(torch, rows * L * 2, torch.float32), Out(torch, n_frames * n_sym * L * 2, torch.float32)
    s = cur(torch)
    tx.map(d_bits, rows * Kd, sym.addr, stream=s)
    tx.dft_spread(sym.addr, rows, Kd, sym.addr, stream=s)
    tx.grid(sym.addr, rows, grid.addr, stream=s)
    tx.ifft_cp(grid.addr, rows, time.addr, stream=s)
    assert tx.mux(time.addr, rows, chain.addr, stream=s) == n_frames * n_sym
    got = comp.read()
    assert np.array_equal(bits_of(got), bits_of(chain.read()))
    x = ref.spread(orc.map_bits(bits, mod).reshape(rows, Kd))
    want = orc.tx_stage_mux(orc.tx_stage_cp(orc.tx_stage_ifft(orc.tx_stage_grid(x, N, Kd, pilots, 1.0)), cp), N, cp, 23, 3, N - 2)
    assert relerr(got.view(np.complex64), want.ravel()) < TOL_MAX
    idle = Out(torch, 64, torch.float32)
    with pytest.raises(ValueError, match="multiple of S"):
        tx.modulate_frames_spread(d_bits, 1, 6, idle.addr)
    with pytest.raises(ValueError, match="frame_stride"):
        tx.modulate_frames_spread(d_bits, 1, 8, idle.addr, frame_stride=8 * L + 1)
    assert idle.untouched()


@pytest.mark.parametrize("N,mod", [(64, "QPSK"), (1024, "64QAM")])
def test_demod_frames_despread_equals_the_separate_calls(om, torch, N, mod):
    cp, Kd = GEOM[N]
    bps = BPS[mod]
    rng = np.random.default_rng(N + bps)
    iq = make_frames(N, mod, 4, 12, rng, no_sync=(1,), late=(2,))
    n, fl = iq.shape
    rx, d_iq, nds = demod(om, N, mod, iq)
    n_sym = n * nds * Kd

    def outs():
        return dict(sym=Out(torch, n_sym * 2, torch.float32), llr=Out(torch, n_sym * bps, torch.float32), bits=Out(torch, n_sym * bps, torch.uint8),
                    beta=Out(torch, n, torch.float32), weight=Out(torch, n, torch.float32))

    p_eq, p_tsr = Out(torch, n_sym * 2, torch.float32), Out(torch, n * 4, torch.int32)
    assert rx.demod_frames(d_iq, n, fl, fl, p_eq.addr, d_tsr=p_tsr.addr) == nds
    d_a = Out(torch, n * Kd, torch.float32)
    rx.csi_frames(n, d_a.addr)
    sig = torch.from_numpy(np.array([0.01, 0.02, 0.03, 0.04])).cuda()
    for mode, nv, ds in ((om.DESPREAD_NOISE_RHO, 0.0, None), (om.DESPREAD_NOISE_GIVEN, 0.02, None), (om.DESPREAD_NOISE_SEG, 0.0, sig)):
        a, b = outs(), outs()
        rx.dft_despread_frames(p_eq.addr, n, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, mod, a["sym"].addr, a["llr"].addr, a["bits"].addr,
                               om.BITS_UNPACKED, a["beta"].addr, a["weight"].addr, mode, nv, ds)
        c_eq, c_tsr = Out(torch, n_sym * 2, torch.float32), Out(torch, n * 4, torch.int32)
        r = rx.demod_frames_despread(d_iq, n, fl, fl, c_eq.addr, b["sym"].addr, b["llr"].addr, b["bits"].addr, om.BITS_UNPACKED,
                                     b["beta"].addr, b["weight"].addr, mode, nv, ds, d_tsr=c_tsr.addr)
        assert r == nds
        assert np.array_equal(bits_of(p_eq.read()), bits_of(c_eq.read())) and np.array_equal(p_tsr.read(), c_tsr.read())
        for k in a:
            assert np.array_equal(a[k].read().view(np.uint8), b[k].read().view(np.uint8)), (k, mode)
    # frame 1 has no sync, frame 2 ends in guard-failed rows: erasures, and the contract on the downloaded rows
    eq = p_eq.read().view(np.complex64).reshape(n, nds * Kd)
    csi = d_a.read().reshape(n, Kd)
    got = {k: v.read().copy() for k, v in b.items()}
    check_against_contract(got, eq, csi, nds, Kd, mod, ("seg", sig.cpu().numpy()), rho=rx.csi_rho)
    dsym = got["sym"].view(np.complex64).reshape(n, nds, Kd)
    assert got["beta"][1] == 0 and got["weight"][1] == 0 and not bits_of(dsym[1]).any()
    assert not bits_of(dsym[2, -1]).any() and dsym[2, 0].all() and got["beta"][2] > 0


def test_graph_capture_equals_eager(om, torch):
    N, mod = 1024, "16QAM"
    cp, Kd = GEOM[N]
    rng = np.random.default_rng(12)
    iq = make_frames(N, mod, 4, 8, rng)
    n, fl = iq.shape
    rx = om.RxEngine(8, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    rx.set_max_trials(0)
    nds = rx.data_symbols_per_frame(fl)
    rx.reserve(n)
    rx.reserve_despread(Kd, n - 1)                           # one frame short of the batch that is captured second
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                sym=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                llr=torch.zeros(n * nds * Kd * 4, dtype=torch.float32, device="cuda"),
                weight=torch.zeros(n, dtype=torch.float32, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(stream, frames):
        return rx.demod_frames_despread(d_iq, frames, fl, fl, outs["eq"], outs["sym"], outs["llr"], d_weight=outs["weight"],
                                        noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=0.02, stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream, n - 1)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["weight"][:n - 1] > 0).all()) and bool(eager["llr"].any())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream, n - 1)
        with pytest.raises(ValueError, match="ofdm_rx_reserve_despread"):
            call(torch.cuda.current_stream().cuda_stream, n)  # a larger batch: the workspace would have to grow
        with pytest.raises(ValueError, match="ofdm_rx_reserve_despread"):
            rx.dft_despread_frames(outs["eq"], 1, 1, 300, 300, None, 0, 0.0, mod, d_sym_out=outs["sym"],
                                   stream=torch.cuda.current_stream().cuda_stream)      # a plan the handle does not hold
    assert not outs["weight"].any()                          # capture enqueues nothing
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k


# ------------------------------------------------------------------------------------------ 5. the link, end to end on the device
def test_link_case_decodes_every_block(om, torch):
    """dft_spread_cases end to end: turbo_encode_frames -> modulate_frames_spread -> channel -> demod_frames_despread ->
    turbo_decode_frames gives every block back at the level test_dft_spread_ref_host.py fixed on the reference."""
    import dft_spread_cases as dc
    n, L = dc.N_FRAMES, dc.N + dc.CP
    txe = om.TxEngine(dc.N, dc.CP, dc.KS, dc.KD, (1, 3), dc.MOD)
    rxe = om.RxEngine(dc.N_SYM, dc.N, dc.CP, dc.KS, (1, 3), dc.KD, dc.SNR_ARG, dc.GATE, modulation=dc.MOD)
    rxe.set_max_trials(0)
    info = dc.info_bits()
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * dc.SEG_BITS)
    txe.turbo_encode_frames(d_info, n, 1, dc.K, dc.F1, dc.F2, d_coded, dc.SEG_BITS)
    fl_tx, fl = dc.N_SYM * L, dc.FRAME_LEN
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = dc.TAPS.astype(np.complex64)
    d_taps = om.DeviceBuffer(taps.nbytes).upload(taps)
    assert txe.modulate_frames_spread(d_coded, n, dc.N_SYM, d_tx) == n * dc.N_SYM
    txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx, fl, fl, noise_var=dc.NOISE_VAR, seed=dc.SEED_NOISE)
    assert rxe.data_symbols_per_frame(fl) == dc.N_DSYM
    d_eq = om.DeviceBuffer(n * dc.N_DSYM * dc.KD * 8)
    d_llr = om.DeviceBuffer(n * dc.SEG_BITS * 4)
    d_hard = om.DeviceBuffer(n * dc.SEG_BITS)
    d_beta = om.DeviceBuffer(n * 4)
    d_bits = om.DeviceBuffer(n * dc.K)
    assert rxe.demod_frames_despread(d_rx, n, fl, fl, d_eq, d_llr=d_llr, d_bits=d_hard, bits_mode=om.BITS_UNPACKED, d_beta=d_beta) == dc.N_DSYM
    assert (d_beta.download(np.float32, n) > 0).all(), "every frame should find its sync"
    rxe.turbo_decode_frames(d_llr, n, dc.SEG_BITS, 1, dc.K, dc.F1, dc.F2, dc.N_ITER, d_bits=d_bits)
    lost = int((d_bits.download(np.uint8, n * dc.K).reshape(n, 1, dc.K) != info).any(axis=(1, 2)).sum())
    n_coded = 3 * dc.K + 12
    hard = d_hard.download(np.uint8, n * dc.SEG_BITS).reshape(n, dc.SEG_BITS)[:, :n_coded]
    sent = d_coded.download(np.uint8, n * dc.SEG_BITS).reshape(n, dc.SEG_BITS)[:, :n_coded]
    rate = float(np.mean(hard != sent))
    print("blocks lost of %d: %d, undecoded bit error rate %.4f" % (n, lost, rate))
    assert lost == 0
    assert rate >= 0.01                                      # the decoder had work to do
