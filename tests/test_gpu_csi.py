"""Channel-state-weighted LLRs on the GPU (-m gpu): ofdm_demap_csi_frames, ofdm_rx_csi_frames and ofdm_rx_demod_frames_csi
against tests/csi_ref.py (the contract of include/ofdm_mi355x.h in NumPy float32, pinned by test_csi_ref_host.py).  Every LLR
comparison is array_equal on the bit patterns, every output sits between poisoned guard bands, and the shapes are the smallest
at which the kernels take another path: odd rows, a tail shorter than one vector, a slice boundary inside a row, the 64-QAM
tile of 128 symbols with remainders 1 and 127."""
import math

import numpy as np
import pytest

import csi_cases as cc
import csi_ref
from oracle import ofdm_oracle as orc
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

MODS = ("QPSK", "16QAM", "64QAM")
BPS = csi_ref.BPS
SHAPES = [(1, 2), (1, 57), (3, 57), (9, 60), (2, 63), (5, 600), (4, 1200)]          # (rows, row_len)
RHO = 0.03
GUARD = 8                                                                            # elements of poison on either side


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


def cur(torch):
    return torch.cuda.current_stream().cuda_stream


class Out:
    """n elements between two bands of poison (NaN; 85 for bytes, -7777 for wider integers)"""

    def __init__(self, torch, n, dtype):
        self.poison = float("nan") if dtype.is_floating_point else 85 if dtype == torch.uint8 else -7777
        self.torch = torch
        self.t = torch.full((n + 2 * GUARD,), self.poison, dtype=dtype, device="cuda")
        torch.cuda.synchronize()                             # the library may write from a stream of its own
        self.n = n
        self.addr = self.t.data_ptr() + GUARD * self.t.element_size()

    def read(self):
        self.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        for band in (h[:GUARD], h[GUARD + self.n:]):
            assert (np.isnan(band) if band.dtype.kind == "f" else band == self.poison).all(), "wrote outside its output"
        return h[GUARD:GUARD + self.n]

    def untouched(self):
        self.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        return bool((np.isnan(h) if h.dtype.kind == "f" else h == self.poison).all())


def segments(rng, n_seg, rows, row_len, mod, extra=0, csi_extra=3, noise=(0.002, 0.005, 0.01)):
    """-> sym [n_seg][rows*row_len + extra] complex64 (NaN in the gap), csi [n_seg][row_len + csi_extra] float32 (NaN in the gap):
    constellation points through a one-tap MMSE equaliser, segment s with noise variance noise[s % 3]"""
    n = rows * row_len
    sym = np.full((n_seg, n + extra), complex(np.nan, np.nan), np.complex64)
    csi = np.full((n_seg, row_len + csi_extra), np.nan, np.float32)
    for s in range(n_seg):
        a = rng.uniform(0.02, 2.0, row_len)
        x = orc.map_bits(rng.integers(0, 2, n * BPS[mod]), mod).reshape(rows, row_len)
        w = (rng.standard_normal((rows, row_len)) + 1j * rng.standard_normal((rows, row_len))) * math.sqrt(noise[s % 3] / 2)
        sym[s, :n] = ((a / (a + RHO)) * (x + w / np.sqrt(a))).ravel()
        csi[s, :row_len] = a
    return sym, csi


def run(om, torch, rx, sym, csi, rows, row_len, mod, noise_var=None, want=("llr", "sigma2", "n_used"), base_off=0, rho=RHO,
        n_seg=None, first=0):
    """demap_csi_frames on host arrays -> dict of host arrays.  base_off: bytes the symbols are moved off the 16-byte grid."""
    n_seg = sym.shape[0] if n_seg is None else n_seg
    bps = BPS[mod]
    t = torch.zeros(sym.size * 2 + 4, dtype=torch.float32, device="cuda")
    t[base_off // 4:base_off // 4 + sym.size * 2] = torch.from_numpy(np.ascontiguousarray(sym).view(np.float32).ravel()).cuda()
    d_csi = torch.from_numpy(np.ascontiguousarray(csi)).cuda()
    o = dict(llr=Out(torch, n_seg * rows * row_len * bps, torch.float32) if "llr" in want else None,
             sigma2=Out(torch, n_seg, torch.float64) if "sigma2" in want else None,
             n_used=Out(torch, n_seg, torch.int64) if "n_used" in want else None)
    rx.demap_csi_frames(t.data_ptr() + base_off + 8 * first * sym.shape[1], n_seg, rows, row_len, sym.shape[1],
                        d_csi.data_ptr() + 4 * first * csi.shape[1], csi.shape[1], rho, mod,
                        d_llr=o["llr"].addr if o["llr"] else None, d_sigma2=o["sigma2"].addr if o["sigma2"] else None,
                        d_n_used=o["n_used"].addr if o["n_used"] else None,
                        noise_mode=om.CSI_NOISE_EST if noise_var is None else om.CSI_NOISE_GIVEN,
                        noise_var=0.0 if noise_var is None else noise_var, stream=cur(torch))
    torch.cuda.synchronize()
    return {k: (v.read().copy() if v else None) for k, v in o.items()}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def reference(sym, csi, rows, row_len, mod, noise_var=None, rho=RHO):
    n = rows * row_len
    return [csi_ref.demap_csi_segment(sym[s, :n].reshape(rows, row_len), csi[s, :row_len], rho, mod, noise_var) for s in range(sym.shape[0])]


# ------------------------------------------------------------------------------------------ 1. given noise
@pytest.mark.parametrize("n_seg", [1, 3])
@pytest.mark.parametrize("rows,row_len", SHAPES)
@pytest.mark.parametrize("mod", MODS)
def test_given_noise_against_the_reference(om, torch, rx0, mod, rows, row_len, n_seg):
    rng = np.random.default_rng(1000 * rows + row_len + 7 * n_seg + BPS[mod])
    nv = 0.05
    for extra, base_off in ((0, 0), (1, 8)):                 # dense and 16-byte aligned; stride + 1 and 8-byte alignment only
        sym, csi = segments(rng, n_seg, rows, row_len, mod, extra=extra)
        ref = reference(sym, csi, rows, row_len, mod, nv)
        got = run(om, torch, rx0, sym, csi, rows, row_len, mod, nv, base_off=base_off)
        per = rows * row_len * BPS[mod]
        for s in range(n_seg):
            assert same_bits(got["llr"][s * per:(s + 1) * per], ref[s][0]), (s, extra)
            assert got["sigma2"][s] == nv and got["n_used"][s] == ref[s][2] == rows * row_len
        assert np.isfinite(got["llr"]).all()


@pytest.mark.parametrize("mod", MODS)
def test_each_output_alone(om, torch, rx0, mod):
    rng = np.random.default_rng(5 + BPS[mod])
    rows, row_len = 3, 57
    sym, csi = segments(rng, 3, rows, row_len, mod, extra=1)
    for nv in (None, 0.05):
        full = run(om, torch, rx0, sym, csi, rows, row_len, mod, nv)
        for k in ("llr", "sigma2", "n_used"):
            one = run(om, torch, rx0, sym, csi, rows, row_len, mod, nv, want=(k,))
            assert np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), (k, nv)
    idle = Out(torch, 16, torch.float32)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    rx0.demap_csi_frames(d, 0, 1, 2, 2, d, 2, RHO, mod, d_llr=idle.addr, stream=cur(torch))           # n_seg = 0
    rx0.demap_csi_frames(d, 1, 0, 2, 0, d, 2, RHO, mod, d_llr=idle.addr, stream=cur(torch))           # rows = 0
    rx0.demap_csi_frames(d, 1, 1, 2, 2, d, 2, RHO, mod, stream=cur(torch))                            # no output
    torch.cuda.synchronize()
    assert idle.untouched()


# ------------------------------------------------------------------------------------------ 2. estimated noise
@pytest.mark.parametrize("rows,row_len", [(3, 57), (9, 60), (5, 600), (4, 1200)])
@pytest.mark.parametrize("mod", MODS)
def test_estimated_noise(om, torch, rx0, mod, rows, row_len):
    rng = np.random.default_rng(rows * 31 + row_len + BPS[mod])
    n, per = rows * row_len, rows * row_len * BPS[mod]
    sym, csi = segments(rng, 3, rows, row_len, mod, extra=1)
    ref = reference(sym, csi, rows, row_len, mod)
    got = run(om, torch, rx0, sym, csi, rows, row_len, mod)
    for s in range(3):
        _, r_s2, r_n, terms = ref[s]
        assert got["n_used"][s] == r_n == n
        want = math.fsum(terms) / r_n
        assert abs(got["sigma2"][s] - want) <= r_n * 2.0 ** -52 * want, (s, got["sigma2"][s], want)
        mine = csi_ref.llr_with_sigma2(sym[s, :n].reshape(rows, row_len), csi[s, :row_len], RHO, mod, got["sigma2"][s])
        assert same_bits(got["llr"][s * per:(s + 1) * per], mine), s
    assert len(set(got["sigma2"])) == 3, "segments with different noise must get different sigma2"
    # the same segment alone, 8 bytes off the 16-byte grid, and dense: the same bits
    for s in (0, 1, 2):
        alone = run(om, torch, rx0, sym, csi, rows, row_len, mod, n_seg=1, first=s)
        moved = run(om, torch, rx0, sym[s:s + 1], csi[s:s + 1], rows, row_len, mod, base_off=8)
        dense = run(om, torch, rx0, np.ascontiguousarray(sym[s:s + 1, :n]), csi[s:s + 1], rows, row_len, mod)
        for other in (alone, moved, dense):
            assert same_bits(other["llr"], got["llr"][s * per:(s + 1) * per]), s
            assert other["sigma2"][0] == got["sigma2"][s] and other["n_used"][0] == got["n_used"][s]


# ------------------------------------------------------------------------------------------ 3. erasures
@pytest.mark.parametrize("mod", MODS)
def test_erasures(om, torch, rx0, mod):
    rng = np.random.default_rng(77 + BPS[mod])
    rows, row_len = 5, 57
    n, bps = rows * row_len, BPS[mod]
    sym, csi = segments(rng, 4, rows, row_len, mod, extra=1)
    sym[0, 2 * row_len:3 * row_len] = 0                      # a guard-failed row
    csi[1, :row_len] = 0                                     # a frame without a sync
    for j, a in zip((3, 11, 20, 31), (np.nan, np.inf, -1.0, 1e-42)):
        csi[2, j] = a
    for i, z in zip((5, 70, 140), (complex(np.nan, 0.1), complex(0.1, np.inf), complex(3e38, 0.1))):
        sym[3, i] = z
    csi[3, 140 % row_len] = 0.1                              # s = 1.3: u = 3e38 * 1.3 overflows
    for nv in (None, 0.05):
        ref = reference(sym, csi, rows, row_len, mod, nv)
        got = run(om, torch, rx0, sym, csi, rows, row_len, mod, nv)
        assert np.isfinite(got["llr"]).all() and np.isfinite(got["sigma2"]).all()
        llr = got["llr"].reshape(4, n, bps)
        for s in range(4):
            assert got["n_used"][s] == ref[s][2], (s, nv)
            sig = got["sigma2"][s]
            assert sig == nv if nv else abs(sig - ref[s][1]) <= max(ref[s][2], 1) * 2.0 ** -52 * ref[s][1]
            mine = csi_ref.llr_with_sigma2(sym[s, :n].reshape(rows, row_len), csi[s, :row_len], RHO, mod, sig)
            assert same_bits(llr[s].ravel(), mine), (s, nv)
        zero = lambda v: not v.any() and not np.signbit(v).any()                                       # noqa: E731
        assert zero(llr[0, 2 * row_len:3 * row_len]) and got["n_used"][0] == n - row_len
        assert zero(llr[1]) and got["n_used"][1] == 0 and (nv or got["sigma2"][1] == 0.0)
        assert all(zero(llr[2, j::row_len]) for j in (3, 11, 20, 31)) and got["n_used"][2] == n - 4 * rows
        assert all(zero(llr[3, i]) for i in (5, 70, 140)) and got["n_used"][3] == n - 3
        assert llr[2, 4].any() and llr[3, 6].any()


# ------------------------------------------------------------------------------------------ 4. |H|^2 rows of the last demod
def demod(om, N, mod, iq, pilots=(), snr=30):
    cp, Kd = GEOM[N]
    n, fl = iq.shape
    rx = om.RxEngine(max(fl // (N + cp), 4), N, cp, N - 2, (1, 3), Kd, snr, 0.7, modulation=mod)
    rx.set_max_trials(0)
    if pilots:
        rx.set_pilots(pilots, 1.0)
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    return rx, d_iq, rx.data_symbols_per_frame(fl)


@pytest.mark.parametrize("N", [64, 1024])
def test_csi_frames(om, torch, N):
    cp, Kd = GEOM[N]
    rng = np.random.default_rng(N)
    iq = make_frames(N, "QPSK", 4, 8, rng, no_sync=(2,))
    pilots = [-21, -7, 7, 21]
    rx, d_iq, nds = demod(om, N, "QPSK", iq, pilots)
    d_eq = om.DeviceBuffer(4 * nds * Kd * 8)
    d_tsr = om.DeviceBuffer(4 * 16)
    assert rx.demod_frames(d_iq, 4, iq.shape[1], iq.shape[1], d_eq, d_tsr=d_tsr) == nds
    tsr = d_tsr.download(np.int32, 16).reshape(4, 4)
    assert list(tsr[:, 3] != 0) == [True, True, False, True]
    bins = om.bins_p(Kd, N)
    keep = np.array([i for i in range(Kd) if (i - Kd // 2 if i < Kd // 2 else i - Kd // 2 + 1) not in pilots])
    assert keep.size == Kd - 4
    for layout, sel in ((om.CSI_ROWS_ALL, np.arange(Kd)), (om.CSI_ROWS_DATA, keep)):
        stride = sel.size + 5
        out = Out(torch, 4 * stride, torch.float32)
        rx.csi_frames(4, out.addr, stride, layout)
        got = out.read().reshape(4, stride)
        assert np.isnan(got[:, sel.size:]).all(), "wrote into the gap"
        for f in range(4):
            want = csi_ref.csi_row(rx.frame_state(f)["chan_freq"], bins[sel])
            assert same_bits(got[f, :sel.size], want), (layout, f)
        assert not got[2, :sel.size].any() and got[0, :sel.size].all()
        dense = Out(torch, 2 * sel.size, torch.float32)
        rx.csi_frames(2, dense.addr, layout=layout)                                   # fewer frames, default stride
        assert same_bits(dense.read().reshape(2, -1), got[:2, :sel.size])
    idle = Out(torch, 8, torch.float32)
    with pytest.raises(ValueError, match="last ofdm_rx_demod_frames call"):
        rx.csi_frames(5, idle.addr, Kd)
    with pytest.raises(ValueError):
        rx.csi_frames(1, idle.addr, Kd - 1)
    rx.set_pilots([])
    with pytest.raises(ValueError, match="pilots"):
        rx.csi_frames(1, idle.addr, Kd, om.CSI_ROWS_DATA)
    assert idle.untouched()


# ------------------------------------------------------------------------------------------ 5. the composite call
@pytest.mark.parametrize("N,mod", [(64, "QPSK"), (1024, "64QAM")])
def test_composite_equals_the_separate_calls(om, torch, N, mod):
    cp, Kd = GEOM[N]
    bps = BPS[mod]
    rng = np.random.default_rng(N + bps)
    iq = make_frames(N, mod, 4, 12, rng, no_sync=(1,), late=(2,))
    n, fl = iq.shape
    rx, d_iq, nds = demod(om, N, mod, iq)
    n_eq, n_b = n * nds * Kd, n * nds * Kd * bps

    def bufs():
        return dict(eq=Out(torch, n_eq * 2, torch.float32), bits=Out(torch, n_b, torch.uint8), tsr=Out(torch, n * 4, torch.int32))

    p, c = bufs(), bufs()
    assert rx.demod_frames(d_iq, n, fl, fl, p["eq"].addr, p["bits"].addr, om.BITS_UNPACKED, p["tsr"].addr) == nds
    d_a = Out(torch, n * Kd, torch.float32)
    rx.csi_frames(n, d_a.addr)
    sep = {}
    for nv in (None, 0.02):
        o = dict(llr=Out(torch, n_b, torch.float32), sigma2=Out(torch, n, torch.float64), n_used=Out(torch, n, torch.int64))
        rx.demap_csi_frames(p["eq"].addr, n, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, mod, o["llr"].addr, o["sigma2"].addr,
                            o["n_used"].addr, om.CSI_NOISE_EST if nv is None else om.CSI_NOISE_GIVEN, nv or 0.0)
        sep[nv] = {k: v.read().copy() for k, v in o.items()}
        o = dict(llr=Out(torch, n_b, torch.float32), sigma2=Out(torch, n, torch.float64), n_used=Out(torch, n, torch.int64))
        r = rx.demod_frames_csi(d_iq, n, fl, fl, c["eq"].addr, o["llr"].addr, o["sigma2"].addr, o["n_used"].addr,
                                om.CSI_NOISE_EST if nv is None else om.CSI_NOISE_GIVEN, nv or 0.0, d_bits=c["bits"].addr,
                                bits_mode=om.BITS_UNPACKED, d_tsr=c["tsr"].addr)
        assert r == nds
        for k in ("eq", "bits", "tsr"):
            assert np.array_equal(p[k].read().view(np.uint8), c[k].read().view(np.uint8)), k
        for k, v in o.items():
            assert np.array_equal(v.read().view(np.uint8), sep[nv][k].view(np.uint8)), (k, nv)
    # against the reference on the downloaded symbols; frame 1 has no sync, frame 2 ends in guard-failed rows
    eq = p["eq"].read().view(np.complex64).reshape(n, nds, Kd)
    a = d_a.read().reshape(n, Kd)
    tsr = p["tsr"].read().reshape(n, 4)
    assert tsr[1, 3] == 0 and not eq[1].any() and tsr[2, 3] and not eq[2, -1].any() and eq[2, 0].any()
    est = sep[None]
    llr = est["llr"].reshape(n, nds, Kd * bps)
    assert est["n_used"][1] == 0 and est["sigma2"][1] == 0.0 and not llr[1].any()
    assert not llr[2, -1].any() and not np.signbit(llr[2, -1]).any() and llr[2, 0].any()
    assert est["n_used"][0] == nds * Kd and est["n_used"][2] == (nds - 3) * Kd          # the last pattern's three rows
    for f in range(n):
        mine = csi_ref.llr_with_sigma2(eq[f], a[f], rx.csi_rho, mod, est["sigma2"][f])
        assert same_bits(llr[f].ravel(), mine), f
        assert est["n_used"][f] == csi_ref.demap_csi_segment(eq[f], a[f], rx.csi_rho, mod)[2]
    with pytest.raises(ValueError, match="needs d_eq"):
        rx.demod_frames_csi(d_iq, n, fl, fl, None, d_llr=c["eq"].addr)


def test_pilot_chain(om, torch):
    """demod_frames_pilots -> csi_frames(CSI_ROWS_DATA) -> demap_csi_frames over the tracked data"""
    N, mod, pilots = 64, "16QAM", [-21, -7, 7, 21]
    cp, K = GEOM[N]
    Kd, bps = K - len(pilots), BPS[mod]
    rng = np.random.default_rng(9)
    iq = make_frames(N, mod, 3, 8, rng)
    n, fl = iq.shape
    rx, d_iq, nds = demod(om, N, mod, iq, pilots)
    d_eq, d_data = Out(torch, n * nds * K * 2, torch.float32), Out(torch, n * nds * Kd * 2, torch.float32)
    assert rx.demod_frames_pilots(d_iq, n, fl, fl, d_eq.addr, d_data=d_data.addr) == nds
    d_a = Out(torch, n * Kd, torch.float32)
    rx.csi_frames(n, d_a.addr, layout=om.CSI_ROWS_DATA)
    o = dict(llr=Out(torch, n * nds * Kd * bps, torch.float32), sigma2=Out(torch, n, torch.float64), n_used=Out(torch, n, torch.int64))
    rx.demap_csi_frames(d_data.addr, n, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, mod, o["llr"].addr, o["sigma2"].addr,
                        o["n_used"].addr)
    data = d_data.read().view(np.complex64).reshape(n, nds, Kd)
    a = d_a.read().reshape(n, Kd)
    sig, used = o["sigma2"].read(), o["n_used"].read()
    llr = o["llr"].read().reshape(n, -1)
    for f in range(n):
        _, r_s2, r_n, _ = csi_ref.demap_csi_segment(data[f], a[f], rx.csi_rho, mod)
        assert used[f] == r_n == nds * Kd and abs(sig[f] - r_s2) <= r_n * 2.0 ** -52 * r_s2
        assert same_bits(llr[f], csi_ref.llr_with_sigma2(data[f], a[f], rx.csi_rho, mod, sig[f])), f


# ------------------------------------------------------------------------------------------ 6. graph capture, argument errors
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
    rx.reserve_csi(n - 1, nds, Kd)                           # one frame short of the batch that is captured second
    d_iq = torch.from_numpy(iq.view(np.float32)).cuda()
    outs = dict(eq=torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda"),
                llr=torch.zeros(n * nds * Kd * 4, dtype=torch.float32, device="cuda"),
                sigma2=torch.zeros(n, dtype=torch.float64, device="cuda"), n_used=torch.zeros(n, dtype=torch.int64, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(stream, frames):
        return rx.demod_frames_csi(d_iq, frames, fl, fl, outs["eq"], outs["llr"], outs["sigma2"], outs["n_used"], stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream, n - 1)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["sigma2"][:n - 1] > 0).all()) and bool((eager["n_used"][:n - 1] == nds * Kd).all())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream, n - 1)
        with pytest.raises(ValueError, match="ofdm_rx_reserve_csi"):
            call(torch.cuda.current_stream().cuda_stream, n)  # a larger batch: the workspace would have to grow
    assert not outs["sigma2"].any()                          # capture enqueues nothing
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k


def test_argument_errors_leave_the_outputs_untouched(om, torch, rx0):
    d = torch.zeros(256, dtype=torch.float32, device="cuda")
    o = Out(torch, 64, torch.float32)
    sg, nu = Out(torch, 4, torch.float64), Out(torch, 4, torch.int64)
    ok = dict(n_seg=2, rows=3, row_len=4, seg_stride=12, csi_stride=4, rho=RHO, modulation="QPSK", noise_mode=om.CSI_NOISE_EST,
              noise_var=0.0)
    for kw in (dict(n_seg=-1), dict(rows=-1), dict(seg_stride=11), dict(csi_stride=3), dict(modulation="BPSK"), dict(modulation=3),
               dict(noise_mode=2), dict(noise_mode=om.CSI_NOISE_GIVEN, noise_var=0.0), dict(noise_mode=om.CSI_NOISE_GIVEN, noise_var=-1.0),
               dict(noise_mode=om.CSI_NOISE_GIVEN, noise_var=float("nan")), dict(rho=-1.0), dict(rho=float("inf")),
               dict(n_seg=1 << 32), dict(n_seg=1 << 20, seg_stride=1 << 30)):
        a = dict(ok, **kw)
        with pytest.raises(ValueError, match="ofdm_demap_csi_frames"):
            rx0.demap_csi_frames(d, a["n_seg"], a["rows"], a["row_len"], a["seg_stride"], d, a["csi_stride"], a["rho"], a["modulation"],
                                 o.addr, sg.addr, nu.addr, a["noise_mode"], a["noise_var"], stream=cur(torch))
    with pytest.raises(ValueError):
        rx0.demap_csi_frames(None, 2, 3, 4, 12, d, 4, RHO, "QPSK", o.addr)
    with pytest.raises(ValueError):
        rx0.reserve_csi(-1, 1, 1)
    bp = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100, modulation="BPSK")
    with pytest.raises(ValueError, match="ofdm_rx_demod_frames_csi"):
        bp.demod_frames_csi(d, 1, 32, 32, d, d_llr=o.addr)
    torch.cuda.synchronize()
    assert o.untouched() and sg.untouched() and nu.untouched()


# ------------------------------------------------------------------------------------------ 7. the link, end to end on the device
def test_chain_decodes_where_the_per_frame_sigma_llrs_do_not(om, torch):
    """csi_cases end to end: turbo_encode_frames -> modulate_frames -> channel -> demod_frames_csi -> turbo_decode_frames gives
    every block back; the same frames through demod_frames_soft's llr lose at least one (the host test guarantees 8 for the
    oracle's receiver on the same noise samples; 1 leaves room for float32 differences)."""
    n, L = cc.N_FRAMES, cc.N + cc.CP
    txe = om.TxEngine(cc.N, cc.CP, cc.KS, cc.KD, (1, 3), cc.MOD)
    rxe = om.RxEngine(cc.N_SYM, cc.N, cc.CP, cc.KS, (1, 3), cc.KD, cc.SNR_ARG, cc.GATE, modulation=cc.MOD)
    rxe.set_max_trials(0)
    info = cc.info_bits()
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * cc.SEG_BITS)
    txe.turbo_encode_frames(d_info, n, 1, cc.K, cc.F1, cc.F2, d_coded, cc.SEG_BITS)
    fl_tx, fl = cc.N_SYM * L, cc.FRAME_LEN
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = cc.TAPS.astype(np.complex64)
    d_taps = om.DeviceBuffer(taps.nbytes).upload(taps)
    txe.modulate_frames(d_coded, n, cc.N_SYM, d_tx)
    txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx, fl, fl, noise_var=cc.NOISE_VAR, seed=cc.SEED_NOISE)
    assert rxe.data_symbols_per_frame(fl) == cc.N_DSYM
    d_eq = om.DeviceBuffer(n * cc.N_DSYM * cc.KD * 8)
    d_llr = om.DeviceBuffer(n * cc.SEG_BITS * 4)
    d_used = om.DeviceBuffer(n * 8)
    d_bits = om.DeviceBuffer(n * cc.K)
    lost = {}
    assert rxe.demod_frames_csi(d_rx, n, fl, fl, d_eq, d_llr, d_n_used=d_used) == cc.N_DSYM
    assert (d_used.download(np.int64, n) == cc.N_DSYM * cc.KD).all(), "every frame should find its sync"
    rxe.turbo_decode_frames(d_llr, n, cc.SEG_BITS, 1, cc.K, cc.F1, cc.F2, cc.N_ITER, d_bits=d_bits)
    lost["csi"] = int((d_bits.download(np.uint8, n * cc.K).reshape(n, 1, cc.K) != info).any(axis=(1, 2)).sum())
    assert rxe.demod_frames_soft(d_rx, n, fl, fl, d_eq, d_llr=d_llr) == cc.N_DSYM
    rxe.turbo_decode_frames(d_llr, n, cc.SEG_BITS, 1, cc.K, cc.F1, cc.F2, cc.N_ITER, d_bits=d_bits)
    lost["per-frame sigma"] = int((d_bits.download(np.uint8, n * cc.K).reshape(n, 1, cc.K) != info).any(axis=(1, 2)).sum())
    print("wrong blocks of %d: %r" % (n, lost))
    assert lost["csi"] == 0
    assert lost["per-frame sigma"] >= 1
