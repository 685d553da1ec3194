"""The second trip of every capped launch on the GPU (-m gpu).  Many launchers cap their grid and let the kernel loop with the grid
as stride, and some host functions cut a batch into parts of 65 535; tests/grid_cap_cases.py holds, for each of them that no
other test drives past its cap, the smallest shape that loops (tests/test_grid_caps_host.py pins those shapes to the caps in the
sources).  Every result is held by a chain of two links:

  1. the capped launch equals, bit for bit over every output byte and the poisoned guard bands around it, the same buffers
     pushed through launches that stay below every cap (compared on the device, on integer views);
  2. the sub-cap results are held to the kernel's reference with the comparison the kernel's own GPU test uses -- on every
     segment where the reference is one flat call, else on the fixed sample of grid_cap_cases.sample(): the first two segments,
     the last two, the two on either side of every multiple of the cap and 1 000 seeded random ones.

Large inputs are drawn on the device from a seeded generator, every segment with data of its own; the sampled segments of the
CSI, MRC and soft de-mapper batches are the ones grid_cap_cases makes on the CPU, with erasures next to the cap multiples.
Every capped shape is launched once per test; the library runs on its handles' own streams, so the tests wait for their own
device work before the first launch and for the launches before they read (settle)."""
import gc as _gc
import math
import time

import numpy as np
import pytest

import csi_ref
import grid_cap_cases as gc
import lte_bits_ref as lb
import mrc_ref
import tb_cases as tc
import tb_ref
from conftest import relerr
from oracle import ofdm_oracle as orc
from test_gpu_soft_frames import check_segment

pytestmark = pytest.mark.gpu

MODS, BPS, RHO = gc.MODS, gc.BPS, gc.RHO
GUARD = 64                                                                               # elements of poison on either side
NV = 0.05                                                                                # OFDM_CSI_NOISE_GIVEN
_CACHE = {}


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
def rx0(om, torch):
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


@pytest.fixture(scope="module", autouse=True)
def drop_the_cached_inputs(torch):
    yield
    _CACHE.clear()
    _gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def wall_time_and_memory(request, torch):
    """prints what the issue asks to be reported, and gives the large buffers back before the next test"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\n[grid caps] %s: %.2f s, peak of the test's own device buffers %.0f MiB"
          % (request.node.name, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2 ** 20))
    _gc.collect()
    torch.cuda.empty_cache()


def cur(torch):
    return torch.cuda.current_stream().cuda_stream


def settle(torch):
    """torch's default stream has the handle 0, which the library reads as "the handle's own stream": its launches are not ordered
    behind the test's fills, draws and copies.  Those have to land before the first launch, and the launches before a read."""
    torch.cuda.synchronize()


def gen(torch, seed):
    return torch.Generator(device="cuda").manual_seed(int(seed))


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


class Buf:
    """n elements on the device between two bands of GUARD poisoned ones (NaN; 85 for bytes, -7777 for wider integers)"""

    def __init__(self, torch, n, dtype):
        self.torch, self.n, self.floating = torch, int(n), dtype.is_floating_point
        self.poison = float("nan") if self.floating else 85 if dtype == torch.uint8 else -7777
        self.t = torch.full((self.n + 2 * GUARD,), self.poison, dtype=dtype, device="cuda")
        self.body = self.t[GUARD:GUARD + self.n]
        self.addr, self.size = self.body.data_ptr(), self.t.element_size()

    def at(self, i):
        return self.addr + int(i) * self.size

    def ints(self, t=None):
        t = self.t if t is None else t
        return t.view({1: self.torch.uint8, 4: self.torch.int32, 8: self.torch.int64}[self.size])

    def is_poison(self, t):
        return self.torch.isnan(t) if self.floating else t == self.poison

    def bands_ok(self):
        return bool(self.is_poison(self.t[:GUARD]).all()) and bool(self.is_poison(self.t[GUARD + self.n:]).all())

    def filled(self):
        """no element of the body is still poison (outputs are finite floats, bits or counts)"""
        return not bool(self.is_poison(self.body).any())

    def same(self, other):
        """bit for bit, guard bands included"""
        return self.torch.equal(self.ints(), other.ints())

    def holds(self, expected):
        """the body equals `expected` (a tensor of the same type) bit for bit and the bands are poison"""
        return self.bands_ok() and self.torch.equal(self.ints(self.body), self.ints(expected.reshape(-1)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def link1(big, small, packed=()):
    """the capped launch against the sub-cap launches: every byte, the bands, and nothing left unwritten"""
    for k in big:
        assert big[k].bands_ok() and small[k].bands_ok(), "%s: wrote outside its output" % k
        assert big[k].same(small[k]), "%s: the capped launch differs from the sub-cap launches" % k
        assert k in packed or big[k].filled(), "%s: elements left unwritten" % k


def draw_points(torch, g, shape, mod):
    """constellation points [*shape][2] float32 on the device, from the library's float32 levels"""
    lv = dev(torch, csi_ref.levels(BPS[mod])[0].astype(np.float32))
    pick = torch.randint(0, lv.numel(), tuple(shape) + (2,), generator=g, device="cuda")
    return lv[pick]


def mmse_symbols(torch, g, a, x, nv):
    """a / (a + rho) * (x + w / sqrt(a)), w complex noise of variance nv: the equalised symbols tests/test_gpu_csi.py draws"""
    w = torch.randn(x.shape, generator=g, device="cuda") * torch.sqrt(nv / 2)
    return ((a / (a + RHO)).unsqueeze(-1) * (x + w / torch.sqrt(a).unsqueeze(-1))).contiguous()


def planted(torch, bulk, di, rows):
    """the CPU-made sample written over the bulk's rows di; read back, it is the sample bit for bit"""
    rows = dev(torch, rows).reshape((di.numel(),) + tuple(bulk.shape[1:]))
    bulk[di] = rows
    itype = {4: torch.int32, 8: torch.int64}[bulk.element_size()]
    assert torch.equal(bulk[di].view(itype), rows.view(itype))


# ------------------------------------------------------------------------------------------ 1. channel-state-weighted LLRs
CSI_WANTS = (("llr", "sigma2", "n_used"), ("llr",), ("sigma2",), ("n_used",))
CSI_TYPES = dict(llr="float32", sigma2="float64", n_used="int64")


def csi_input(torch, mod):
    key = ("csi", mod)
    if key not in _CACHE:
        n, rl = gc.N_SEG, gc.ROW_LEN
        idx, s_sym, s_csi = gc.csi_sample(mod)
        g = gen(torch, 100 + BPS[mod])
        a = 0.02 + 1.98 * torch.rand((n, rl), generator=g, device="cuda")
        nv = dev(torch, np.array((0.002, 0.005, 0.01), np.float32))[torch.arange(n, device="cuda") % 3].view(n, 1, 1)
        sym = mmse_symbols(torch, g, a, draw_points(torch, g, (n, rl), mod), nv)        # [n][3][2]: seg_stride = 3
        csi = torch.full((n, gc.CSI_STRIDE), float("nan"), dtype=torch.float32, device="cuda")
        csi[:, :rl] = a
        di = dev(torch, idx)
        planted(torch, sym, di, s_sym.view(np.float32))
        planted(torch, csi, di, s_csi)
        _CACHE[key] = dict(sym=sym, csi=csi, di=di)
    return _CACHE[key]


def csi_outs(torch, n_seg, seg_len, mod, want):
    size = dict(llr=n_seg * seg_len * BPS[mod], sigma2=n_seg, n_used=n_seg)
    return {k: Buf(torch, size[k], getattr(torch, CSI_TYPES[k])) for k in want}


def csi_call(om, torch, rx, sym, csi, first, count, rows, row_len, seg_stride, csi_stride, mod, given, out, first_out=None):
    """demap_csi_frames over segments first .. first + count - 1 of the buffers, into the outputs at segment first_out"""
    fo = first if first_out is None else first_out
    per = rows * row_len * BPS[mod]
    rx.demap_csi_frames(sym.data_ptr() + 8 * seg_stride * first, count, rows, row_len, seg_stride, csi.data_ptr() + 4 * csi_stride * first,
                        csi_stride, RHO, mod, d_llr=out["llr"].at(fo * per) if "llr" in out else None,
                        d_sigma2=out["sigma2"].at(fo) if "sigma2" in out else None, d_n_used=out["n_used"].at(fo) if "n_used" in out else None,
                        noise_mode=om.CSI_NOISE_GIVEN if given else om.CSI_NOISE_EST, noise_var=NV if given else 0.0, stream=cur(torch))


def csi_est_reference(om, torch, rx, mod):
    """OFDM_CSI_NOISE_EST on the sample alone (one sub-cap launch of its 1 0xx segments, every output), held to csi_ref as
    tests/test_gpu_csi.py::test_estimated_noise holds it -> the outputs, which the batch must repeat bit for bit"""
    key = ("csi est", mod)
    if key not in _CACHE:
        idx, s_sym, s_csi = gc.csi_sample(mod)
        k, rl = idx.size, gc.ROW_LEN
        out = csi_outs(torch, k, rl, mod, CSI_WANTS[0])
        d_sym, d_csi = dev(torch, s_sym.view(np.float32)), dev(torch, s_csi)
        settle(torch)
        csi_call(om, torch, rx, d_sym, d_csi, 0, k, 1, rl, gc.SEG_STRIDE, gc.CSI_STRIDE, mod, False, out)
        torch.cuda.synchronize()
        assert all(b.bands_ok() and b.filled() for b in out.values())
        got = {name: b.body.cpu().numpy() for name, b in out.items()}
        llr = got["llr"].reshape(k, -1)
        for i in range(k):
            _, _, r_n, terms = csi_ref.demap_csi_segment(s_sym[i][None], s_csi[i, :rl], RHO, mod)
            assert got["n_used"][i] == r_n, idx[i]
            want = math.fsum(terms) / r_n if r_n else 0.0
            assert abs(got["sigma2"][i] - want) <= max(r_n, 1) * 2.0 ** -52 * want, (idx[i], got["sigma2"][i], want)
            assert same_bits(llr[i], csi_ref.llr_with_sigma2(s_sym[i][None], s_csi[i, :rl], RHO, mod, got["sigma2"][i])), idx[i]
        zero = gc._at(idx, gc.CSI_GRID_CAP)
        assert got["n_used"][zero] == 0 and got["sigma2"][zero] == 0.0 and not llr[zero].view(np.uint32).any()
        assert (got["n_used"] == rl).sum() >= k - 5 and np.isfinite(llr).all()
        _CACHE[key] = got
    return _CACHE[key]


def csi_given_reference(torch, inp, mod):
    """OFDM_CSI_NOISE_GIVEN: an LLR depends on its own symbol only, so csi_ref runs flat over all 1.57 M symbols -> LLRs, counts"""
    key = ("csi given", mod)
    if key not in _CACHE:
        rl = gc.ROW_LEN
        z = inp["sym"].cpu().numpy().view(np.complex64).ravel()
        a = inp["csi"][:, :rl].cpu().numpy().ravel()
        usable, d, _, _ = csi_ref.symbols(z, a, RHO, mod)
        _CACHE[key] = (csi_ref.llr_from(usable, d, a, NV).ravel(), usable.reshape(-1, rl).sum(axis=1).astype(np.int64))
    return _CACHE[key]


@pytest.mark.parametrize("want", CSI_WANTS, ids=("all", "llr", "sigma2", "n_used"))
@pytest.mark.parametrize("given", (False, True), ids=("est", "given"))
@pytest.mark.parametrize("mod", MODS)
def test_demap_csi_frames_past_the_grid_cap(om, torch, rx0, mod, given, want):
    """n_seg = 2 * 262144 + 5 = 524 293 segments of rows = 1, row_len = 3: one slice per segment, so csi_noise_kernel,
    csi_llr_kernel (<MOD, false>; <MOD, true> when the noise is given and n_used is wanted) and csi_finish_kernel all get
    524 293 items for a grid of CSI_GRID_CAP = 262 144 workgroups: every workgroup takes 2 trips, workgroups 0 .. 4 take 3.
    seg_stride = 3 (24 bytes): the segments of a looping workgroup are 262 144 * 24 bytes apart, a multiple of 16, but
    consecutive workgroups alternate between the 16-byte path and the per-float path.
    Link 1: five launches of at most 100 000 segments.  Link 2: noise given -- csi_ref flat over every segment; noise estimated
    -- the sample (its own sub-cap launch against csi_ref), with n_used = 0 planted in the first segment of the second trip."""
    n, rl, bps = gc.N_SEG, gc.ROW_LEN, BPS[mod]
    assert n * gc.seg_slices(rl) > gc.CSI_GRID_CAP
    inp = csi_input(torch, mod)
    big, small = csi_outs(torch, n, rl, mod, want), csi_outs(torch, n, rl, mod, want)
    settle(torch)
    csi_call(om, torch, rx0, inp["sym"], inp["csi"], 0, n, 1, rl, gc.SEG_STRIDE, gc.CSI_STRIDE, mod, given, big)
    for first, count in gc.parts(n, gc.SLICE_SEGS):
        csi_call(om, torch, rx0, inp["sym"], inp["csi"], first, count, 1, rl, gc.SEG_STRIDE, gc.CSI_STRIDE, mod, given, small)
    settle(torch)
    link1(big, small)
    if given:
        llr, used = csi_given_reference(torch, inp, mod)
        if "llr" in want:
            assert same_bits(small["llr"].body.cpu().numpy(), llr)
        if "sigma2" in want:
            assert bool((small["sigma2"].body == NV).all())
        if "n_used" in want:
            assert np.array_equal(small["n_used"].body.cpu().numpy(), used) and (used < rl).any() and (used == rl).any()
    else:
        ref = csi_est_reference(om, torch, rx0, mod)
        for k in want:
            got = small[k].body.view(n, -1)[inp["di"]].cpu().numpy()
            assert np.array_equal(got.ravel().view(np.uint8), ref[k].view(np.uint8)), k


def test_csi_table_kernel_past_its_cap(om, torch, rx0):
    """csi_table_kernel takes one thread per (segment, entry) on at most CSI_GRID_CAP * 256 = 2^26 threads: 524 293 segments of
    row_len = 129 are 67 633 797 entries, so 524 933 threads take a second trip.  64-QAM: a row is one tile of 128 symbols, which
    goes through the wave's LDS stage, and a remainder of 1 -- every workgroup of csi_llr_kernel<6, true> refills its stage on its
    second trip.  seg_stride = 129 (1 032 bytes): every other segment is off the 16-byte grid.  Noise given, every output.
    Link 1: slices of 100 000 segments (12.9 M entries).  Link 2: the sample, segment by segment against csi_ref."""
    mod, n, rl = "64QAM", gc.N_SEG, gc.TAB_ROW_LEN
    assert n * rl > gc.CSI_GRID_CAP * gc.WG
    g = gen(torch, 7)
    a = 0.02 + 1.98 * torch.rand((n, rl), generator=g, device="cuda")
    sym = mmse_symbols(torch, g, a, draw_points(torch, g, (n, rl), mod), torch.tensor(0.01, device="cuda"))
    a[torch.rand((n, rl), generator=g, device="cuda") < 0.01] = 0                        # erasures: entries without an estimate
    big, small = csi_outs(torch, n, rl, mod, CSI_WANTS[0]), csi_outs(torch, n, rl, mod, CSI_WANTS[0])
    settle(torch)
    csi_call(om, torch, rx0, sym, a, 0, n, 1, rl, rl, rl, mod, True, big)
    for first, count in gc.parts(n, gc.SLICE_SEGS):
        csi_call(om, torch, rx0, sym, a, first, count, 1, rl, rl, rl, mod, True, small)
    settle(torch)
    link1(big, small)
    di = dev(torch, gc.sample(n, gc.CSI_GRID_CAP, seed=1))
    z, av = sym[di].cpu().numpy().view(np.complex64).reshape(-1, rl), a[di].cpu().numpy()
    llr, used, s2 = (small[k].body.view(n, -1)[di].cpu().numpy() for k in ("llr", "n_used", "sigma2"))
    assert (s2 == NV).all() and (used < rl).any() and used.min() > rl // 2
    for i in range(di.numel()):
        r_llr, _, r_n, _ = csi_ref.demap_csi_segment(z[i][None], av[i], RHO, mod, NV)
        assert same_bits(llr[i], r_llr) and used[i, 0] == r_n, int(di[i])


# ------------------------------------------------------------------------------------------ 2. receive-diversity combining
MRC_WANTS = (("llr", "sym", "weight"), ("llr",), ("sym",), ("weight",))


def mrc_input(torch, mod):
    key = ("mrc", mod)
    if key not in _CACHE:
        n, rl, B = gc.N_SEG, gc.ROW_LEN, gc.MRC_B
        idx, s_z, s_a, s_s2 = gc.mrc_sample(mod)
        g = gen(torch, 200 + BPS[mod])
        a = 0.02 + 1.98 * torch.rand((B, n, rl), generator=g, device="cuda")
        nv = dev(torch, np.array(gc.MRC_NOISE, np.float32)).view(B, 1, 1, 1)
        sym = mmse_symbols(torch, g, a, draw_points(torch, g, (n, rl), mod).unsqueeze(0).expand(B, n, rl, 2), nv)
        csi = torch.full((B, n, gc.CSI_STRIDE), float("nan"), dtype=torch.float32, device="cuda")
        csi[:, :, :rl] = a
        s2 = dev(torch, np.array(gc.MRC_NOISE)).view(B, 1) * (0.8 + 0.45 * torch.rand((B, n), generator=g, device="cuda", dtype=torch.float64))
        di = dev(torch, idx)
        s_csi = np.full((B, idx.size, gc.CSI_STRIDE), np.nan, np.float32)
        s_csi[:, :, :rl] = s_a
        for b in range(B):
            planted(torch, sym[b], di, s_z[b].view(np.float32))
            planted(torch, csi[b], di, s_csi[b])
            planted(torch, s2[b].view(n, 1), di, s_s2[b])
        _CACHE[key] = dict(sym=sym, csi=csi, s2=s2.contiguous(), di=di)
    return _CACHE[key]


def mrc_outs(torch, n_seg, seg_len, mod, want):
    size = dict(llr=n_seg * seg_len * BPS[mod], sym=n_seg * seg_len * 2, weight=n_seg * seg_len)
    return {k: Buf(torch, size[k], torch.float32) for k in want}


def mrc_call(torch, rx, sym, csi, noise, first, count, mod, out):
    """combine_csi_frames over segments first .. first + count - 1 of branch-major buffers sym [B][n][seg_len][2], csi [B][n][cs];
    noise: [B][n] float64 on the device (one variance per unit) or B numbers.  A slice of a branch-major batch is not a
    branch-major batch: it is copied into one."""
    B, n, seg_len = sym.shape[0], sym.shape[1], sym.shape[2]
    per_unit = hasattr(noise, "data_ptr")
    if count != n:
        sym, csi = sym[:, first:first + count].contiguous(), csi[:, first:first + count].contiguous()
        noise = noise[:, first:first + count].contiguous() if per_unit else noise
    settle(torch)
    rx.combine_csi_frames(sym, B, count, 1, seg_len, seg_len, csi, csi.shape[2], RHO, mod, noise_var=None if per_unit else noise,
                          d_sigma2=noise if per_unit else None, d_llr=out["llr"].at(first * seg_len * BPS[mod]) if "llr" in out else None,
                          d_sym_out=out["sym"].at(first * seg_len * 2) if "sym" in out else None,
                          d_weight=out["weight"].at(first * seg_len) if "weight" in out else None, stream=cur(torch))
    settle(torch)                                                                        # the slice's copies live until the launch has run


def mrc_reference(mod):
    key = ("mrc ref", mod)
    if key not in _CACHE:
        _, z, a, s2 = gc.mrc_sample(mod)
        llr, sym, weight = mrc_ref.combine_segments(z[:, :, None, :], a, RHO, mod, s2)
        _CACHE[key] = dict(llr=llr, sym=np.ascontiguousarray(sym).view(np.float32), weight=weight)
    return _CACHE[key]


@pytest.mark.parametrize("want", MRC_WANTS, ids=("all", "llr", "sym", "weight"))
@pytest.mark.parametrize("mod", MODS)
def test_combine_csi_frames_past_the_grid_cap(torch, rx0, mod, want):
    """The segment shape of the CSI test with B = 3 branches, one variance per unit: mrc_llr_kernel gets 524 293 items for a grid
    of MRC_GRID_CAP = 262 144 workgroups (2 trips each, workgroups 0 .. 4 take 3), and the branch loop runs two rounds of
    MRC_ROUND = 2 with the second one half empty.  llr alone is mrc_llr_kernel<MOD, false>, every other set <MOD, true>.
    Link 1: six launches of at most 100 000 segments, each on its own branch-major copy.  Link 2: the sample against mrc_ref,
    with a branch without a sync planted in the first segment of the second trip."""
    n, rl = gc.N_SEG, gc.ROW_LEN
    assert n * gc.seg_slices(rl) > gc.MRC_GRID_CAP
    inp = mrc_input(torch, mod)
    big, small = mrc_outs(torch, n, rl, mod, want), mrc_outs(torch, n, rl, mod, want)
    mrc_call(torch, rx0, inp["sym"], inp["csi"], inp["s2"], 0, n, mod, big)
    for first, count in gc.parts(n, gc.SLICE_SEGS):
        mrc_call(torch, rx0, inp["sym"], inp["csi"], inp["s2"], first, count, mod, small)
    link1(big, small)
    ref = mrc_reference(mod)
    for k in want:
        assert same_bits(small[k].body.view(n, -1)[inp["di"]].cpu().numpy(), ref[k]), k


def test_mrc_table_kernel_past_its_cap(torch, rx0):
    """mrc_table_kernel takes one thread per (unit, entry) on at most MRC_GRID_CAP * 256 = 2^26 threads: B = 2 branches of
    524 293 segments of row_len = 129 are 135 267 594 entries, so every thread takes 2 trips and 1 049 866 take 3.  64-QAM, every
    output: one tile of 128 symbols through the wave's LDS stage and a remainder of 1 per segment, refilled on the second trip of
    mrc_llr_kernel<6, true>; seg_stride = 129 puts every other segment off the 16-byte grid.  One variance per branch.
    Link 1: slices of 100 000 segments (25.8 M entries).  Link 2: the sample, segment by segment against mrc_ref."""
    mod, n, rl, B = "64QAM", gc.N_SEG, gc.TAB_ROW_LEN, gc.MRC_TAB_B
    assert B * n * rl > gc.MRC_GRID_CAP * gc.WG
    noise = [0.004, 0.01]
    g = gen(torch, 8)
    a = 0.02 + 1.98 * torch.rand((B, n, rl), generator=g, device="cuda")
    nv = dev(torch, np.array(noise, np.float32)).view(B, 1, 1, 1)
    sym = mmse_symbols(torch, g, a, draw_points(torch, g, (n, rl), mod).unsqueeze(0).expand(B, n, rl, 2), nv)
    a[torch.rand((B, n, rl), generator=g, device="cuda") < 0.01] = 0                     # entries without an estimate
    big, small = mrc_outs(torch, n, rl, mod, MRC_WANTS[0]), mrc_outs(torch, n, rl, mod, MRC_WANTS[0])
    mrc_call(torch, rx0, sym, a, noise, 0, n, mod, big)
    for first, count in gc.parts(n, gc.SLICE_SEGS):
        mrc_call(torch, rx0, sym, a, noise, first, count, mod, small)
    link1(big, small)
    di = dev(torch, gc.sample(n, gc.MRC_GRID_CAP, seed=2))
    z, av = sym[:, di].cpu().numpy().view(np.complex64).reshape(B, -1, rl), a[:, di].cpu().numpy()
    got = {k: small[k].body.view(n, -1)[di].cpu().numpy() for k in MRC_WANTS[0]}
    for i in range(di.numel()):
        r_llr, r_sym, r_w, _ = mrc_ref.combine(z[:, i, None, :], av[:, i], RHO, mod, noise)
        assert same_bits(got["llr"][i], r_llr) and same_bits(got["sym"][i], r_sym.view(np.float32)) and same_bits(got["weight"][i], r_w), int(di[i])
    assert (got["weight"] == 0).any() and (got["weight"] > 0).mean() > 0.99              # both branches erased somewhere


# ------------------------------------------------------------------------------------------ 3. the segmented soft de-mapper
SOFT_WANTS = (("sigma",), ("soft0", "soft1", "llr", "sigma"), ("llr",))


def soft_input(torch, mod):
    key = ("soft", mod)
    if key not in _CACHE:
        n, rl = gc.N_SEG, gc.ROW_LEN
        idx, s_z = gc.demap_sample(mod)
        g = gen(torch, 300 + BPS[mod])
        r = gc.DEMAP_R[0] + (gc.DEMAP_R[1] - gc.DEMAP_R[0]) * torch.rand((n, rl), generator=g, device="cuda")
        th = 2 * math.pi * torch.rand((n, rl), generator=g, device="cuda")
        sym = (draw_points(torch, g, (n, rl), mod) + torch.stack([r * torch.cos(th), r * torch.sin(th)], dim=-1)).contiguous()
        di = dev(torch, idx)
        planted(torch, sym, di, s_z.view(np.float32))
        _CACHE[key] = dict(sym=sym, di=di)
    return _CACHE[key]


def soft_outs(torch, n_seg, seg_len, mod, want):
    return {k: Buf(torch, n_seg if k == "sigma" else n_seg * seg_len * BPS[mod], torch.float64 if k == "sigma" else torch.float32) for k in want}


@pytest.mark.parametrize("want", SOFT_WANTS, ids=("sigma", "all", "llr"))
@pytest.mark.parametrize("mod", MODS)
def test_demap_frames_past_the_grid_caps(torch, rx0, mod, want):
    """524 293 segments of seg_len = 3 (one slice each) at seg_stride = 3: demap_seg_dmin_kernel gets 524 293 items for
    OFDM_DEMAP_CAP1 = 262 144 workgroups, demap_seg_soft_kernel<MOD, OUTS> 524 293 items for OFDM_DEMAP_CAP2 = 262 144 -- with
    OUTS = 0 (sigma only) one item per segment, which is the same count here: 2 trips per workgroup, 3 for workgroups 0 .. 4.
    Link 1: six launches of at most 100 000 segments.  Link 2: the sample against the oracle, segment by segment, as
    tests/test_gpu_soft_frames.py::check_segment does (grid_cap_cases.demap_sample says why these symbols keep 0.03 from their
    points)."""
    n, rl, bps = gc.N_SEG, gc.ROW_LEN, BPS[mod]
    assert n * gc.seg_slices(rl) > max(gc.OFDM_DEMAP_CAP1, gc.OFDM_DEMAP_CAP2)
    inp = soft_input(torch, mod)
    big, small = soft_outs(torch, n, rl, mod, want), soft_outs(torch, n, rl, mod, want)

    def call(first, count, out):
        p = {k: (b.at(first) if k == "sigma" else b.at(first * rl * bps)) for k, b in out.items()}
        rx0.demap_frames(inp["sym"].data_ptr() + 8 * gc.SEG_STRIDE * first, count, rl, gc.SEG_STRIDE, mod, d_soft0=p.get("soft0"),
                         d_soft1=p.get("soft1"), d_llr=p.get("llr"), d_sigma=p.get("sigma"), stream=cur(torch))

    settle(torch)
    call(0, n, big)
    for first, count in gc.parts(n, gc.SLICE_SEGS):
        call(first, count, small)
    settle(torch)
    link1(big, small)
    idx, s_z = gc.demap_sample(mod)
    got = {k: small[k].body.view(n, -1)[inp["di"]].cpu().numpy() for k in want}
    for i in range(idx.size):
        row = lambda k: got[k][i] if k in got else None                                   # noqa: E731
        sig = got["sigma"][i, 0] if "sigma" in got else None
        check_segment(s_z[i], mod, row("soft0"), row("soft1"), row("llr"), sig, "segment %d" % idx[i])
    if "sigma" in got:
        assert len(set(got["sigma"].ravel())) == idx.size, "segments with their own data get their own sigma"


# ------------------------------------------------------------------------------------------ 4. |H|^2 rows of a large batch
def test_csi_frames_past_its_cap(om, torch):
    """csi_frames_kernel takes one thread per output on at most 2^26 threads: 64-pt, Kd = 62, n_frames = 2^26 // 62 + 2 =
    1 082 403 frames of four symbols are 67 108 986 outputs, so threads 0 .. 121 take a second trip (the last one and a half
    frames).  The IQ buffer tiles seven distinct frames on the device (frame f is a copy of frame f % 7), so a frame's row is
    the row of the frame it copies in a batch of seven.  csi_stride = 63: one float of poison behind every row.
    Link 1: the large batch against the tiled rows of the seven-frame batch.  Link 2: those rows against csi_ref.csi_row on the
    handle's channel estimates, as tests/test_gpu_csi.py::test_csi_frames does."""
    c = gc.CSI_FRAMES
    N, cp, Ks, Kd, n_sym, n, K = c["N"], c["cp"], c["Ks"], c["Kd"], c["n_sym"], c["n_frames"], c["distinct"]
    assert n * Kd > gc.CSI_GRID_CAP * gc.WG
    L = N + cp
    fl, stride = n_sym * L, Kd + 1
    rng = np.random.default_rng(62)
    few = np.zeros((K, fl), np.complex64)
    for f in range(K):
        if f == 3:                                                                       # noise only
            few[f] = (0.3 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
            continue
        bits = rng.integers(0, 2, 3 * Kd * 2).astype(np.uint8)
        tx = orc.channel_apply(orc.tx_modulate(bits, N, cp, Ks, Kd, n_sym), orc.REF_TAPS, N)
        lead = int(rng.integers(0, cp))
        x = np.concatenate([0.05 * (rng.standard_normal(lead) + 1j * rng.standard_normal(lead)), tx])[:fl]
        x = np.concatenate([x, np.zeros(fl - len(x))])
        few[f] = (x + (0.01 + 0.005 * f) * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    rx = om.RxEngine(n_sym, N, cp, Ks, (1, 3), Kd, 30, 0.7)
    rx.set_max_trials(0)
    d_few = dev(torch, few.view(np.float32).reshape(K, fl, 2))
    reps = (n + K - 1) // K
    d_iq = d_few.repeat(reps, 1, 1)[:n]
    big, small = Buf(torch, n * stride, torch.float32), Buf(torch, K * stride, torch.float32)
    settle(torch)
    assert rx.demod_frames(d_iq, n, fl, fl, stream=cur(torch)) == 3
    rx.csi_frames(n, big.addr, stride, stream=cur(torch))
    assert rx.demod_frames(d_few, K, fl, fl, stream=cur(torch)) == 3
    rx.csi_frames(K, small.addr, stride, stream=cur(torch))
    torch.cuda.synchronize()
    assert small.bands_ok() and big.holds(small.body.view(K, stride).repeat(reps, 1)[:n])
    rows = small.body.view(K, stride).cpu().numpy()
    assert np.isnan(rows[:, Kd:]).all(), "wrote into the gap"
    bins = om.bins_p(Kd, N)
    for f in range(K):
        assert same_bits(rows[f, :Kd], csi_ref.csi_row(rx.frame_state(f)["chan_freq"], bins)), f
    live = [f for f in range(K) if rows[f, :Kd].any()]
    assert len(live) >= K - 1 and len(set(rows[f, :Kd].tobytes() for f in live)) == len(live), "distinct frames, distinct rows"


# ------------------------------------------------------------------------------------------ 5. the transmitter's element kernels
def test_tx_map_past_its_cap(om, torch):
    """tx_map_kernel takes one thread per symbol on at most 262144 * 256 = 2^26 threads: n_sym = 2^26 + 5, so threads 0 .. 4
    take a second trip.  64-QAM (six bit-bytes per symbol, the largest i * bps).
    Link 1: five launches of at most 2^24 symbols.  Link 2: windows of the output (head, tail, the one that straddles symbol
    2^26, 64 seeded random ones) against orc.map_bits as tests/test_gpu_tx_stages.py compares 16/64-QAM symbols."""
    n, bps = gc.TX_MAP_SYMS, 6
    assert n > gc.TX_GRID_CAP * gc.WG
    tx = om.TxEngine(64, 16, 62, 60, (1, 3), "64QAM")
    bits = torch.randint(0, 2, (n * bps,), generator=gen(torch, 11), device="cuda", dtype=torch.uint8)
    big, small = Buf(torch, 2 * n, torch.float32), Buf(torch, 2 * n, torch.float32)
    settle(torch)
    tx.map(bits, n, big.addr, om.BITS_UNPACKED, stream=cur(torch))
    for first, count in gc.parts(n, 1 << 24):
        tx.map(bits.data_ptr() + first * bps, count, small.at(2 * first), om.BITS_UNPACKED, stream=cur(torch))
    settle(torch)
    link1(dict(sym=big), dict(sym=small))
    for first, count in gc.windows(n, [gc.TX_GRID_CAP * gc.WG]):
        got = small.body[2 * first:2 * (first + count)].cpu().numpy().view(np.complex64)
        assert relerr(got, orc.map_bits(bits[first * bps:(first + count) * bps].cpu().numpy(), "64QAM")) < 2e-7, first


def test_tx_grid_past_its_cap(om, torch):
    """tx_grid_kernel takes one thread per grid bin on at most 2^26 threads: rows = 2^20 + 1 at N = 64 are 2^26 + 64 bins, so
    the last row is written on second trips.  Kd = 58 with four pilots: the data index skips the pilot entries.
    Link 1: five launches of at most 2^18 rows.  Link 2: the sampled rows (cap = 2^20 rows) equal orc.tx_stage_grid exactly, as
    in tests/test_gpu_tx_stages.py::test_pilots_and_flowgraph_parameters_vs_oracle."""
    c = gc.TX_GRID
    N, Kd, pil, rows = c["N"], c["Kd"], list(c["pilots"]), c["rows"]
    assert rows * N > gc.TX_GRID_CAP * gc.WG
    tx = om.TxEngine(N, 16, N - 2, Kd, (1, 3), "QPSK")
    tx.set_pilots(pil, 1 - 1j)
    sym = torch.randn((rows, Kd, 2), generator=gen(torch, 12), device="cuda")
    big, small = Buf(torch, rows * N * 2, torch.float32), Buf(torch, rows * N * 2, torch.float32)
    settle(torch)
    tx.grid(sym, rows, big.addr, stream=cur(torch))
    for first, count in gc.parts(rows, 1 << 18):
        tx.grid(sym.data_ptr() + 8 * Kd * first, count, small.at(2 * N * first), stream=cur(torch))
    settle(torch)
    link1(dict(grid=big), dict(grid=small))
    di = dev(torch, gc.sample(rows, gc.TX_GRID_CAP * gc.WG // N, seed=3))
    got = small.body.view(rows, 2 * N)[di].cpu().numpy().view(np.complex64)
    want = orc.tx_stage_grid(sym[di].cpu().numpy().view(np.complex64).ravel(), N, Kd, pil, 1 - 1j)
    assert np.array_equal(got, np.asarray(want).reshape(-1, N).astype(np.complex64))


def test_tx_random_bits_past_its_cap(om, torch):
    """tx_random_bits_kernel takes one thread per 128-bit Philox block on at most 2^26 threads: n = 2^33 + 640 bits from offset
    77 are 2^26 + 6 blocks, so threads 0 .. 5 take a second trip, and the bits from output index 2^33 - 77 on come from second
    trips.  The contract says any window can be produced independently: windows of the large launch (head, tail, the one that
    straddles the second trip, 64 seeded random ones) equal a small launch at the matching offset (link 1) and orc.random_bits
    (link 2), both exactly."""
    r = gc.TX_RANDOM
    seed, offset, n = r["seed"], r["offset"], r["n"]
    edge = gc.TX_GRID_CAP * gc.WG * gc.RANDOM_BLOCK - offset
    assert (offset + n + 127) // 128 > gc.TX_GRID_CAP * gc.WG and 0 < edge < n
    tx = om.TxEngine(64, 16, 62, 60)
    big = Buf(torch, n, torch.uint8)
    settle(torch)
    tx.random_bits(seed, offset, big.addr, n, stream=cur(torch))
    torch.cuda.synchronize()
    assert big.bands_ok() and int(big.body.max()) == 1, "a byte that is no bit: left unwritten"
    for first, count in gc.windows(n, [edge]):
        one = Buf(torch, count, torch.uint8)
        settle(torch)
        tx.random_bits(seed, offset + first, one.addr, count, stream=cur(torch))
        torch.cuda.synchronize()
        assert one.bands_ok() and torch.equal(big.body[first:first + count], one.body), first
        assert np.array_equal(one.body.cpu().numpy(), orc.random_bits(seed, offset + first, count)), first


# ------------------------------------------------------------------------------------------ 6. gridDim.y = 65 535
def distinct_cinits(torch, n, seed):
    """31-bit c_init values, all different: an odd multiplier is a bijection modulo 2^31"""
    v = (torch.arange(n, device="cuda", dtype=torch.int64) * 1103515245 + seed) % (1 << 31)
    return v.to(torch.int32)


@pytest.mark.parametrize("mode", ("bytes", "packed", "llr"))
def test_gold_sequence_past_65535_segments(om, torch, rx0, mode):
    """gold_apply_kernel puts the segments on gridDim.y, capped at 65 535: n_seg = 65 535 + 37 segments of 40 bits, so grid rows
    0 .. 36 take a second trip and overwrite their LDS sequence words.  A c_init of its own per segment.  bytes / packed:
    ofdm_tx_scramble_frames; llr: ofdm_descramble_llr_frames at a stride of 43 floats (172 bytes: a grid row meets another
    16-byte alignment on its second trip, and the three floats behind every segment must stay poison).
    Link 1: three launches of at most 30 000 segments.  Link 2: the sample against lte_bits_ref, exactly."""
    c = gc.GOLD
    n, seg_bits = c["n_seg"], c["seg_bits"]
    assert n > gc.GRID_Y_CAP
    g = gen(torch, 13)
    cinit = distinct_cinits(torch, n, 12345)
    tx = om.TxEngine(64, 16, 62, 60)
    if mode == "llr":
        stride = c["llr_stride"]
        src = torch.randn((n, stride), generator=g, device="cuda")
        big, small = Buf(torch, n * stride, torch.float32), Buf(torch, n * stride, torch.float32)
        settle(torch)
        rx0.descramble_llr_frames(src, n, stride, seg_bits, cinit, big.addr, stride, stream=cur(torch))
        for first, count in gc.parts(n, gc.SLICE_ROWS):
            rx0.descramble_llr_frames(src.data_ptr() + 4 * stride * first, count, stride, seg_bits, cinit.data_ptr() + 4 * first,
                                      small.at(stride * first), stride, stream=cur(torch))
    else:
        row = seg_bits // 8 if mode == "packed" else seg_bits
        m = om.BITS_PACKED if mode == "packed" else om.BITS_UNPACKED
        src = torch.randint(0, 256 if mode == "packed" else 2, (n, row), generator=g, device="cuda", dtype=torch.uint8)
        big, small = Buf(torch, n * row, torch.uint8), Buf(torch, n * row, torch.uint8)
        settle(torch)
        tx.scramble_frames(src, n, seg_bits, cinit, big.addr, mode=m, stream=cur(torch))
        for first, count in gc.parts(n, gc.SLICE_ROWS):
            tx.scramble_frames(src.data_ptr() + row * first, count, seg_bits, cinit.data_ptr() + 4 * first, small.at(row * first), mode=m,
                               stream=cur(torch))
    settle(torch)
    link1(dict(out=big), dict(out=small), packed=("out",))
    idx = gc.sample(n, gc.GRID_Y_CAP, seed=4)
    di = dev(torch, idx)
    ci = cinit[di].cpu().numpy().astype(np.int64)
    if mode == "llr":
        body = small.body.view(n, stride)
        assert bool(torch.isnan(body[:, seg_bits:]).all()) and not bool(torch.isnan(body[:, :seg_bits]).any())
        want = lb.descramble_llr(src[di][:, :seg_bits].cpu().numpy(), ci)
        assert same_bits(body[di][:, :seg_bits].cpu().numpy(), want)
    else:
        got, plain = small.body.view(n, -1)[di].cpu().numpy(), src[di].cpu().numpy()
        if mode == "packed":
            got, plain = np.unpackbits(got, axis=1), np.unpackbits(plain, axis=1)
        else:
            assert int(small.body.max()) == 1
        assert np.array_equal(got, lb.scramble(plain, ci))
    assert len(set(ci.tolist())) == idx.size


def test_tb_concat_past_65535_transport_blocks(om, torch):
    """tb_concat_kernel puts the transport blocks on gridDim.y, capped at 65 535: n_tb = 65 535 + 37 at A = 40, so grid rows
    0 .. 36 take a second trip.  Z = 40 cuts a transport block into four code blocks of K = 40, and G = 530 gives them E = 132,
    132, 133, 133: two groups, so the gather crosses a group boundary; cw_bits = 535 leaves five zero bits behind G.
    Link 1: three launches of at most 30 000 transport blocks.  Link 2: the sample against tb_ref.encode, exactly."""
    c = gc.TB
    n, A, Z, G, cw_bits = c["n_tb"], c["A"], c["Z"], c["G"], c["cw_bits"]
    assert n > gc.GRID_Y_CAP
    qm, qp = tc.pairs(A, Z)
    assert om.turbo_qpp_check(tb_ref.segmentation(A, Z)["K_plus"], *qp)
    tx = om.TxEngine(64, 16, 62, 60)
    pay = torch.randint(0, 2, (n, A), generator=gen(torch, 14), device="cuda", dtype=torch.uint8)
    big, small = Buf(torch, n * cw_bits, torch.uint8), Buf(torch, n * cw_bits, torch.uint8)
    settle(torch)
    tx.tb_encode_frames(pay, n, A, G, qp, big.addr, cw_bits, qpp_minus=qm, Z=Z, stream=cur(torch))
    for first, count in gc.parts(n, gc.SLICE_ROWS):
        tx.tb_encode_frames(pay.data_ptr() + A * first, count, A, G, qp, small.at(cw_bits * first), cw_bits, qpp_minus=qm, Z=Z,
                            stream=cur(torch))
    settle(torch)
    link1(dict(cw=big), dict(cw=small))
    di = dev(torch, gc.sample(n, gc.GRID_Y_CAP, seed=5))
    want = tb_ref.encode(pay[di].cpu().numpy(), G, qm, qp, Z=Z, cw_bits=cw_bits)
    assert np.array_equal(small.body.view(n, cw_bits)[di].cpu().numpy(), want)
    assert not want[:, G:].any() and len(set(map(bytes, want))) > di.numel() - 3


# ------------------------------------------------------------------------------------------ 7. the CFO-search receiver's parts
def tiled(torch, few, n):
    """[K][...] host array -> [n][...] on the device, row f a copy of row f % K"""
    t = dev(torch, few)
    return t.repeat(((n + t.shape[0] - 1) // t.shape[0],) + (1,) * (t.dim() - 1))[:n].contiguous()


def test_fo_despread_past_65535_rows(om, torch):
    """ofdm_fo_demod_frames despreads the (frame, row) units in parts of 65 535 rows: 700 frames are 70 000 rows, so a second
    launch takes rows 65 535 .. 69 999 at the offsets r0 * Kd (input) and r0 * n_spread (output) -- frame 655 from row 35 on and
    frames 656 .. 699, whose first rows are live syncs.  DSSS case 4 (128-pt, Kd = 32, DSSS = 8) as
    tests/test_gpu_fo_batch.py::test_batch_despread_equals_fresh_stream_calls; the IQ buffer tiles seven distinct frames on the
    device.  Only status and the despread rows are asked for, so the equalised rows go to the handle's own buffer.
    Link 1: the large batch against the tiled outputs of the seven-frame batch.  Link 2: that batch against a fresh stream call
    per frame."""
    import test_gpu_fo_batch as fb
    c = gc.FO_DESPREAD
    case, fo_range, n, K = c["case"], list(c["fo_range"]), c["n_frames"], c["distinct"]
    assert n * gc.FO_MAX_SYNC > gc.FO_PART
    n_symb, fs, N = orc.DSSS_CASES[case][:3]
    L = N + N // 4
    blk = fb._dsss_block(case, fo_range, py2_rotators=False)
    eng = blk._engine
    rng = np.random.default_rng(8)
    fl = n_symb * L + L
    few = np.stack([fb._fit(fb._tx(blk, n_symb, rng, -fo_range[f % 3], fs)[0], int(rng.integers(0, L)), fl) for f in range(K)])
    ref = fb._run_engine(om, eng, few, om.BITS_PACKED, want_despread=True)
    for f in range(K):
        st = fb._fresh(lambda: fb._dsss_block(case, fo_range, py2_rotators=False), few[f])
        assert ref["status"][f] == st["status"] >= 1
        assert np.array_equal(ref["tsr"][f], st["time_synch_ref"].astype(np.int32))
        assert fb._same(ref["data_freq"][f], st["data_freq"]) and fb._same(ref["data_freq_d"][f], st["data_freq_d"])
    ns = eng.n_spread
    d_iq = tiled(torch, few.view(np.float32).reshape(K, fl, 2), n)
    status, edfd = Buf(torch, n, torch.int32), Buf(torch, n * gc.FO_MAX_SYNC * ns * 2, torch.float32)
    settle(torch)
    assert eng.demod_frames(d_iq, n, fl, fl, status.addr, d_data_freq_d=edfd.addr, stream=cur(torch)) == gc.FO_MAX_SYNC
    torch.cuda.synchronize()
    assert status.holds(tiled(torch, ref["status"].astype(np.int32), n))
    assert edfd.holds(tiled(torch, ref["data_freq_d"].view(np.float32).reshape(K, -1), n))
    second = ref["data_freq_d"][[f % K for f in range(656, n)]]
    assert second[:, 0].any(), "the second part holds live rows"


def test_fo_trial_table_past_65535_frames(om, torch):
    """ofdm_fo_demod_frames builds the trial table in parts of 65 535 frames (one grid row per frame): n_frames = 65 535 + 3, so a
    second launch writes the tables of frames 65 535 .. 65 537 at h->b_tm + f0 * n_fo * pv.  FO case 0 (64-pt, Kd = 12), three
    candidates, frames of nine symbol lengths; only status, time_synch_ref and the candidate index are asked for (what the
    decision stage writes from the table).  The IQ buffer tiles four distinct frames with 1 .. 4 syncs: frames 0 .. 2 and frames
    65 535 .. 65 537 are copies of different ones, so a second part written over the first, or read from there, shows.
    Workspace: 65 538 frames * 100 rows * (12 gains * 8 + 16) bytes = 0.73 GB, the tables a few tens of MB.
    Link 1: the large batch against the tiled outputs of the four-frame batch.  Link 2: that batch against a fresh stream call
    per frame."""
    import test_gpu_fo_batch as fb
    c = gc.FO_LARGE
    case, fo_range, n, K = c["case"], list(c["fo_range"]), c["n_frames"], c["distinct"]
    assert n > gc.FO_PART
    _, fs, N = orc.FO_CASES[case][:3]
    L = N + N // 4
    blk = fb._fo_block(case, fo_range, py2_rotators=False)
    eng = blk._engine
    rng = np.random.default_rng(15)
    fl = c["n_sym"] * L + L
    few = np.stack([fb._fit(fb._tx(blk, 2 * (k + 1), rng, -fo_range[k % 3], fs)[0], 7 * k + 3, fl) for k in range(K)])
    ref = fb._run_engine(om, eng, few, om.BITS_UNPACKED)
    for f in range(K):
        st = fb._fresh(lambda: fb._fo_block(case, fo_range, py2_rotators=False), few[f])
        assert ref["status"][f] == st["status"] >= 1
        assert np.array_equal(ref["tsr"][f], st["time_synch_ref"].astype(np.int32)) and ref["fo_idx"][f] == st["fo_idx"]
        for key in ("data_freq", "chan_freq", "chan_time", "synch_freq"):
            assert fb._same(ref[key][f], st[key]), (f, key)
    assert len(set(ref["status"].tolist())) == K, "frames 0 .. 2 and 65535 .. 65537 must differ in what the table decides"
    d_iq = tiled(torch, few.view(np.float32).reshape(K, fl, 2), n)
    status, tsr, fo = Buf(torch, n, torch.int32), Buf(torch, n * gc.FO_MAX_SYNC * 3, torch.int32), Buf(torch, n, torch.int32)
    settle(torch)
    assert eng.demod_frames(d_iq, n, fl, fl, status.addr, d_tsr=tsr.addr, d_fo_idx=fo.addr, stream=cur(torch)) == gc.FO_MAX_SYNC
    torch.cuda.synchronize()
    assert status.holds(tiled(torch, ref["status"].astype(np.int32), n))
    assert tsr.holds(tiled(torch, ref["tsr"].astype(np.int32).reshape(K, -1), n))
    assert fo.holds(tiled(torch, ref["fo_idx"].astype(np.int32), n))
