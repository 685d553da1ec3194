"""Multi-user allocations of DFT-spread OFDM on the GPU (-m gpu): ofdm_dft_despread_alloc_frames, ofdm_tx_dft_spread_alloc and the
two composite calls.  The contract (include/ofdm_mi355x.h) is one sentence: block u holds, bit for bit, what
ofdm_dft_despread_frames writes for M_u and mod_u on a dense copy of the allocation's columns -- so the existing call on a
gather made with torch is the reference for every output, and tests/dft_alloc_ref.py (fp64) for the transforms at the suite's
1e-5 bar.  Every output sits between poisoned guard bands.

Sets: the smallest that reach every path.  S1 one M at two modulations; S2 odd starts, odd sizes, M = 1, gaps at both ends and
inside, with an even and an odd row length (the row alignment then alternates); S3 the LTE 20 MHz row; S4 both size classes in
one call and the padded power-of-two LDS layout; S5 the cap of 32 allocations; S6 dense.  rows is 1 and the largest
rows_per_group of the set plus 1; n_seg 1 and 3; the input base on a 16-byte and on an 8-byte address; the three noise modes and
d_csi = NULL.  These are combined in four runs per set, not crossed: each run's reference is one existing call per allocation."""
import math

import numpy as np
import pytest

import dft_alloc_ref as aref
import dft_spread_ref as ref
from conftest import TOL_MAX, relerr
from oracle import ofdm_oracle as orc
from test_gpu_csi import Out, cur, demod
from test_gpu_dft_spread import RHO, WANT_ALL, bits_of, put
from test_gpu_dft_spread import run as run_single
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

NAME = {2: "QPSK", 4: "16QAM", 6: "64QAM"}
S1 = [(0, 12, 2), (12, 24, 4), (36, 24, 6)]
S2 = [(1, 25, 4), (27, 1, 2), (31, 45, 6)]
S3 = [(0, 300, 2), (300, 600, 6), (900, 288, 4), (1188, 12, 2)]
S4 = [(0, 2400, 4), (2400, 1200, 2), (3600, 64, 6), (3664, 36, 4)]
S5 = [(12 * k, 12, 2 + 2 * (k % 3)) for k in range(32)]
S6 = [(0, 60, 4)]
SETS = {"S1": (60, S1), "S2-80": (80, S2), "S2-81": (81, S2), "S3": (1200, S3), "S4": (3700, S4), "S5": (384, S5), "S6": (60, S6)}
K600 = [(0, 300, 6), (300, 288, 2), (588, 12, 4)]           # the 1024-pt fixture: Kd = 600, three users at three modulations


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


@pytest.fixture(scope="module")
def rxg(om):
    """the handle of the gathered single-M reference calls: its plan cache is churned, the set of rx0 is not in it"""
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


@pytest.fixture(scope="module")
def tx0(om):
    return om.TxEngine(64, 16, 62, 60, (1, 3), "QPSK")


def max_rpg(om, allocs):
    return max(om.dft_plan_info(a[1])[2] for a in allocs)


def make_rows(rng, n_seg, rows, row_len, allocs, extra=0):
    """-> sym [n_seg][rows*row_len + extra] complex64, csi [n_seg][row_len + 3] float32, sigma2 [n_seg]: every allocation a user
    of its own (spread constellation rows through a one-tap MMSE equaliser over its own channel); gaps and strides hold noise"""
    n = rows * row_len
    sym = (rng.standard_normal((n_seg, n + extra)) + 1j * rng.standard_normal((n_seg, n + extra))).astype(np.complex64)
    csi = rng.uniform(0.1, 1.0, (n_seg, row_len + 3)).astype(np.float32)
    sig = np.array([(0.002, 0.005, 0.01)[s % 3] for s in range(n_seg)])
    for s in range(n_seg):
        z = sym[s, :n].reshape(rows, row_len)
        for start, M, bps in allocs:
            a = rng.uniform(0.02, 2.0, M)
            x = ref.spread(orc.map_bits(rng.integers(0, 2, rows * M * bps), NAME[bps]).reshape(rows, M))
            w = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))) * math.sqrt(sig[s] / 2)
            z[:, start:start + M] = (a / (a + RHO)) * (x + w / np.sqrt(a))
            csi[s, start:start + M] = a
    return sym, csi, sig


def noise_args(om, torch, noise):
    mode = dict(rho=om.DESPREAD_NOISE_RHO, given=om.DESPREAD_NOISE_GIVEN, seg=om.DESPREAD_NOISE_SEG)[noise[0]]
    d_sig = torch.from_numpy(np.asarray(noise[1], np.float64)).cuda() if noise[0] == "seg" else None
    return mode, (noise[1] if noise[0] == "given" else 0.0), d_sig


def run_alloc(om, torch, rx, sym, csi, rows, row_len, allocs, noise=("rho", None), want=WANT_ALL, base_off=0, bits_mode=None, rho=RHO):
    """dft_despread_alloc_frames on host arrays -> dict of host arrays in the allocation-major layout"""
    n_seg = sym.shape[0]
    bits_mode = om.BITS_UNPACKED if bits_mode is None else bits_mode
    t, addr = put(torch, sym, base_off)
    d_csi = None if csi is None else torch.from_numpy(np.ascontiguousarray(csi)).cuda()
    lay = om.alloc_layout([a[1] for a in allocs], [a[2] for a in allocs], n_seg, rows, bits_mode)
    size = dict(sym=(2 * lay["sym"], torch.float32), llr=(lay["llr"], torch.float32), bits=(lay["bits"], torch.uint8),
                beta=(len(allocs) * n_seg, torch.float32), weight=(len(allocs) * n_seg, torch.float32))
    o = {k: (Out(torch, *size[k]) if k in want else None) for k in WANT_ALL}
    mode, nv, d_sig = noise_args(om, torch, noise)
    rx.dft_despread_alloc_frames(addr, n_seg, rows, row_len, sym.shape[1], d_csi, 0 if csi is None else csi.shape[1], rho,
                                 d_sym_out=o["sym"] and o["sym"].addr, d_llr=o["llr"] and o["llr"].addr,
                                 d_bits=o["bits"] and o["bits"].addr, bits_mode=bits_mode if "bits" in want else om.BITS_NONE,
                                 d_beta=o["beta"] and o["beta"].addr, d_weight=o["weight"] and o["weight"].addr, noise_mode=mode,
                                 noise_var=nv, d_sigma2=d_sig, stream=cur(torch))
    torch.cuda.synchronize()
    return {k: (v.read().copy() if v else None) for k, v in o.items()}


def blocks(om, got, allocs, n_seg, rows, bits_mode=None):
    """the outputs of run_alloc cut into the allocations' blocks: a list of dicts"""
    bits_mode = om.BITS_UNPACKED if bits_mode is None else bits_mode
    lay = om.alloc_layout([a[1] for a in allocs], [a[2] for a in allocs], n_seg, rows, bits_mode)
    out = []
    for u, (_, M, bps) in enumerate(allocs):
        n = n_seg * rows * M
        nb = n * bps // 8 if bits_mode == om.BITS_PACKED else n * bps
        cut = dict(sym=(2 * int(lay["sym_off"][u]), 2 * n), llr=(int(lay["llr_off"][u]), n * bps), bits=(int(lay["bits_off"][u]), nb),
                   beta=(u * n_seg, n_seg), weight=(u * n_seg, n_seg))
        out.append({k: (None if got[k] is None else got[k][cut[k][0]:cut[k][0] + cut[k][1]]) for k in WANT_ALL})
    return out


def gathered(torch, sym, csi, rows, row_len, start, M):
    """columns start .. start+M-1 of every row and of csi, dense, gathered with torch on the device"""
    n_seg = sym.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(sym[:, :rows * row_len]).view(np.float32)).cuda().view(n_seg, rows, row_len, 2)
    g = t[:, :, start:start + M, :].contiguous().cpu().numpy().view(np.complex64).reshape(n_seg, rows * M)
    c = None if csi is None else torch.from_numpy(csi).cuda()[:, start:start + M].contiguous().cpu().numpy()
    return g, c


def reference(om, torch, rxg, sym, csi, rows, row_len, allocs, noise, bits_mode=None):
    """the existing call on the gathered copy of every allocation: a list of dicts"""
    out = []
    for start, M, bps in allocs:
        g, c = gathered(torch, sym, csi, rows, row_len, start, M)
        out.append(run_single(om, torch, rxg, g, c, rows, M, NAME[bps], noise, bits_mode=bits_mode))
    return out


def assert_blocks_equal(got_blocks, want_blocks, tag=""):
    for u, (g, w) in enumerate(zip(got_blocks, want_blocks)):
        for k in WANT_ALL:
            if g[k] is not None:
                assert np.array_equal(g[k].view(np.uint8), w[k].view(np.uint8)), (tag, u, k)


# ------------------------------------------------------------------------------------------ 1, 2. block equality, fp64
@pytest.mark.parametrize("name", list(SETS))
def test_every_block_is_the_existing_call_on_the_gathered_columns(om, torch, rx0, rxg, name):
    row_len, allocs = SETS[name]
    assert aref.check_set(allocs, row_len) is None
    rx0.set_allocations(allocs)
    R = max_rpg(om, allocs) + 1
    rng = np.random.default_rng(len(name) + row_len)
    packable = all(M * bps % 8 == 0 for _, M, bps in allocs)
    for rows, n_seg, base_off, kind in ((1, 1, 0, "rho"), (R, 3, 8, "seg"), (R, 1, 8, "given"), (1, 3, 0, "none")):
        sym, csi, sig = make_rows(rng, n_seg, rows, row_len, allocs, extra=1 if base_off else 0)
        noise = dict(rho=("rho", None), seg=("seg", sig), given=("given", 0.004), none=("given", 1.0))[kind]
        if kind == "none":
            csi = None
        got = run_alloc(om, torch, rx0, sym, csi, rows, row_len, allocs, noise, base_off=base_off)
        want = reference(om, torch, rxg, sym, csi, rows, row_len, allocs, noise)
        mine = blocks(om, got, allocs, n_seg, rows)
        assert_blocks_equal(mine, want, (name, rows, n_seg, kind))
        for k in ("sym", "llr", "beta", "weight"):
            assert np.isfinite(got[k]).all(), k
        for u, (start, M, bps) in enumerate(allocs):         # the transforms against fp64
            for s in range(n_seg):
                z = sym[s, :rows * row_len].reshape(rows, row_len)
                wt = aref.despread_alloc_segment(z, None if csi is None else csi[s, :row_len], [allocs[u]], RHO,
                                                 float(np.float32(RHO)) if kind == "rho" else noise[1] if kind != "seg" else sig[s])
                dev = mine[u]["sym"].view(np.complex64).reshape(n_seg, rows * M)[s]
                assert relerr(dev, wt[0][0].ravel()) < TOL_MAX, (name, u, s, relerr(dev, wt[0][0].ravel()))
                if kind == "none":
                    assert mine[u]["beta"][s] == 1 and mine[u]["weight"][s] == 1
                else:
                    assert mine[u]["beta"][s] > 0 and mine[u]["weight"][s] > 0
        if kind == "seg":                                    # packed bits where every allocation fills bytes, refused elsewhere
            if packable:
                gp = run_alloc(om, torch, rx0, sym, csi, rows, row_len, allocs, noise, want=("bits",), base_off=base_off,
                               bits_mode=om.BITS_PACKED)
                for u, (b, w) in enumerate(zip(blocks(om, gp, allocs, n_seg, rows, om.BITS_PACKED), want)):
                    assert np.array_equal(b["bits"], np.packbits(w["bits"])), (name, u)
            else:
                o = Out(torch, 64, torch.uint8)
                d = torch.zeros(2 * n_seg * (rows * row_len + 1) + 8, dtype=torch.float32, device="cuda")
                with pytest.raises(ValueError, match="packed bits need"):
                    rx0.dft_despread_alloc_frames(d, n_seg, rows, row_len, rows * row_len, None, 0, RHO, d_bits=o.addr,
                                                  bits_mode=om.BITS_PACKED, stream=cur(torch))
                assert o.untouched()


def test_dense_set_equals_the_existing_call_on_the_same_buffer(om, torch, rx0, rxg):
    rows, n_seg = 17, 3
    sym, csi, sig = make_rows(np.random.default_rng(6), n_seg, rows, 60, S6)
    rx0.set_allocations(S6)
    got = run_alloc(om, torch, rx0, sym, csi, rows, 60, S6, ("seg", sig))
    want = run_single(om, torch, rxg, sym, csi, rows, 60, "16QAM", ("seg", sig))
    for k in WANT_ALL:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k


# ------------------------------------------------------------------------------------------ 3. independence
@pytest.mark.parametrize("name", ["S1", "S2-81"])
def test_independence(om, torch, rx0, name):
    row_len, allocs = SETS[name]
    rows, n_seg = max_rpg(om, allocs) + 1, 2
    rng = np.random.default_rng(31)
    sym, csi, sig = make_rows(rng, n_seg, rows, row_len, allocs, extra=1)
    noise = ("seg", sig)
    rx0.set_allocations(allocs)
    full = run_alloc(om, torch, rx0, sym, csi, rows, row_len, allocs, noise, base_off=8)
    for k in WANT_ALL:                                       # each output alone; a repeated call
        one = run_alloc(om, torch, rx0, sym, csi, rows, row_len, allocs, noise, want=(k,), base_off=8)
        assert np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), k
    again = run_alloc(om, torch, rx0, sym, csi, rows, row_len, allocs, noise, base_off=0)
    assert all(np.array_equal(again[k].view(np.uint8), full[k].view(np.uint8)) for k in WANT_ALL)
    base = blocks(om, full, allocs, n_seg, rows)
    # the gaps and the strides poisoned: never read for data
    covered = np.zeros(row_len, bool)
    for s, M, _ in allocs:
        covered[s:s + M] = True
    z2, c2 = sym.copy(), csi.copy()
    for s in range(n_seg):
        z2[s, :rows * row_len].reshape(rows, row_len)[:, ~covered] = complex(np.nan, np.nan)
    z2[:, rows * row_len:] = complex(np.nan, np.nan)
    c2[:, :row_len][:, ~covered] = np.nan
    c2[:, row_len:] = np.nan
    poisoned = run_alloc(om, torch, rx0, z2, c2, rows, row_len, allocs, noise, base_off=8)
    assert all(np.array_equal(poisoned[k].view(np.uint8), full[k].view(np.uint8)) for k in WANT_ALL)
    # the list in another order: the same blocks, permuted
    perm = allocs[1:] + allocs[:1]
    rx0.set_allocations(perm)
    turned = blocks(om, run_alloc(om, torch, rx0, sym, csi, rows, row_len, perm, noise, base_off=8), perm, n_seg, rows)
    assert_blocks_equal(turned, base[1:] + base[:1], "permuted")
    rx0.set_allocations(allocs)
    # user v's data and channel changed: user u's block keeps its bits, user v's does not
    for v, (s, M, _) in enumerate(allocs):
        z3, c3 = sym.copy(), csi.copy()
        for k in range(n_seg):
            z3[k, :rows * row_len].reshape(rows, row_len)[:, s:s + M] *= np.complex64(0.5 + 0.25j)
        c3[:, s:s + M] *= np.float32(0.7)
        other = blocks(om, run_alloc(om, torch, rx0, z3, c3, rows, row_len, allocs, noise, base_off=8), allocs, n_seg, rows)
        for u in range(len(allocs)):
            same = all(np.array_equal(other[u][k].view(np.uint8), base[u][k].view(np.uint8)) for k in WANT_ALL)
            assert same == (u != v), (u, v)


# ------------------------------------------------------------------------------------------ 4. planted entries
def test_planted_entries_per_allocation(om, torch, rx0, rxg):
    row_len, allocs = SETS["S1"]
    rows, n_seg = 5, 3
    sym, csi, sig = make_rows(np.random.default_rng(41), n_seg, rows, row_len, allocs)
    z = sym.reshape(n_seg, rows, row_len)
    z[0, 1, 3] = complex(np.nan, 0.1)                        # user 0: non-finite symbols
    z[0, 4, 11] = complex(0.1, -np.inf)
    for j, a in zip((13, 20, 35), (0.0, -1.0, np.nan)):      # user 1: unusable entries
        csi[0, j] = a
    z[0, 2, 36:60] = 0                                       # user 2: a zero row (its neighbours' entries of the row are not)
    csi[1, 12:36] = 0                                        # segment 1, user 1: every entry unusable
    csi[1, 36:60] = 1e-44                                    # segment 1, user 2: beta underflows, float(1/beta) is not finite
    sig[2] = 1e300                                           # segment 2: the weights underflow, the symbols stay
    noise = ("seg", sig)
    rx0.set_allocations(allocs)
    got = run_alloc(om, torch, rx0, sym, csi, rows, row_len, allocs, noise)
    mine = blocks(om, got, allocs, n_seg, rows)
    assert_blocks_equal(mine, reference(om, torch, rxg, sym, csi, rows, row_len, allocs, noise), "planted")
    for k in ("sym", "llr", "beta", "weight"):
        assert np.isfinite(got[k]).all(), k                  # no non-finite value leaves the call
    s2 = mine[2]["sym"].view(np.complex64).reshape(n_seg, rows, 24)
    assert not bits_of(s2[0, 2]).any() and s2[0, 1].all()    # the zero row is an erasure, +0
    assert mine[1]["beta"][1] == 0 and mine[1]["weight"][1] == 0 and mine[2]["beta"][1] == 0 and mine[2]["weight"][1] == 0
    assert mine[0]["beta"][1] > 0 and mine[0]["sym"].view(np.complex64).reshape(n_seg, rows, 12)[1].all()
    assert all(m["weight"][2] == 0 and m["beta"][2] > 0 for m in mine)


# ------------------------------------------------------------------------------------------ 5. the transmit precoder
@pytest.mark.parametrize("name", ["S2-81", "S2-80", "S4", "S5"])
def test_transmit_precoder(om, torch, tx0, name):
    row_len, allocs = SETS[name]
    tx_list = [(s, M) for s, M, _ in allocs]
    tx0.set_allocations(tx_list)
    rng = np.random.default_rng(51)
    covered = np.zeros(row_len, bool)
    for s, M in tx_list:
        covered[s:s + M] = True
    for n_rows in (1, max_rpg(om, allocs) + 1):
        x = (rng.standard_normal((n_rows, row_len)) + 1j * rng.standard_normal((n_rows, row_len))).astype(np.complex64)
        first = None
        for base_off in (0, 8):
            for in_place in (False, True):
                t, addr = put(torch, x, base_off)
                o = Out(torch, 2 * x.size, torch.float32)
                tx0.dft_spread_alloc(addr, n_rows, row_len, addr if in_place else o.addr, stream=cur(torch))
                torch.cuda.synchronize()
                if in_place:
                    assert o.untouched()
                    got = t.cpu().numpy()[base_off // 4:base_off // 4 + 2 * x.size].view(np.complex64).reshape(n_rows, row_len)
                else:
                    got = o.read().view(np.complex64).reshape(n_rows, row_len)
                first = got.copy() if first is None else first
                assert np.array_equal(bits_of(got), bits_of(first)), (n_rows, base_off, in_place)
        assert not bits_of(first[:, ~covered]).any()         # +0+0j where nothing is sent
        assert relerr(first, aref.spread_alloc(x, tx_list)) < TOL_MAX
        for s, M in tx_list:                                 # bit for bit the single transform on the gathered columns
            g = np.ascontiguousarray(x[:, s:s + M])
            t, addr = put(torch, g)
            o = Out(torch, 2 * g.size, torch.float32)
            tx0.dft_spread(addr, n_rows, M, o.addr, stream=cur(torch))
            assert np.array_equal(bits_of(o.read()), bits_of(np.ascontiguousarray(first[:, s:s + M])).ravel()), (s, M)
    d = torch.zeros(2 * row_len, dtype=torch.float32, device="cuda")
    o = Out(torch, 2 * row_len, torch.float32)
    with pytest.raises(ValueError, match="row_len <"):
        tx0.dft_spread_alloc(d, 1, max(s + M for s, M in tx_list) - 1, o.addr, stream=cur(torch))
    tx0.set_allocations([])
    with pytest.raises(ValueError, match="no allocation set"):
        tx0.dft_spread_alloc(d, 1, row_len, o.addr, stream=cur(torch))
    assert o.untouched()


# ------------------------------------------------------------------------------------------ 6. the composite receiver
@pytest.mark.parametrize("N,mod,allocs", [(64, "QPSK", S1), (1024, "64QAM", K600)])
def test_composite_equals_the_separate_calls(om, torch, N, mod, allocs):
    cp, Kd = GEOM[N]
    rng = np.random.default_rng(N + 7)
    iq = make_frames(N, mod, 4, 12, rng, no_sync=(1,), late=(2,))
    n, fl = iq.shape
    rx, d_iq, nds = demod(om, N, mod, iq)
    rx.set_allocations(allocs)
    lay = om.alloc_layout([a[1] for a in allocs], [a[2] for a in allocs], n, nds, om.BITS_UNPACKED)

    def outs():
        return dict(sym=Out(torch, 2 * lay["sym"], torch.float32), llr=Out(torch, lay["llr"], torch.float32),
                    bits=Out(torch, lay["bits"], torch.uint8), beta=Out(torch, len(allocs) * n, torch.float32),
                    weight=Out(torch, len(allocs) * n, torch.float32))

    n_sym = n * nds * Kd
    p_eq, p_tsr = Out(torch, n_sym * 2, torch.float32), Out(torch, n * 4, torch.int32)
    assert rx.demod_frames(d_iq, n, fl, fl, p_eq.addr, d_tsr=p_tsr.addr) == nds
    d_a = Out(torch, n * Kd, torch.float32)
    rx.csi_frames(n, d_a.addr)
    sig = torch.from_numpy(np.array([0.01, 0.02, 0.03, 0.04])).cuda()
    for mode, nv, ds in ((om.DESPREAD_NOISE_RHO, 0.0, None), (om.DESPREAD_NOISE_GIVEN, 0.02, None), (om.DESPREAD_NOISE_SEG, 0.0, sig)):
        a, b = outs(), outs()
        rx.dft_despread_alloc_frames(p_eq.addr, n, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, a["sym"].addr, a["llr"].addr,
                                     a["bits"].addr, om.BITS_UNPACKED, a["beta"].addr, a["weight"].addr, mode, nv, ds)
        c_eq, c_tsr = Out(torch, n_sym * 2, torch.float32), Out(torch, n * 4, torch.int32)
        r = rx.demod_frames_despread_alloc(d_iq, n, fl, fl, c_eq.addr, b["sym"].addr, b["llr"].addr, b["bits"].addr, om.BITS_UNPACKED,
                                           b["beta"].addr, b["weight"].addr, mode, nv, ds, d_tsr=c_tsr.addr)
        assert r == nds
        assert np.array_equal(bits_of(p_eq.read()), bits_of(c_eq.read())) and np.array_equal(p_tsr.read(), c_tsr.read())
        for k in a:
            assert np.array_equal(a[k].read().view(np.uint8), b[k].read().view(np.uint8)), (k, mode)
    got = {k: v.read().copy() for k, v in b.items()}
    for k in ("sym", "llr", "beta", "weight"):
        assert np.isfinite(got[k]).all(), k
    for u, blk in enumerate(blocks(om, got, allocs, n, nds)):  # frame 1 has no sync, frame 2 ends in guard-failed rows
        M = allocs[u][1]
        dsym = blk["sym"].view(np.complex64).reshape(n, nds, M)
        assert blk["beta"][1] == 0 and blk["weight"][1] == 0 and not bits_of(dsym[1]).any()
        assert not bits_of(dsym[2, -1]).any() and dsym[2, 0].any() and blk["beta"][2] > 0 and blk["beta"][0] > 0
    bad = om.RxEngine(8, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    o = Out(torch, 64, torch.float32)
    with pytest.raises(ValueError, match="no allocation set"):
        bad.demod_frames_despread_alloc(d_iq, n, fl, fl, p_eq.addr, d_beta=o.addr)
    bad.set_allocations([(Kd - 11, 12, 2)])
    with pytest.raises(ValueError, match="row_len <"):
        bad.demod_frames_despread_alloc(d_iq, n, fl, fl, p_eq.addr, d_beta=o.addr)
    assert o.untouched()


# ------------------------------------------------------------------------------------------ 7. loopback
@pytest.mark.parametrize("allocs", [[(s, M, 2) for s, M, _ in S1], [(0, 12, 2), (36, 24, 2)]])
def test_loopback(om, torch, allocs):
    """modulate_frames_alloc -> flat unit channel, no noise -> demod_frames_despread_alloc: the case
    test_dft_alloc_ref_host.test_loopback_case_is_error_free_on_the_reference found error-free on the CPU"""
    N, cp, Kd, n_sym, n = 64, 16, 60, 8, 3
    L = N + cp
    tx = om.TxEngine(N, cp, N - 2, Kd, (1, 3), "QPSK")
    rx = om.RxEngine(n_sym + 1, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation="QPSK")
    rx.set_max_trials(0)
    tx.set_allocations([(s, M) for s, M, _ in allocs])
    rx.set_allocations(allocs)
    nds = 6
    bits = np.random.default_rng(71).integers(0, 2, n * nds * Kd * 2).astype(np.uint8)
    d_bits = torch.from_numpy(bits).cuda()
    d_tx = torch.zeros(n * n_sym * L * 2, dtype=torch.float32, device="cuda")
    assert tx.modulate_frames_alloc(d_bits, n, n_sym, d_tx, stream=cur(torch)) == n * n_sym
    fl = n_sym * L + L
    d_rx = torch.zeros((n, fl, 2), dtype=torch.float32, device="cuda")
    d_rx[:, 5:5 + n_sym * L, :] = d_tx.view(n, n_sym * L, 2)
    assert rx.data_symbols_per_frame(fl) == nds
    lay = om.alloc_layout([a[1] for a in allocs], [2] * len(allocs), n, nds, om.BITS_UNPACKED)
    d_eq = torch.zeros(n * nds * Kd * 2, dtype=torch.float32, device="cuda")
    hard, beta = Out(torch, lay["bits"], torch.uint8), Out(torch, len(allocs) * n, torch.float32)
    assert rx.demod_frames_despread_alloc(d_rx, n, fl, fl, d_eq, d_bits=hard.addr, bits_mode=om.BITS_UNPACKED, d_beta=beta.addr,
                                          stream=cur(torch)) == nds
    assert (beta.read() > 0).all()
    sent = bits.reshape(n, nds, Kd, 2)
    got = hard.read()
    assert got.size == sum(n * nds * M * 2 for _, M, _ in allocs)      # the allocated entries alone: nothing else is written
    for u, (s, M, _) in enumerate(allocs):
        blk = got[int(lay["bits_off"][u]):int(lay["bits_off"][u]) + n * nds * M * 2]
        assert np.array_equal(blk, sent[:, :, s:s + M].ravel()), (s, M)
    idle = Out(torch, 64, torch.float32)
    tx.set_allocations([(0, 64)])
    with pytest.raises(ValueError, match="does not fit"):
        tx.modulate_frames_alloc(d_bits, n, n_sym, idle.addr)
    assert idle.untouched()


# ------------------------------------------------------------------------------------------ 8. capture, refusals, the set's life
def test_capture_refusals_and_the_life_of_the_set(om, torch):
    row_len, allocs = SETS["S1"]
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    rows, n_seg = 17, 3
    sym, csi, sig = make_rows(np.random.default_rng(81), n_seg, rows, row_len, allocs)
    d = torch.from_numpy(sym.view(np.float32)).cuda()
    d_csi = torch.from_numpy(csi).cuda()
    lay = om.alloc_layout([a[1] for a in allocs], [a[2] for a in allocs], n_seg, rows)
    o = {k: Out(torch, 4096, torch.uint8 if k == "bits" else torch.float32) for k in WANT_ALL}

    def stage(n, stream, **kw):
        a = dict(rows=rows, row_len=row_len, seg_stride=sym.shape[1], csi=d_csi, csi_stride=csi.shape[1], rho=RHO,
                 bits_mode=om.BITS_UNPACKED, noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=0.01, sigma2=None, sym_out=o["sym"].addr)
        a.update(kw)
        rx.dft_despread_alloc_frames(d, n, a["rows"], a["row_len"], a["seg_stride"], a["csi"], a["csi_stride"], a["rho"],
                                     d_sym_out=a["sym_out"], d_llr=o["llr"].addr, d_bits=o["bits"].addr, bits_mode=a["bits_mode"],
                                     d_beta=o["beta"].addr, d_weight=o["weight"].addr, noise_mode=a["noise_mode"],
                                     noise_var=a["noise_var"], d_sigma2=a["sigma2"], stream=stream)

    with pytest.raises(ValueError, match="no allocation set"):
        stage(n_seg, cur(torch))
    with pytest.raises(ValueError, match="no allocation set"):
        rx.reserve_despread_alloc(n_seg)
    rx.set_allocations(allocs)
    for kw in (dict(row_len=59), dict(seg_stride=rows * row_len - 1), dict(csi_stride=59), dict(rows=-1), dict(noise_mode=3),
               dict(noise_var=0.0), dict(noise_mode=om.DESPREAD_NOISE_SEG), dict(rho=-1.0), dict(bits_mode=om.BITS_NONE),
               dict(sym_out=d.data_ptr()), dict(rows=1 << 41, seg_stride=1 << 60)):
        with pytest.raises(ValueError, match="ofdm_dft_despread_alloc_frames"):
            stage(n_seg, cur(torch), **kw)
    with pytest.raises(ValueError, match="ofdm_dft_despread_alloc_frames"):
        stage(-1, cur(torch))
    with pytest.raises(ValueError, match="workgroups"):      # 3 allocations x 2^30 segments of one group: past the grid's range
        stage(1 << 30, cur(torch), rows=1, seg_stride=60)
    with pytest.raises(ValueError, match="no pointer"):
        rx.dft_despread_alloc_frames(d, n_seg, rows, row_len, sym.shape[1], d_csi, csi.shape[1], RHO, stream=cur(torch))
    for bad in ([(0, 12, 2), (11, 12, 2)], [(0, 7, 2)], [(0, 12, 1)]):                   # a refused set leaves the one in force
        with pytest.raises(ValueError, match="ofdm_rx_set_allocations"):
            rx.set_allocations(bad)
    torch.cuda.synchronize()
    assert all(v.untouched() for v in o.values())            # every refusal so far left the outputs alone

    size = dict(sym=2 * lay["sym"], llr=lay["llr"], bits=lay["llr"], beta=len(allocs) * n_seg, weight=len(allocs) * n_seg)
    outs = {k: torch.zeros(size[k], dtype=torch.uint8 if k == "bits" else torch.float32, device="cuda") for k in WANT_ALL}

    def call(n, stream):
        rx.dft_despread_alloc_frames(d, n, rows, row_len, sym.shape[1], d_csi, csi.shape[1], RHO, outs["sym"], outs["llr"], outs["bits"],
                                     om.BITS_UNPACKED, outs["beta"], outs["weight"], om.DESPREAD_NOISE_GIVEN, 0.01, stream=stream)

    rx.reserve_despread_alloc(n_seg - 1)                     # one segment short of the batch that is captured second
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(n_seg - 1, s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["weight"][:len(allocs) * (n_seg - 1)] > 0).all()) and bool(eager["llr"].any())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(n_seg - 1, torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="ofdm_rx_reserve_despread_alloc"):
            call(n_seg, torch.cuda.current_stream().cuda_stream)        # a larger batch: the table would have to grow
    assert not outs["weight"].any()                          # capture enqueues nothing
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k

    # more single-M plans than the cache holds, between two stage calls: the set does not live there
    call(n_seg, cur(torch))
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in outs.items()}
    for M in (2, 3, 4, 5, 6, 8, 9, 10, 15):
        rx.reserve_despread(M, 1)
    for v in outs.values():
        v.zero_()
    call(n_seg, cur(torch))
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], before[k]), k
    # the set replaced between two calls takes effect; cleared, the calls refuse
    rx.set_allocations([(36, 24, 6), (0, 12, 2)])
    for v in outs.values():
        v.zero_()
    call(n_seg, cur(torch))
    torch.cuda.synchronize()
    n0, n2 = n_seg * rows * 12, n_seg * rows * 24
    b_sym, n_sym = before["sym"].cpu().numpy(), outs["sym"].cpu().numpy()
    assert np.array_equal(bits_of(n_sym[:2 * n2]), bits_of(b_sym[2 * (n0 + n2):2 * (n0 + 2 * n2)]))
    assert np.array_equal(bits_of(n_sym[2 * n2:2 * (n2 + n0)]), bits_of(b_sym[:2 * n0]))
    assert not n_sym[2 * (n2 + n0):].any()
    rx.set_allocations([])
    with pytest.raises(ValueError, match="no allocation set"):
        call(n_seg, cur(torch))
