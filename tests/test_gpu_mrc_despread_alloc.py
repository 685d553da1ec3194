"""Receive diversity for multi-user allocations of DFT-spread OFDM on the GPU (-m gpu): ofdm_combine_despread_alloc_frames and
ofdm_rx_demod_frames_mrc_despread_alloc.  The contract (include/ofdm_mi355x.h) is one sentence: block u of every output holds,
bit for bit, what ofdm_combine_despread_frames writes for M_u and mod_u on a dense copy of the allocation's columns of every
branch -- so the existing call on a gather made with torch, on a second handle, is the reference for all six outputs, and
tests/mrc_despread_alloc_ref.py (fp64 on the float32 combined symbols) for sym at the suite's 1e-5 bar.  Every output sits
between poisoned guard bands.

Sets: those of test_gpu_dft_alloc.py.  S1 one M at several modulations; S2 odd starts, M = 1 and gaps, with an even and an odd row
length (the row alignment then alternates); S3 the 20 MHz row; S4 both size classes with rows of more than 64 lanes; S5 the cap of
32 allocations.  B = 1, 2, 3, 8 (half a load round, one round, an odd tail, the most); rows 1 and the set's largest
rows_per_group + 1; n_seg 1 and 3; the input base on a 16-byte address, and on an 8-byte address with an odd unit stride and an
odd n_seg, so that the alignment alternates between branches too; both noise modes.  Combined in four runs per set, not crossed."""
import ctypes as C

import numpy as np
import pytest

import mrc_despread_alloc_ref as aref
from conftest import TOL_MAX, relerr
from test_gpu_csi import Out, cur, demod
from test_gpu_dft_alloc import K600, NAME, S1, SETS, max_rpg
from test_gpu_dft_spread import bits_of, put
from test_gpu_mrc_despread import RHO, WANT_ALL
from test_gpu_mrc_despread import run as run_single
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

MY_SETS = {k: SETS[k] for k in ("S1", "S2-80", "S2-81", "S3", "S4", "S5")}


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


def odd_extra(rows, row_len):
    """stride padding that makes the unit stride odd: on an 8-byte base the units' alignment then alternates"""
    return 1 + (rows * row_len) % 2


def make_units(rng, B, n_seg, rows, row_len, allocs, extra=0, csi_extra=3):
    """-> sym [B*n_seg][rows*row_len + extra] complex64, csi [B*n_seg][row_len + csi_extra] float32, sigma2 [B*n_seg]: every
    allocation a user of its own, the same spread constellation rows per segment through B channels and one-tap MMSE equalisers;
    unit g = b*n_seg + s; gaps and stride padding hold noise"""
    import math
    import dft_spread_ref
    from oracle import ofdm_oracle as orc
    n = rows * row_len
    sym = (rng.standard_normal((B * n_seg, n + extra)) + 1j * rng.standard_normal((B * n_seg, n + extra))).astype(np.complex64)
    csi = rng.uniform(0.1, 1.0, (B * n_seg, row_len + csi_extra)).astype(np.float32)
    sig = np.array([(0.02, 0.05, 0.1)[(g // n_seg + g % n_seg) % 3] for g in range(B * n_seg)])
    for s in range(n_seg):
        for start, M, bps in allocs:
            x = dft_spread_ref.spread(orc.map_bits(rng.integers(0, 2, rows * M * bps), NAME[bps]).reshape(rows, M))
            for b in range(B):
                g = b * n_seg + s
                a = rng.uniform(0.02, 2.0, M)
                w = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))) * math.sqrt(sig[g] / 2)
                sym[g, :n].reshape(rows, row_len)[:, start:start + M] = (a / (a + RHO)) * (x + w / np.sqrt(a))
                csi[g, start:start + M] = a
    return sym, csi, sig


def sizes(om, torch, allocs, n_seg, rows, bits_mode):
    lay = om.alloc_layout([a[1] for a in allocs], [a[2] for a in allocs], n_seg, rows, bits_mode)
    per_row = len(allocs) * n_seg * rows
    return lay, dict(sym=(2 * lay["sym"], torch.float32), llr=(lay["llr"], torch.float32), bits=(lay["bits"], torch.uint8),
                     beta=(per_row, torch.float32), weight=(per_row, torch.float32), comb=(2 * lay["sym"], torch.float32))


def run_alloc(om, torch, rx, sym, csi, B, rows, row_len, allocs, noise, want=WANT_ALL, base_off=0, bits_mode=None, rho=RHO):
    """combine_despread_alloc_frames on host arrays -> dict of host arrays in the contract's layout.  noise: ("given", [B]) or
    ("seg", [B*n_seg])"""
    n_seg = sym.shape[0] // B
    bits_mode = om.BITS_UNPACKED if bits_mode is None else bits_mode
    t, addr = put(torch, sym, base_off)
    d_csi = torch.from_numpy(np.ascontiguousarray(csi)).cuda()
    _, size = sizes(om, torch, allocs, n_seg, rows, bits_mode)
    o = {k: (Out(torch, *size[k]) if k in want else None) for k in WANT_ALL}
    d_sig = torch.from_numpy(np.asarray(noise[1], np.float64)).cuda() if noise[0] == "seg" else None
    rx.combine_despread_alloc_frames(addr, B, n_seg, rows, row_len, sym.shape[1], d_csi, csi.shape[1], rho,
                                     noise_var=list(noise[1]) if noise[0] == "given" else None, d_sigma2=d_sig,
                                     d_sym_out=o["sym"] and o["sym"].addr, d_llr=o["llr"] and o["llr"].addr,
                                     d_bits=o["bits"] and o["bits"].addr, bits_mode=bits_mode if "bits" in want else om.BITS_NONE,
                                     d_beta=o["beta"] and o["beta"].addr, d_weight=o["weight"] and o["weight"].addr,
                                     d_comb=o["comb"] and o["comb"].addr, stream=cur(torch))
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
        cut = dict(sym=(2 * int(lay["sym_off"][u]), 2 * n), comb=(2 * int(lay["sym_off"][u]), 2 * n), llr=(int(lay["llr_off"][u]), n * bps),
                   bits=(int(lay["bits_off"][u]), nb), beta=(u * n_seg * rows, n_seg * rows), weight=(u * n_seg * rows, n_seg * rows))
        out.append({k: (None if got[k] is None else got[k][cut[k][0]:cut[k][0] + cut[k][1]]) for k in WANT_ALL})
    return out


def gathered(torch, sym, csi, rows, row_len, start, M):
    """columns start .. start+M-1 of every row of every unit and of every unit's csi row, dense, gathered with torch on the device"""
    units = sym.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(sym[:, :rows * row_len]).view(np.float32)).cuda().view(units, rows, row_len, 2)
    g = t[:, :, start:start + M, :].contiguous().cpu().numpy().view(np.complex64).reshape(units, rows * M)
    c = torch.from_numpy(np.ascontiguousarray(csi)).cuda()[:, start:start + M].contiguous().cpu().numpy()
    return g, c


def reference(om, torch, rxg, sym, csi, B, rows, row_len, allocs, noise, only=None):
    """the existing single-M call on the gathered copy of every allocation (of those in `only`): a list of dicts"""
    out = []
    for u, (start, M, bps) in enumerate(allocs):
        if only is not None and u not in only:
            out.append(None)
            continue
        g, c = gathered(torch, sym, csi, rows, row_len, start, M)
        out.append(run_single(om, torch, rxg, g, c, B, rows, M, NAME[bps], noise))
    return out


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_blocks_equal(got_blocks, want_blocks, tag=""):
    for u, (g, w) in enumerate(zip(got_blocks, want_blocks)):
        if w is None:
            continue
        for k in WANT_ALL:
            if g[k] is not None:
                assert same(g[k], w[k]), (tag, u, k)


def assert_finite(got):
    for k in ("sym", "llr", "beta", "weight", "comb"):
        if got[k] is not None:
            assert np.isfinite(got[k]).all(), k


def unit_sigma2(noise, B, n_seg):
    s2 = np.asarray(noise[1], np.float64)
    return (np.repeat(s2, n_seg) if noise[0] == "given" else s2).reshape(B, n_seg)


# ------------------------------------------------------------------------------------------ 1. block equality, fp64, packed bits
@pytest.mark.parametrize("name", list(MY_SETS))
def test_every_block_is_the_existing_call_on_the_gathered_columns(om, torch, rx0, rxg, name):
    row_len, allocs = MY_SETS[name]
    assert aref.check_set(allocs, row_len) is None
    rx0.set_allocations(allocs)
    R = max_rpg(om, allocs) + 1
    rng = np.random.default_rng(len(name) + row_len)
    packable = all(M * bps % 8 == 0 for _, M, bps in allocs)
    for B, rows, n_seg, base_off, kind in ((1, 1, 1, 0, "given"), (2, R, 3, 8, "seg"), (3, R, 1, 8, "given"), (8, 1, 3, 0, "seg")):
        extra = odd_extra(rows, row_len) if base_off else 0
        sym, csi, sig = make_units(rng, B, n_seg, rows, row_len, allocs, extra=extra)
        noise = ("seg", sig) if kind == "seg" else ("given", sig[::n_seg])
        got = run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, noise, base_off=base_off)
        want = reference(om, torch, rxg, sym, csi, B, rows, row_len, allocs, noise)
        mine = blocks(om, got, allocs, n_seg, rows)
        assert_blocks_equal(mine, want, (name, B, rows, n_seg, kind))
        assert_finite(got)
        assert (got["beta"] > 0).all() and (got["weight"] > 0).all() and got["llr"].any()
        # sym against fp64 on the float32 combined symbols; comb bit for bit the float32 restatement
        z = sym[:, :rows * row_len].reshape(B, n_seg, rows, row_len)
        res = aref.combine_despread_alloc(z, csi[:, :row_len].reshape(B, n_seg, row_len), allocs, np.float32(RHO),
                                          unit_sigma2(noise, B, n_seg))
        assert same(got["comb"].view(np.complex64), res["comb"])
        for u, (_, M, _) in enumerate(allocs):
            for s in range(n_seg):
                dev = mine[u]["sym"].view(np.complex64).reshape(n_seg, rows * M)[s]
                e = relerr(dev, res["segs"][u][s]["sym"].ravel())
                assert e < TOL_MAX, (name, B, u, s, e)
        if kind == "seg" and B == 2:                         # packed bits where every allocation fills bytes, refused elsewhere
            if packable:
                gp = run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, noise, want=("bits",), base_off=base_off,
                               bits_mode=om.BITS_PACKED)
                for u, (b, w) in enumerate(zip(blocks(om, gp, allocs, n_seg, rows, om.BITS_PACKED), want)):
                    assert np.array_equal(b["bits"], np.packbits(w["bits"])), (name, u)
            else:
                o = Out(torch, 64, torch.uint8)
                t, addr = put(torch, sym, base_off)
                d_csi = torch.from_numpy(csi).cuda()
                with pytest.raises(ValueError, match="packed bits need"):
                    rx0.combine_despread_alloc_frames(addr, B, n_seg, rows, row_len, sym.shape[1], d_csi, csi.shape[1], RHO,
                                                      noise_var=[0.1] * B, d_bits=o.addr, bits_mode=om.BITS_PACKED, stream=cur(torch))
                assert o.untouched()


def test_one_allocation_over_the_row_equals_the_existing_call_on_the_same_buffer(om, torch, rx0, rxg):
    B, rows, n_seg, allocs = 3, 17, 3, [(0, 60, 4)]
    sym, csi, sig = make_units(np.random.default_rng(6), B, n_seg, rows, 60, allocs)
    rx0.set_allocations(allocs)
    got = run_alloc(om, torch, rx0, sym, csi, B, rows, 60, allocs, ("seg", sig))
    want = run_single(om, torch, rxg, sym, csi, B, rows, 60, "16QAM", ("seg", sig))
    for k in WANT_ALL:
        assert same(got[k], want[k]), k


# ------------------------------------------------------------------------------------------ 2. the same bits
@pytest.mark.parametrize("name", ["S1", "S2-81"])
def test_same_bits_invariants(om, torch, rx0, name):
    row_len, allocs = MY_SETS[name]
    B, rows, n_seg = 3, max_rpg(om, allocs) + 1, 3
    rng = np.random.default_rng(31)
    extra = odd_extra(rows, row_len)
    sym, csi, sig = make_units(rng, B, n_seg, rows, row_len, allocs, extra=extra)
    noise = ("seg", sig)
    rx0.set_allocations(allocs)
    full = run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, noise, base_off=8)
    for k in WANT_ALL:                                       # each output alone
        one = run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, noise, want=(k,), base_off=8)
        assert same(one[k], full[k]), k
    again = run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, noise, base_off=0)      # a repeated call, the other base
    assert all(same(again[k], full[k]) for k in WANT_ALL)
    base = blocks(om, full, allocs, n_seg, rows)
    for s in range(n_seg):                                   # a segment alone, dense and aligned
        pick = [b * n_seg + s for b in range(B)]
        alone = blocks(om, run_alloc(om, torch, rx0, np.ascontiguousarray(sym[pick, :rows * row_len]), csi[pick], B, rows, row_len,
                                     allocs, ("seg", sig[pick])), allocs, 1, rows)
        for u, (_, M, bps) in enumerate(allocs):
            for k, width in (("sym", 2 * rows * M), ("comb", 2 * rows * M), ("llr", rows * M * bps), ("bits", rows * M * bps),
                             ("beta", rows), ("weight", rows)):
                assert same(alone[u][k], base[u][k][s * width:(s + 1) * width]), (s, u, k)
    # NaN in the gaps, in the stride padding and in the gaps of csi: never read for data
    covered = np.zeros(row_len, bool)
    for s, M, _ in allocs:
        covered[s:s + M] = True
    z2, c2 = sym.copy(), csi.copy()
    for g in range(B * n_seg):
        z2[g, :rows * row_len].reshape(rows, row_len)[:, ~covered] = complex(np.nan, np.nan)
    z2[:, rows * row_len:] = complex(np.nan, np.nan)
    c2[:, :row_len][:, ~covered] = np.nan
    c2[:, row_len:] = np.nan
    poisoned = run_alloc(om, torch, rx0, z2, c2, B, rows, row_len, allocs, noise, base_off=8)
    assert all(same(poisoned[k], full[k]) for k in WANT_ALL)
    # the list in another order: the same blocks, permuted
    perm = allocs[1:] + allocs[:1]
    rx0.set_allocations(perm)
    turned = blocks(om, run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, perm, noise, base_off=8), perm, n_seg, rows)
    assert_blocks_equal(turned, base[1:] + base[:1], "permuted")
    rx0.set_allocations(allocs)
    # user v's data and channel changed: every other user's block keeps its bits, user v's does not
    for v, (s, M, _) in enumerate(allocs):
        z3, c3 = sym.copy(), csi.copy()
        for g in range(B * n_seg):
            z3[g, :rows * row_len].reshape(rows, row_len)[:, s:s + M] *= np.complex64(0.5 + 0.25j)
        c3[:, s:s + M] *= np.float32(0.7)
        other = blocks(om, run_alloc(om, torch, rx0, z3, c3, B, rows, row_len, allocs, noise, base_off=8), allocs, n_seg, rows)
        for u in range(len(allocs)):
            keeps = all(same(other[u][k], base[u][k]) for k in WANT_ALL)
            assert keeps == (u != v), (u, v)


# ------------------------------------------------------------------------------------------ 3. planted values
def test_planted_values_stay_in_their_allocation(om, torch, rx0, rxg):
    row_len, allocs = MY_SETS["S1"]                          # users at 0..11, 12..35, 36..59
    B, rows, n_seg = 3, 5, 3
    sym, csi, sig = make_units(np.random.default_rng(41), B, n_seg, rows, row_len, allocs)
    noise = ("seg", sig)
    rx0.set_allocations(allocs)
    clean = blocks(om, run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, noise), allocs, n_seg, rows)
    plants = []                                              # (the allocation hit, what was planted)
    z, c = sym.copy(), csi.copy()
    zz = lambda b, s: z[b * n_seg + s].reshape(rows, row_len)                            # noqa: E731
    zz(1, 0)[1, 3] = complex(np.nan, 0.1)                    # user 0: non-finite symbols in branch 1
    zz(1, 0)[4, 11] = complex(0.1, -np.inf)
    plants.append((0, "non-finite symbols"))
    for j, a in zip((13, 20, 35), (0.0, -1.0, np.nan)):      # user 1: unusable entries in branch 2
        c[2 * n_seg + 0, j] = a
    plants.append((1, "zero, negative and NaN csi"))
    zz(0, 0)[2, 36:60] = 0                                   # user 2: branch 0 misses row 2 (the guard-failed row)
    plants.append((2, "a zero row in one branch"))
    got = run_alloc(om, torch, rx0, z, c, B, rows, row_len, allocs, noise)
    mine = blocks(om, got, allocs, n_seg, rows)
    assert_blocks_equal(mine, reference(om, torch, rxg, z, c, B, rows, row_len, allocs, noise), "planted")
    assert_finite(got)
    for u in range(3):
        assert not all(same(mine[u][k], clean[u][k]) for k in WANT_ALL), plants[u]
    beta2 = mine[2]["beta"].reshape(n_seg, rows)
    assert 0 < beta2[0, 2] < clean[2]["beta"].reshape(n_seg, rows)[0, 2]                  # the row of two branches: a smaller gain
    assert same(np.delete(beta2, 2, axis=1), np.delete(clean[2]["beta"].reshape(n_seg, rows), 2, axis=1))
    # one plant at a time: the other allocations' blocks are untouched, and so are the gathered call's outputs for them
    for v, start, stop in ((0, 0, 12), (1, 12, 36), (2, 36, 60)):
        z1, c1 = sym.copy(), csi.copy()
        for g in range(B * n_seg):
            z1[g].reshape(rows, row_len)[:, start:stop] = z[g].reshape(rows, row_len)[:, start:stop]
        c1[:, start:stop] = c[:, start:stop]
        one = blocks(om, run_alloc(om, torch, rx0, z1, c1, B, rows, row_len, allocs, noise), allocs, n_seg, rows)
        ref1 = reference(om, torch, rxg, z1, c1, B, rows, row_len, allocs, noise)
        assert_blocks_equal(one, ref1, ("one plant", v))
        for u in range(3):
            if u != v:
                assert all(same(one[u][k], clean[u][k]) for k in WANT_ALL), (u, v)
                assert all(same(ref1[u][k], clean[u][k]) for k in WANT_ALL), (u, v)
    # a beta that underflows in one user's columns: csi is a float32 denormal there in every branch of segment 1, so
    # float(1/beta) is not finite and the rows are not usable although every symbol was combined; the other users carry on
    c2 = csi.copy()
    for b in range(B):
        c2[b * n_seg + 1, 36:60] = 1e-42
    got = run_alloc(om, torch, rx0, sym, c2, B, rows, row_len, allocs, noise)
    mine = blocks(om, got, allocs, n_seg, rows)
    assert_blocks_equal(mine, reference(om, torch, rxg, sym, c2, B, rows, row_len, allocs, noise, only=(2,)), "underflow")
    assert_finite(got)
    b2, w2 = mine[2]["beta"].reshape(n_seg, rows), mine[2]["weight"].reshape(n_seg, rows)
    assert not bits_of(b2[1]).any() and not bits_of(w2[1]).any() and (b2[[0, 2]] > 0).all() and (w2[[0, 2]] > 0).all()
    assert mine[2]["comb"].reshape(n_seg, -1)[1].any() and not bits_of(mine[2]["sym"].reshape(n_seg, -1)[1]).any()
    assert all(same(mine[u][k], clean[u][k]) for u in (0, 1) for k in WANT_ALL)
    # a unit's variance is the receiver's, shared by its allocations: <= 0 or NaN erases that unit for every user of segment 0
    # and leaves the other segments' bits alone
    for bad in (0.0, np.nan, -0.5):
        s2 = sig.copy()
        s2[1 * n_seg + 0] = bad                              # branch 1 of segment 0
        got = run_alloc(om, torch, rx0, sym, csi, B, rows, row_len, allocs, ("seg", s2))
        mine = blocks(om, got, allocs, n_seg, rows)
        pick = [b * n_seg + s for b in (0, 2) for s in range(n_seg)]
        others = blocks(om, run_alloc(om, torch, rx0, np.ascontiguousarray(sym[pick]), csi[pick], 2, rows, row_len, allocs,
                                      ("seg", sig[pick])), allocs, n_seg, rows)
        assert_finite(got)
        for u in range(3):
            for k in WANT_ALL:
                per = mine[u][k].size // n_seg
                assert same(mine[u][k][:per], others[u][k][:per]), (bad, u, k)           # segment 0: branches 0 and 2 carry
                assert same(mine[u][k][per:], clean[u][k][per:]), (bad, u, k)
        assert_blocks_equal(mine, reference(om, torch, rxg, sym, csi, B, rows, row_len, allocs, ("seg", s2), only=(1,)), ("variance", bad))


# ------------------------------------------------------------------------------------------ 4. the composite call
@pytest.mark.parametrize("N,mod,allocs", [(64, "QPSK", S1), (1024, "64QAM", K600)])
def test_composite_equals_the_separate_calls(om, torch, N, mod, allocs):
    cp, Kd = GEOM[N]
    rng = np.random.default_rng(N + 11)
    B, nf = 2, 3
    iq = make_frames(N, mod, B * nf, 12, rng, no_sync=(nf + 1,), late=(2,))            # branch 1 of frame 1 is noise only
    n, fl = iq.shape
    rx, d_iq, nds = demod(om, N, mod, iq)
    rx.set_allocations(allocs)
    _, size = sizes(om, torch, allocs, nf, nds, om.BITS_UNPACKED)

    def outs():
        return {k: Out(torch, *size[k]) for k in WANT_ALL}

    n_eq = n * nds * Kd
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
        rx.combine_despread_alloc_frames(p_eq.addr, B, nf, nds, Kd, nds * Kd, d_a.addr, Kd, rx.csi_rho, nv, ds, a["sym"].addr,
                                         a["llr"].addr, a["bits"].addr, om.BITS_UNPACKED, a["beta"].addr, a["weight"].addr, a["comb"].addr)
        c_eq, c_tsr = Out(torch, n_eq * 2, torch.float32), Out(torch, n * 4, torch.int32)
        r = rx.demod_frames_mrc_despread_alloc(d_iq, B, nf, fl, fl, c_eq.addr, nv, ds, b["sym"].addr, b["llr"].addr, b["bits"].addr,
                                               om.BITS_UNPACKED, b["beta"].addr, b["weight"].addr, b["comb"].addr, d_tsr=c_tsr.addr)
        assert r == nds
        assert np.array_equal(bits_of(p_eq.read()), bits_of(c_eq.read())) and np.array_equal(p_tsr.read(), c_tsr.read())
        for k in a:
            assert same(a[k].read(), b[k].read()), (k, noise[0])
        got = {k: v.read().copy() for k, v in b.items()}
        assert_finite(got)
        eq = p_eq.read().view(np.complex64).reshape(B, nf, nds, Kd)
        assert not eq[0, 2, -1].any()                        # frame 2 of branch 0 ends in guard-failed rows: branch 1 carries them
        for u, blk in enumerate(blocks(om, got, allocs, nf, nds)):
            beta = blk["beta"].reshape(nf, nds)
            assert (beta > 0).all() and beta[2, -1] < beta[2, 0], u      # frame 1: branch 0 alone carries every row
    bad = om.RxEngine(8, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    o = Out(torch, 64, torch.float32)
    with pytest.raises(ValueError, match="no allocation set"):
        bad.demod_frames_mrc_despread_alloc(d_iq, B, nf, fl, fl, p_eq.addr, noise_var=[0.1] * B, d_beta=o.addr)
    bad.set_allocations([(Kd - 11, 12, 2)])
    with pytest.raises(ValueError, match="row_len <"):
        bad.demod_frames_mrc_despread_alloc(d_iq, B, nf, fl, fl, p_eq.addr, noise_var=[0.1] * B, d_beta=o.addr)
    assert o.untouched()


# ------------------------------------------------------------------------------------------ 5. capture, refusals, the set's life
def test_capture_refusals_and_the_life_of_the_set(om, torch):
    row_len, allocs = MY_SETS["S1"]
    rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
    B, rows, n_seg = 2, 17, 3
    sym, csi, sig = make_units(np.random.default_rng(81), B, n_seg, rows, row_len, allocs)
    d = torch.from_numpy(sym.view(np.float32)).cuda()
    d_csi = torch.from_numpy(csi).cuda()
    d_sig = torch.from_numpy(sig).cuda()
    o = {k: Out(torch, 4096, torch.uint8 if k == "bits" else torch.float32) for k in WANT_ALL}

    def stage(n, stream, **kw):
        a = dict(n_branch=B, rows=rows, row_len=row_len, seg_stride=sym.shape[1], csi=d_csi, csi_stride=csi.shape[1], rho=RHO,
                 bits_mode=om.BITS_UNPACKED, noise_var=[0.02, 0.05], sigma2=None, sym_out=o["sym"].addr, comb=o["comb"].addr)
        a.update(kw)
        rx.combine_despread_alloc_frames(d, a["n_branch"], n, a["rows"], a["row_len"], a["seg_stride"], a["csi"], a["csi_stride"],
                                         a["rho"], noise_var=a["noise_var"], d_sigma2=a["sigma2"], d_sym_out=a["sym_out"],
                                         d_llr=o["llr"].addr, d_bits=o["bits"].addr, bits_mode=a["bits_mode"], d_beta=o["beta"].addr,
                                         d_weight=o["weight"].addr, d_comb=a["comb"], stream=stream)

    with pytest.raises(ValueError, match="no allocation set"):
        stage(n_seg, cur(torch))
    rx.set_allocations(allocs)
    who = "ofdm_combine_despread_alloc_frames"
    for kw in (dict(row_len=59), dict(seg_stride=rows * row_len - 1), dict(csi_stride=59), dict(rows=-1), dict(noise_var=[0.02, 0.0]),
               dict(noise_var=[0.02, float("nan")]), dict(rho=-1.0), dict(bits_mode=om.BITS_NONE), dict(bits_mode=7),
               dict(sym_out=d.data_ptr()), dict(comb=d.data_ptr()), dict(csi=None), dict(n_branch=0, noise_var=[]),
               dict(n_branch=9, noise_var=[0.1] * 9), dict(rows=1 << 41, seg_stride=1 << 60)):
        with pytest.raises(ValueError, match=who):
            stage(n_seg, cur(torch), **kw)
    with pytest.raises(ValueError, match=who):
        stage(-1, cur(torch))
    rx.set_allocations([(0, 12, 2), (12, 25, 2)])            # 25 QPSK symbols do not fill bytes
    with pytest.raises(ValueError, match="packed bits need"):
        stage(n_seg, cur(torch), bits_mode=om.BITS_PACKED)
    rx.set_allocations(allocs)
    with pytest.raises(ValueError, match="workgroups"):      # 3 allocations x 2^30 segments of one group: past the grid's range
        stage(1 << 30, cur(torch), n_branch=1, noise_var=[0.1], rows=1, seg_stride=60)
    with pytest.raises(ValueError, match="index range"):     # n_branch*n_seg > 2^31
        stage((1 << 30) + 1, cur(torch), rows=1, seg_stride=60)
    with pytest.raises(ValueError, match="no pointer"):
        rx.combine_despread_alloc_frames(d, B, n_seg, rows, row_len, sym.shape[1], d_csi, csi.shape[1], RHO, noise_var=[0.1, 0.1],
                                         stream=cur(torch))
    from ofdm_mi355x import _lib
    out = _lib.MrcDespreadOut(llr=o["llr"].addr, sym=o["sym"].addr)
    two = (C.c_double * 2)(0.1, 0.2)
    assert rx.lib.ofdm_combine_despread_alloc_frames(rx._h, d.data_ptr(), B, n_seg, rows, row_len, sym.shape[1], d_csi.data_ptr(),
                                                     csi.shape[1], RHO, om.MRC_NOISE_EST, two, d_sig.data_ptr(), om.BITS_NONE,
                                                     C.byref(out), None) == -1
    assert b"OFDM_MRC_NOISE_EST" in rx.lib.ofdm_last_error()
    for bad in ([(0, 12, 2), (11, 12, 2)], [(0, 7, 2)], [(0, 12, 1)]):                   # a refused set leaves the one in force
        with pytest.raises(ValueError, match="ofdm_rx_set_allocations"):
            rx.set_allocations(bad)
    with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc_despread_alloc"):
        rx.reserve_mrc_despread_alloc(9, 1, 60)
    stage(0, cur(torch))                                     # zero counts: no-ops
    stage(n_seg, cur(torch), rows=0, seg_stride=0)
    torch.cuda.synchronize()
    assert all(v.untouched() for v in o.values())            # every refusal so far left the outputs alone

    _, size = sizes(om, torch, allocs, n_seg, rows, om.BITS_UNPACKED)
    outs = {k: torch.zeros(size[k][0], dtype=size[k][1], device="cuda") for k in WANT_ALL}

    def call(n, stream):
        rx.combine_despread_alloc_frames(d, B, n, rows, row_len, sym.shape[1], d_csi, csi.shape[1], RHO, [0.02, 0.05], None, outs["sym"],
                                         outs["llr"], outs["bits"], om.BITS_UNPACKED, outs["beta"], outs["weight"], outs["comb"],
                                         stream=stream)

    # a batch of n < n_seg segments reads the same buffer with its branches n*stride apart: other units, the same in both runs
    rx.reserve_mrc_despread_alloc(B, n_seg - 1, row_len)     # one segment per branch short of the batch that is captured second
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(n_seg - 1, s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert bool((eager["weight"][:len(allocs) * (n_seg - 1) * rows] > 0).all()) and bool(eager["llr"].any())
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                      # a linear capture: one stream, no parallel branches
        call(n_seg - 1, torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match="ofdm_rx_reserve_mrc_despread_alloc"):
            call(n_seg, torch.cuda.current_stream().cuda_stream)        # a larger batch: the table would have to grow
    assert not outs["weight"].any()                          # capture enqueues nothing
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k

    # more single-M plans than the cache holds, between two stage calls: the set does not live there
    call(n_seg, cur(torch))
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    for M in (2, 3, 4, 5, 6, 8, 9, 10, 15):
        rx.reserve_despread(M, 1)
    for v in outs.values():
        v.zero_()
    call(n_seg, cur(torch))
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], eager[k]), k
    # a refused set left the previous one in force (above); the set replaced between two calls takes effect; cleared, the calls refuse
    rx.set_allocations([(36, 24, 6), (0, 12, 2)])
    for v in outs.values():
        v.zero_()
    call(n_seg, cur(torch))
    torch.cuda.synchronize()
    n0, n2 = n_seg * rows * 12, n_seg * rows * 24
    b_sym, n_sym = eager["sym"].cpu().numpy(), outs["sym"].cpu().numpy()
    assert np.array_equal(bits_of(n_sym[:2 * n2]), bits_of(b_sym[2 * (n0 + n2):2 * (n0 + 2 * n2)]))
    assert np.array_equal(bits_of(n_sym[2 * n2:2 * (n2 + n0)]), bits_of(b_sym[:2 * n0]))
    assert not n_sym[2 * (n2 + n0):].any()
    b_beta, n_beta = eager["beta"].cpu().numpy(), outs["beta"].cpu().numpy()
    assert np.array_equal(n_beta[:n_seg * rows], b_beta[2 * n_seg * rows:]) and np.array_equal(n_beta[n_seg * rows:2 * n_seg * rows], b_beta[:n_seg * rows])
    rx.set_allocations([])
    with pytest.raises(ValueError, match="no allocation set"):
        call(n_seg, cur(torch))


# ------------------------------------------------------------------------------------------ 6. the link, end to end on the device
def test_link_case_decodes_where_neither_branch_does(om, torch):
    """mrc_despread_alloc_cases end to end: turbo_encode_frames -> modulate_frames_alloc -> channel (taps and noise seed per
    branch, into one IQ buffer of 2 * 64 frames) -> demod_frames_mrc_despread_alloc -> the LLRs back into row order ->
    turbo_decode_frames gives every block back; each branch alone through demod_frames_despread_alloc with the noise given loses
    the blocks it loses on the oracle's receiver (mrc_despread_alloc_cases.LOST_AT_LEVEL)."""
    import mrc_despread_alloc_cases as ac
    n, L, B = ac.N_FRAMES, ac.N + ac.CP, ac.N_BRANCH
    txe = om.TxEngine(ac.N, ac.CP, ac.KS, ac.KD, (1, 3), ac.MOD)
    rxe = om.RxEngine(ac.N_SYM, ac.N, ac.CP, ac.KS, (1, 3), ac.KD, ac.SNR_ARG, ac.GATE, modulation=ac.MOD)
    rxe.set_max_trials(0)
    txe.set_allocations([(s, M) for s, M, _ in ac.ALLOCS])
    rxe.set_allocations(ac.ALLOCS)
    info = ac.info_bits()
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    d_coded = om.DeviceBuffer(n * ac.SEG_BITS)
    txe.turbo_encode_frames(d_info, n, 1, ac.K, ac.F1, ac.F2, d_coded, ac.SEG_BITS)
    fl_tx, fl = ac.N_SYM * L, ac.FRAME_LEN
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(B * n * fl * 8)
    assert txe.modulate_frames_alloc(d_coded, n, ac.N_SYM, d_tx) == n * ac.N_SYM
    for b in range(B):
        taps = np.asarray(ac.TAPS[b]).astype(np.complex64)
        d_taps = om.DeviceBuffer(taps.nbytes).upload(taps)
        txe.channel(d_tx, n, fl_tx, fl_tx, d_taps, len(taps), d_rx.data_ptr() + b * n * fl * 8, fl, fl, noise_var=ac.NOISE_VAR,
                    seed=ac.SEED_NOISE + b)
    assert rxe.data_symbols_per_frame(fl) == ac.N_DSYM
    d_eq = om.DeviceBuffer(B * n * ac.N_DSYM * ac.KD * 8)
    d_blk = om.DeviceBuffer(n * ac.SEG_BITS * 4)             # allocation-major
    d_llr = om.DeviceBuffer(n * ac.SEG_BITS * 4)             # row order
    d_beta = om.DeviceBuffer(len(ac.ALLOCS) * n * ac.N_DSYM * 4)
    d_bits = om.DeviceBuffer(n * ac.K)

    def lost():
        rows = ac.rows_from_blocks(d_blk.download(np.float32, n * ac.SEG_BITS))
        d_llr.upload(np.ascontiguousarray(rows))
        rxe.turbo_decode_frames(d_llr, n, ac.SEG_BITS, 1, ac.K, ac.F1, ac.F2, ac.N_ITER, d_bits=d_bits)
        return int((d_bits.download(np.uint8, n * ac.K).reshape(n, 1, ac.K) != info).any(axis=(1, 2)).sum())

    assert rxe.demod_frames_mrc_despread_alloc(d_rx, B, n, fl, fl, d_eq, noise_var=[ac.NOISE_VAR] * B, d_llr=d_blk,
                                               d_beta=d_beta) == ac.N_DSYM
    assert (d_beta.download(np.float32, len(ac.ALLOCS) * n * ac.N_DSYM) > 0).all(), "every frame should find its sync"
    res = {"combined": lost()}
    for b in range(B):
        assert rxe.demod_frames_despread_alloc(d_rx.data_ptr() + b * n * fl * 8, n, fl, fl, d_eq, d_llr=d_blk,
                                               noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=ac.NOISE_VAR) == ac.N_DSYM
        res["branch %d alone" % b] = lost()
    print("blocks lost of %d: %r (the oracle's receiver: %r)" % (n, res, ac.LOST_AT_LEVEL))
    assert res == ac.LOST_AT_LEVEL
