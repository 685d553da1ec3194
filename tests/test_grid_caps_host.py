"""The grid-cap cases on the CPU: the caps tests/grid_cap_cases.py restates are the ones the sources hold, every case exceeds its
cap while its sub-cap launches do not, the sample rule picks the segments next to every cap multiple, and the references run
on the sampled segments at the operating point the GPU test (tests/test_gpu_grid_caps.py) relies on."""
import os
import re

import numpy as np
import pytest

import csi_ref
import grid_cap_cases as gc
import mrc_ref
import tb_cases as tc
import tb_ref
from oracle import ofdm_oracle as orc
from test_gpu_soft_frames import oracle_soft, sigma_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-gnu-radio-code_amd", "csrc")


def source(name, root=CSRC):
    with open(os.path.join(root, name)) as f:
        return f.read()


def one(pattern, text):
    """the single match of `pattern` in `text`, as an int"""
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


# ------------------------------------------------------------------------------------------ the caps of the sources
def test_named_caps_equal_the_sources():
    assert one(r"constexpr int64_t CSI_GRID_CAP = (\d+);", source("rx_csi.hip")) == gc.CSI_GRID_CAP
    assert one(r"constexpr int64_t MRC_GRID_CAP = (\d+);", source("rx_mrc.hip")) == gc.MRC_GRID_CAP
    demap = source("rx_demap.hip")
    assert one(r"#define OFDM_DEMAP_CAP1 (\d+)", demap) == gc.OFDM_DEMAP_CAP1
    assert one(r"#define OFDM_DEMAP_CAP2 (\d+)", demap) == gc.OFDM_DEMAP_CAP2
    assert one(r"constexpr int SEG_SLICE = (\d+);", source("ofdm_launch.hpp")) == gc.SEG_SLICE
    assert one(r"#define OFDM_FO_MAX_SYNC (\d+)", source("ofdm_mi355x.h", os.path.join(ROOT, "include"))) == gc.FO_MAX_SYNC
    assert "OFDM_DEMAP_CAP" not in source("Makefile"), "the build overrides a cap the tests restate"


def test_the_launchers_use_the_named_caps():
    """the grid of every launch under test is min(count, cap) with the cap parsed above, on 256-thread workgroups"""
    csi, mrc, demap = source("rx_csi.hip"), source("rx_mrc.hip"), source("rx_demap.hip")
    for name in ("gi", "gs", "gt"):
        assert re.search(r"const unsigned %s = unsigned\(std::min<int64_t>\([^;]*, CSI_GRID_CAP\)\);" % name, csi), name
    assert re.search(r"const unsigned g = unsigned\(std::min<int64_t>\(\(n_frames \* n_out \+ 255\) / 256, CSI_GRID_CAP\)\);", csi)
    for name in ("gt", "gi"):
        assert re.search(r"const unsigned %s = unsigned\(std::min<int64_t>\([^;]*, MRC_GRID_CAP\)\);" % name, mrc), name
    assert "demap_seg_dmin_kernel<MOD>, dim3(unsigned(std::min<int64_t>(items, OFDM_DEMAP_CAP1))), dim3(256)" in demap
    assert "const unsigned g2 = unsigned(std::min<int64_t>(outs ? items : a.n_seg, OFDM_DEMAP_CAP2));" in demap
    for text, loops in ((csi, 2), (mrc, 1), (demap, 2)):                                # the item loops stride by the grid
        assert len(re.findall(r"for \(int64_t w = blockIdx\.x; w < n_items; w \+= gridDim\.x\)", text)) == loops


def test_literal_caps_equal_the_sources():
    tx = source("tx_kernels.hip")
    for kernel, count in (("tx_random_bits_kernel", "nblk"), ("tx_map_kernel", "n_sym"), ("tx_grid_kernel", "total")):
        cap = one(r"hipLaunchKernelGGL\(%s, dim3\(unsigned\(std::min<int64_t>\(\(%s \+ 255\) / 256, (\d+)\)\)\), dim3\(256\)" % (kernel, count), tx)
        assert cap == gc.TX_GRID_CAP, kernel
    assert one(r"for \(int j = 0; j < (\d+); \+\+j\) \{\s*const uint64_t k = \(c << 7\)", tx) == gc.RANDOM_BLOCK
    gold = one(r"const dim3 grid\(unsigned\(\(a\.seg_bits \+ GOLD_SPAN - 1\) / GOLD_SPAN\), unsigned\(std::min<int64_t>\(a\.n_seg, (\d+)\)\)\);",
               source("bitproc.hip"))
    tb = one(r"const dim3 grid\(unsigned\(\(row \+ 255\) / 256\), unsigned\(std::min<int64_t>\(a\.n_tb, (\d+)\)\)\);", source("tb.hip"))
    assert gold == tb == gc.GRID_Y_CAP
    fo = source("capi_fo.hip")
    assert one(r"for \(int64_t f0 = 0; f0 < n_frames && pv > 0; f0 \+= (\d+)\)", fo) == gc.FO_PART
    assert one(r"sa\.n_frames = int\(std::min<int64_t>\((\d+), n_frames - f0\)\);", fo) == gc.FO_PART
    assert one(r"for \(int64_t r0 = 0; r0 < units; r0 \+= (\d+)\)", fo) == gc.FO_PART
    assert one(r"const int rows = int\(std::min<int64_t>\((\d+), units - r0\)\);", fo) == gc.FO_PART
    assert one(r"if \(a\.n_frames > (\d+)\) return hipErrorInvalidValue;", source("rx_sync.hip")) == gc.FO_PART


# ------------------------------------------------------------------------------------------ every case loops, no slice does
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_case_exceeds_its_cap_and_its_slices_do_not(name):
    what, count, cap, sub = gc.CASES[name]
    assert count > cap, "%s: %d %s fit one trip of %d" % (name, count, what, cap)
    assert 0 < sub <= cap, "%s: a sub-cap launch of %d %s loops itself (cap %d)" % (name, sub, what, cap)


def test_the_slices_cover_their_batches():
    for n, step in ((gc.N_SEG, gc.SLICE_SEGS), (gc.GOLD["n_seg"], gc.SLICE_ROWS), (gc.TB["n_tb"], gc.SLICE_ROWS), (gc.TX_MAP_SYMS, 1 << 24),
                    (gc.TX_GRID["rows"], 1 << 18)):
        p = gc.parts(n, step)
        assert len(p) >= 2 and p[0][0] == 0 and sum(c for _, c in p) == n and all(c <= step for _, c in p)
        assert all(p[i][0] + p[i][1] == p[i + 1][0] for i in range(len(p) - 1))
    # a slice of segments starts on an even segment: with 24-byte segments it meets the alignments its segments meet in the batch
    assert gc.SLICE_SEGS % 2 == 0 and gc.SEG_STRIDE * 8 % 16 == 8
    assert gc.N_SEG == 2 * gc.CSI_GRID_CAP + 5 and gc.seg_slices(gc.ROWS * gc.ROW_LEN) == 1
    assert gc.MRC_B % 2 == 1 and gc.TAB_ROW_LEN > 128                                   # MRC_ROUND = 2; one 64-QAM tile and a tail
    assert one(r"constexpr int MRC_ROUND = (\d+);", source("rx_mrc.hip")) == 2
    assert one(r"constexpr int TILE = (\d+);", source("rx_mrc.hip")) == 128
    # the random-bit window that straddles the second trip: thread 0's second block is block cap * 256
    r = gc.TX_RANDOM
    edge = gc.TX_GRID_CAP * gc.WG * gc.RANDOM_BLOCK - r["offset"]
    assert 0 < edge < r["n"] and any(f < edge < f + c for f, c in gc.windows(r["n"], [edge]))
    # FO: part two of the trial table and of the despread rows holds live frames
    assert gc.FO_LARGE["n_frames"] - gc.FO_PART == 3 and gc.FO_PART % gc.FO_LARGE["distinct"] != 0
    assert gc.FO_DESPREAD["n_frames"] * gc.FO_MAX_SYNC - gc.FO_PART > 40 * gc.FO_MAX_SYNC


@pytest.mark.parametrize("n,cap", [(gc.N_SEG, gc.CSI_GRID_CAP), (gc.GOLD["n_seg"], gc.GRID_Y_CAP), (3 * 1000 + 1, 1000), (2000, 1000)])
def test_the_sample_rule(n, cap):
    idx = gc.sample(n, cap)
    assert np.array_equal(idx, np.unique(idx)) and idx[0] == 0 and idx[-1] == n - 1
    want = {0, 1, n - 2, n - 1}
    for m in range(cap, n, cap):
        want |= {m - 1, m}
    assert len(want) >= 6 and want <= set(idx.tolist())
    assert gc.N_RANDOM <= idx.size <= gc.N_RANDOM + len(want)
    assert np.array_equal(idx, gc.sample(n, cap))                                        # seeded
    trips = set((idx // cap).tolist())
    assert trips == set(range((n + cap - 1) // cap)), "the random part misses a trip"


# ------------------------------------------------------------------------------------------ the operating point of the samples
@pytest.mark.parametrize("mod", gc.MODS)
def test_csi_sample_on_the_reference(mod):
    idx, sym, csi = gc.csi_sample(mod)
    cap = gc.CSI_GRID_CAP
    est = [csi_ref.demap_csi_segment(sym[i][None], csi[i, :gc.ROW_LEN], gc.RHO, mod) for i in range(idx.size)]
    giv = [csi_ref.demap_csi_segment(sym[i][None], csi[i, :gc.ROW_LEN], gc.RHO, mod, 0.05) for i in range(idx.size)]
    used = np.array([r[2] for r in est])
    at = {int(s): i for i, s in enumerate(idx)}
    assert used[at[cap]] == 0 and used[at[cap - 1]] == 0 and est[at[cap]][1] == 0.0     # n_used = 0: sigma2 = 0, every LLR +0
    assert not est[at[cap]][0].view(np.uint32).any() and not giv[at[cap - 1]][0].view(np.uint32).any()
    assert used[at[2 * cap]] == 0 and used[at[2 * cap - 1]] == 0 and used[at[1]] == 2
    assert used[at[0]] == used[at[gc.N_SEG - 1]] == 3
    assert (used == 3).sum() >= idx.size - 5 and np.array_equal(used, [r[2] for r in giv])
    llr = np.stack([r[0] for r in est])
    assert np.isfinite(llr).all() and (llr != 0).mean() > 0.98
    s2 = np.array([r[1] for r in est])
    assert len(set(s2[used == 3])) == (used == 3).sum(), "segments with their own data get their own sigma2"
    # flat, as link 2 runs it for OFDM_CSI_NOISE_GIVEN: the same LLRs as segment by segment
    a = csi[:, :gc.ROW_LEN].ravel()
    usable, d, _, _ = csi_ref.symbols(sym.ravel(), a, gc.RHO, mod)
    flat = csi_ref.llr_from(usable, d, a, 0.05).ravel()
    assert np.array_equal(flat.view(np.uint32), np.concatenate([r[0] for r in giv]).view(np.uint32))
    assert np.array_equal(usable.reshape(-1, gc.ROW_LEN).sum(axis=1), used)


@pytest.mark.parametrize("mod", gc.MODS)
def test_mrc_sample_on_the_reference(mod):
    idx, z, a, s2 = gc.mrc_sample(mod)
    cap = gc.MRC_GRID_CAP
    llr, sym, weight = mrc_ref.combine_segments(z[:, :, None, :], a, gc.RHO, mod, s2)
    at = {int(s): i for i, s in enumerate(idx)}
    took = lambda s: mrc_ref.combine(z[:, at[s], None, :], a[:, at[s]], gc.RHO, mod, s2[:, at[s]])[3]      # noqa: E731
    assert not took(cap)[1].any() and took(cap)[0].all() and took(cap)[2].all()
    assert not took(cap - 1)[:, 1].any() and weight[at[cap - 1], 1] == 0 and not llr[at[cap - 1]].reshape(gc.ROW_LEN, -1)[1].any()
    assert not took(2 * cap)[2].any() and not took(2 * cap - 1)[0].any() and not took(1)[2, 1]
    assert np.isfinite(llr).all() and np.isfinite(weight).all() and (weight > 0).sum() == weight.size - 1
    assert (llr != 0).mean() > 0.98


@pytest.mark.parametrize("mod", gc.MODS)
def test_demap_sample_on_the_reference(mod):
    idx, z = gc.demap_sample(mod)
    sig = np.array([sigma_ref(z[i], mod) for i in range(idx.size)])
    assert (sig >= 0.7071 * gc.DEMAP_R[0] * (1 - 1e-5)).all() and (sig <= 0.7071 * gc.DEMAP_R[1] * (1 + 1e-5)).all()
    assert len(set(sig)) == idx.size
    for i in (0, 1, idx.size // 2, idx.size - 1):
        s0, s1 = oracle_soft(z[i], mod)
        assert np.isfinite(s0).all() and np.isfinite(s1).all() and s0.size == gc.ROW_LEN * gc.BPS[mod]
    # every symbol is nearer to the point it was drawn from than DEMAP_R[1]: re-mapping its hard bits gives that point
    near = orc.map_bits(orc.demap_hard(z.ravel(), mod), mod)
    assert np.max(np.abs(z.ravel() - near)) <= gc.DEMAP_R[1] * (1 + 1e-5) and np.min(np.abs(z.ravel() - near)) >= gc.DEMAP_R[0] * (1 - 1e-5)


def test_tb_case_on_the_reference():
    t = gc.TB
    g = tb_ref.geometry(t["A"], t["Z"], t["G"])
    assert g is not None and g["C"] == 4 and len(g["groups"]) == 2 and t["cw_bits"] > t["G"]
    qm, qp = tc.pairs(t["A"], t["Z"])
    cw = tb_ref.encode(tc.payloads(t["A"], 5), t["G"], qm, qp, Z=t["Z"], cw_bits=t["cw_bits"])
    assert cw.shape == (5, t["cw_bits"]) and not cw[:, t["G"]:].any() and len(set(map(bytes, cw))) == 5
