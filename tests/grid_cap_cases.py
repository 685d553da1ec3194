"""Shapes and seeded inputs of the grid-cap tests, shared by tests/test_grid_caps_host.py (no GPU) and tests/test_gpu_grid_caps.py.
Plain NumPy, no GPU.  Every function is deterministic.

Many launchers cap their grid and let the kernel loop with the grid as stride, and some host functions cut a batch into parts.
Every case here is the smallest shape at which some workgroup takes a second trip (or the host loop a second part), together with
the slices that stay below every cap: the GPU test asserts that the capped launch equals the sub-cap launches bit for bit, and
holds the sub-cap launches to the kernel's reference.  The constants below restate the sources; test_grid_caps_host.py parses
the sources and fails when one of them moves, so that a later change of a cap cannot turn these into one-trip tests unnoticed."""
import functools

import numpy as np

import csi_ref
from oracle import ofdm_oracle as orc

# ------------------------------------------------------------------------------------------ the caps, as the sources state them
CSI_GRID_CAP = 262144            # rx_csi.hip: workgroups of csi_noise / csi_llr / csi_finish / csi_table / csi_frames
MRC_GRID_CAP = 262144            # rx_mrc.hip: workgroups of mrc_llr / mrc_table
OFDM_DEMAP_CAP1 = 262144         # rx_demap.hip: workgroups of demap_seg_dmin
OFDM_DEMAP_CAP2 = 262144         # rx_demap.hip: workgroups of demap_seg_soft
SEG_SLICE = 2048                 # ofdm_launch.hpp: symbols of one (segment, slice) item
TX_GRID_CAP = 262144             # tx_kernels.hip: workgroups of tx_map / tx_grid / tx_random_bits
GRID_Y_CAP = 65535               # bitproc.hip, tb.hip: gridDim.y of gold_apply / tb_concat
FO_PART = 65535                  # capi_fo.hip: frames per trial-table launch, rows per despread launch
FO_MAX_SYNC = 100                # include/ofdm_mi355x.h: rows per frame of the CFO-search receiver
WG = 256                         # threads per workgroup of every table / element kernel above
RANDOM_BLOCK = 128               # bits one thread of tx_random_bits produces

MODS = ("QPSK", "16QAM", "64QAM")
BPS = csi_ref.BPS
RHO = 0.03
SLICE_SEGS = 100000              # segments per sub-cap launch
SLICE_ROWS = 30000               # gridDim.y rows per sub-cap launch
N_RANDOM = 1000                  # seeded random segments of a sample


def seg_slices(seg_len):
    return (seg_len + SEG_SLICE - 1) // SEG_SLICE


def parts(n, step):
    """[(first, count)] that cut n into pieces of at most `step`"""
    return [(s, min(step, n - s)) for s in range(0, n, step)]


def sample(n, cap, seed=0):
    """The segments link 2 checks where the reference loops per segment: the first two, the last two, the two on either side of
    every multiple of the cap and N_RANDOM seeded random ones; sorted, without repeats."""
    idx = {0, 1, n - 2, n - 1}
    for m in range(cap, n, cap):
        idx |= {m - 1, m}
    idx |= set(int(i) for i in np.random.default_rng(9000 + seed).choice(n, N_RANDOM, replace=False))
    return np.array(sorted(i for i in idx if 0 <= i < n), np.int64)


# ------------------------------------------------------------------------------------------ the shapes
# One slice per segment: items = segments.  2 * cap + 5 segments: every workgroup takes at least 2 trips, five take 3.
N_SEG = 2 * 262144 + 5
ROWS, ROW_LEN = 1, 3
SEG_STRIDE = 3                   # complex items = 24 bytes: consecutive segments alternate between the 16-byte and the per-float path
CSI_STRIDE = 4                   # one float of gap (NaN) behind every row of channel powers
MRC_B = 3                        # odd against MRC_ROUND = 2: the last round of the branch loop is half empty
TAB_ROW_LEN = 129                # table kernels: n_seg * row_len entries; 129 = one 64-QAM tile of 128 symbols and a remainder of 1
MRC_TAB_B = 2
CSI_FRAMES = dict(N=64, cp=16, Ks=62, Kd=62, n_sym=4, n_frames=(1 << 26) // 62 + 2, distinct=7)
TX_MAP_SYMS = (1 << 26) + 5
TX_GRID = dict(N=64, Kd=58, pilots=(-21, -7, 7, 21), rows=(1 << 20) + 1)
TX_RANDOM = dict(seed=(7 << 32) | 20260101, offset=77, n=(1 << 33) + 640)
GOLD = dict(n_seg=65535 + 37, seg_bits=40, llr_stride=43)
TB = dict(n_tb=65535 + 37, A=40, Z=40, G=530, cw_bits=535)
FO_DESPREAD = dict(case=4, fo_range=(-24000.0, 0.0, 24000.0), n_frames=700, distinct=7)
FO_LARGE = dict(case=0, fo_range=(-12000.0, 0.0, 12000.0), n_frames=65535 + 3, distinct=4, n_sym=8)

# name -> (what is counted, count of the capped launch, its cap, the largest count of a sub-cap launch)
CASES = {
    "csi items": ("segments x slices", N_SEG * seg_slices(ROWS * ROW_LEN), CSI_GRID_CAP, SLICE_SEGS * seg_slices(ROWS * ROW_LEN)),
    "csi segments": ("segments", N_SEG, CSI_GRID_CAP, SLICE_SEGS),
    "mrc items": ("segments x slices", N_SEG * seg_slices(ROWS * ROW_LEN), MRC_GRID_CAP, SLICE_SEGS * seg_slices(ROWS * ROW_LEN)),
    "demap pass 1": ("segments x slices", N_SEG * seg_slices(ROWS * ROW_LEN), OFDM_DEMAP_CAP1, SLICE_SEGS * seg_slices(ROWS * ROW_LEN)),
    "demap pass 2": ("segments x slices", N_SEG * seg_slices(ROWS * ROW_LEN), OFDM_DEMAP_CAP2, SLICE_SEGS * seg_slices(ROWS * ROW_LEN)),
    "demap sigma only": ("segments", N_SEG, OFDM_DEMAP_CAP2, SLICE_SEGS),
    "csi table": ("entries", N_SEG * TAB_ROW_LEN, CSI_GRID_CAP * WG, SLICE_SEGS * TAB_ROW_LEN),
    "csi table items": ("segments x slices", N_SEG * seg_slices(TAB_ROW_LEN), CSI_GRID_CAP, SLICE_SEGS * seg_slices(TAB_ROW_LEN)),
    "mrc table": ("entries", MRC_TAB_B * N_SEG * TAB_ROW_LEN, MRC_GRID_CAP * WG, MRC_TAB_B * SLICE_SEGS * TAB_ROW_LEN),
    "csi frames": ("outputs", CSI_FRAMES["n_frames"] * CSI_FRAMES["Kd"], CSI_GRID_CAP * WG, CSI_FRAMES["distinct"] * CSI_FRAMES["Kd"]),
    "tx map": ("symbols", TX_MAP_SYMS, TX_GRID_CAP * WG, 1 << 24),
    "tx grid": ("bins", TX_GRID["rows"] * TX_GRID["N"], TX_GRID_CAP * WG, (1 << 18) * TX_GRID["N"]),
    "tx random bits": ("128-bit blocks", (TX_RANDOM["offset"] + TX_RANDOM["n"] + 127) // 128, TX_GRID_CAP * WG, 4096 // 128 + 2),
    "gold": ("segments", GOLD["n_seg"], GRID_Y_CAP, SLICE_ROWS),
    "tb concat": ("transport blocks", TB["n_tb"], GRID_Y_CAP, SLICE_ROWS),
    "fo despread": ("rows", FO_DESPREAD["n_frames"] * FO_MAX_SYNC, FO_PART, FO_DESPREAD["distinct"] * FO_MAX_SYNC),
    "fo trial table": ("frames", FO_LARGE["n_frames"], FO_PART, FO_LARGE["distinct"]),
}


# ------------------------------------------------------------------------------------------ sampled segments, made on the CPU
# The bulk of a batch is drawn on the device; the sampled segments are made here, so that the references run on them on the CPU
# too (test_grid_caps_host.py) and the erasures sit where a trip that reads the wrong segment would show: next to the cap.
def _at(idx, seg):
    """position of segment `seg` in the sample"""
    p = int(np.searchsorted(idx, seg))
    assert idx[p] == seg
    return p


def points(rng, n, mod):
    return orc.map_bits(rng.integers(0, 2, n * BPS[mod]), mod)


@functools.lru_cache(maxsize=None)
def csi_sample(mod):
    """-> idx [k], sym [k][3] complex64, csi [k][CSI_STRIDE] float32 (NaN in the gap): constellation points through a one-tap MMSE
    equaliser as tests/test_gpu_csi.py draws them (segment s with noise variance (0.002, 0.005, 0.01)[s % 3]), with erasures
    planted on either side of the cap multiples: segment cap has no channel estimate (n_used = 0), segment cap - 1 is a
    guard-failed row of zeros (n_used = 0 too), 2 cap - 1 and 2 cap carry non-finite powers and symbols.  Read-only."""
    idx = sample(N_SEG, CSI_GRID_CAP)
    k = idx.size
    rng = np.random.default_rng(9100 + BPS[mod])
    a = rng.uniform(0.02, 2.0, (k, ROW_LEN))
    x = points(rng, k * ROW_LEN, mod).reshape(k, ROW_LEN)
    nv = np.array((0.002, 0.005, 0.01))[idx % 3][:, None]
    w = (rng.standard_normal((k, ROW_LEN)) + 1j * rng.standard_normal((k, ROW_LEN))) * np.sqrt(nv / 2)
    sym = ((a / (a + RHO)) * (x + w / np.sqrt(a))).astype(np.complex64)
    csi = np.full((k, CSI_STRIDE), np.nan, np.float32)
    csi[:, :ROW_LEN] = a
    cap = CSI_GRID_CAP
    csi[_at(idx, cap), :ROW_LEN] = 0                                                     # a frame without a sync
    sym[_at(idx, cap - 1)] = 0                                                           # a guard-failed row
    csi[_at(idx, 2 * cap), :ROW_LEN] = (np.nan, np.inf, -1.0)
    sym[_at(idx, 2 * cap - 1)] = (complex(np.nan, 0.1), complex(0.1, np.inf), complex(3e38, 0.1))
    csi[_at(idx, 2 * cap - 1), 2] = 0.1                                                  # s = 1.3: 3e38 * 1.3 overflows
    csi[_at(idx, 1), 1] = 1e-42                                                          # (a + rho) / a overflows
    for v in (idx, sym, csi):
        v.setflags(write=False)
    return idx, sym, csi


MRC_NOISE = (0.004, 0.01, 0.006)                                                         # variance of branch b


@functools.lru_cache(maxsize=None)
def mrc_sample(mod):
    """-> idx [k], z [B][k][3] complex64, a [B][k][3] float32, s2 [B][k] float64 (the variance of every unit), drawn as
    tests/test_gpu_mrc.py draws its branches.  Planted: branch 1 of segment cap found no sync, every branch is out of symbol 1 of
    segment cap - 1, the unit (2, 2 cap) has sigma2 = 0, branch 0 of segment 2 cap - 1 carries non-finite symbols.  Read-only."""
    idx = sample(N_SEG, MRC_GRID_CAP)
    k, B = idx.size, MRC_B
    rng = np.random.default_rng(9200 + BPS[mod])
    a = rng.uniform(0.02, 2.0, (B, k, ROW_LEN))
    x = points(rng, k * ROW_LEN, mod).reshape(k, ROW_LEN)
    w = rng.standard_normal((B, k, ROW_LEN)) + 1j * rng.standard_normal((B, k, ROW_LEN))
    w *= np.sqrt(np.array(MRC_NOISE) / 2)[:, None, None]
    z = ((a / (a + RHO)) * (x[None] + w / np.sqrt(a))).astype(np.complex64)
    a = a.astype(np.float32)
    s2 = np.array(MRC_NOISE)[:, None] * rng.uniform(0.8, 1.25, (B, k))
    cap = MRC_GRID_CAP
    z[1, _at(idx, cap)] = 0
    a[1, _at(idx, cap)] = 0
    z[:, _at(idx, cap - 1), 1] = (0j, complex(np.nan, np.nan), complex(np.inf, 0))
    s2[2, _at(idx, 2 * cap)] = 0.0
    z[0, _at(idx, 2 * cap - 1)] = (complex(np.nan, 0.1), complex(0.1, np.inf), complex(3e38, 0.1))
    a[2, _at(idx, 1), 1] = np.inf
    for v in (idx, z, a, s2):
        v.setflags(write=False)
    return idx, z, a, s2


DEMAP_R = (0.03, 0.08)           # distance of a symbol from its constellation point


@functools.lru_cache(maxsize=None)
def demap_sample(mod):
    """-> idx [k], z [k][3] complex64: constellation points moved by DEMAP_R[0] .. DEMAP_R[1] in a random direction.  A segment
    of three symbols has no average to lean on: its sigma is 0.7071 times the mean of three distances, and the fp64 oracle's
    64-QAM levels differ from the library's float32 ones by up to 6e-8 (tests/test_gpu_soft_frames.py, sigma_ref).  With every
    distance at least 0.03 that moves sigma by at most 2e-6 of itself and a metric (1 / sigma^2) by 4e-6, inside the 1e-5 of the
    existing comparison; 0.08 is about half of the 64-QAM half spacing (0.154), so the nearest point stays the one drawn.
    Read-only."""
    idx = sample(N_SEG, OFDM_DEMAP_CAP1)
    k = idx.size
    rng = np.random.default_rng(9300 + BPS[mod])
    x = points(rng, k * ROW_LEN, mod).reshape(k, ROW_LEN)
    r = rng.uniform(DEMAP_R[0], DEMAP_R[1], (k, ROW_LEN))
    z = (x + r * np.exp(2j * np.pi * rng.uniform(0, 1, (k, ROW_LEN)))).astype(np.complex64)
    for v in (idx, z):
        v.setflags(write=False)
    return idx, z


def windows(n, edges, width=4096, n_random=64, seed=0):
    """[(first, count)] windows of a flat output of n elements: the head, the tail, one that straddles every edge, and seeded
    random ones of odd lengths"""
    out = [(0, width), (n - width, width)]
    out += [(e - width // 2 + 1, width) for e in edges]
    rng = np.random.default_rng(9400 + seed)
    for _ in range(n_random):
        c = int(rng.integers(1, 1200))
        out.append((int(rng.integers(0, n - c)), c))
    return [(f, c) for f, c in out if f >= 0 and f + c <= n]
