"""Planted de-mapper inputs: symbols whose coordinates sit ON the hard-decision edges of each modulation, one or two ulps
either side of them, and at the float32 extremes (shared by test_demap_rules.py and test_gpu_fused_demap_edges.py).

The edges are those of the float32 rules in oracle.demap_hard / csrc/demap_hard.hpp:hard_bits:
  BPSK    x > 0
  QPSK    (x < 0) xor (|x| > SQRT2_F32)              (plus the literal tie path for an exactly-zero coordinate)
  16-QAM  x < 0, |x| > float32(2/sqrt(10))
  64-QAM  x < 0, |x| > a, |(|x| - a)| > c            a = float32(4/sqrt(42)), c = float32(2/sqrt(42))
"""
import numpy as np

from oracle import ofdm_oracle as orc

MODS = {1: "BPSK", 2: "QPSK", 4: "16QAM", 6: "64QAM"}
F32 = np.float32
HUGE = (F32(1e19), F32(3e19), F32(1e20))          # |x*y*x'*y'| overflows float32 (FLT_MAX ~ 3.4e38) for two such symbols


def ulps(v, k):
    """float32 v moved by k ulps (k may be negative), crossing zero like nextafter does"""
    v = F32(v)
    to = F32(np.inf) if k > 0 else F32(-np.inf)
    for _ in range(abs(k)):
        v = np.nextafter(v, to, dtype=np.float32)
    return v


def qam64_c_edges():
    """The edges of 64-QAM's third axis bit, |(|x| - a)| > c, as float32 arithmetic sees them: next to a + c and next to a - c,
    the positive x where the bit is still 0 and one ulp further it is 1.  Where |(|x| - a)| == c holds exactly that is the x
    (next to a - c); next to a + c, x - a is exact (Sterbenz) on a grid twice as coarse as c's and equality never holds."""
    a, c = F32(4.0 / np.sqrt(42.0)), F32(2.0 / np.sqrt(42.0))
    out = []
    for centre, out_dir in ((a + c, 1), (a - c, -1)):
        xs = [ulps(centre, k) for k in range(-8, 9)]
        edge = [x for x in xs if not np.abs(np.abs(x) - a) > c and np.abs(np.abs(ulps(x, out_dir)) - a) > c]
        assert len(edge) == 1, "no single 64-QAM c edge next to %r" % centre
        out.append(edge[0])
    return out


def thresholds(bits):
    """positive float32 decision edges of the modulation (the sign edge 0 is added by the caller)"""
    if bits == 1:
        return []
    if bits == 2:
        return [orc.SQRT2_F32]
    if bits == 4:
        return [F32(2.0 / np.sqrt(10.0))]
    return [F32(4.0 / np.sqrt(42.0))] + qam64_c_edges()


def levels(bits):
    if bits == 1:
        return [F32(1.0)]
    if bits == 2:
        return [F32(np.sqrt(0.5))]
    return [F32(v) for v in orc.qam_levels(MODS[bits])[0] if v > 0]


def coordinate_values(bits):
    """float32 coordinate values of the corpus of one modulation"""
    v = [F32(0.0), F32(-0.0)]
    for t in thresholds(bits):
        for k in (-2, -1, 0, 1, 2):
            v += [ulps(t, k), -ulps(t, k)]
    for lv in levels(bits):
        v += [lv, -lv]
    tiny = np.finfo(np.float32).smallest_subnormal
    fmin, fmax = np.finfo(np.float32).tiny, np.finfo(np.float32).max
    for x in (tiny, F32(1e-40), ulps(F32(1e-40), 1), fmin, fmax) + HUGE:
        v += [F32(x), -F32(x)]
    v += [F32(np.inf), F32(-np.inf), F32(np.nan)]
    return np.array(v, np.float32)


def adversarial_groups():
    """every placement of {huge, 0+0j, (0, y), (x, 0), NaN, a plain point, a tiny point} over the 4 symbols of a group: the
    QPSK tie pre-check of pack4 (4 symbols) and pack2 (2 symbols) multiplies all coordinates of its group, so an overflow or a
    NaN next to an exact zero must not hide the zero."""
    el = np.array([complex(1e20, 1e20), 0j, complex(0.0, 0.6), complex(-0.6, 0.0), complex(np.nan, 0.3),
                   complex(0.5, -0.9), complex(1e-30, -1e-30)], np.complex64)
    idx = np.stack(np.meshgrid(*[np.arange(len(el))] * 4, indexing="ij"), axis=-1).reshape(-1)
    return el[idx]


def corpus(bits, seed=0, shuffles=3):
    """complex64 symbols, length divisible by 4: all ordered pairs of coordinate_values, the adversarial groups, then
    `shuffles` seeded permutations of both (so that every value also meets other neighbours in a group)."""
    v = coordinate_values(bits)
    x, y = np.meshgrid(v, v, indexing="ij")
    pairs = np.empty(x.size, np.complex64)
    pairs.real, pairs.imag = x.ravel(), y.ravel()
    base = np.concatenate([pairs, adversarial_groups()])
    rng = np.random.default_rng(seed)
    z = np.concatenate([base] + [base[rng.permutation(base.size)] for _ in range(shuffles)])
    pad = (-z.size) % 4
    return np.concatenate([z, np.full(pad, 0.5 - 0.25j, np.complex64)])


def finite(z):
    z = np.asarray(z, np.complex64)
    return np.isfinite(z.real) & np.isfinite(z.imag)


def expected_bits(z, bits):
    """orc.demap_hard per symbol for the finite symbols, shape [n, bits]; rows of non-finite symbols are left at 255 (the
    reference defines no bits for them: the tests hold those to the device's own hard_bits rule instead)."""
    z = np.asarray(z, np.complex64)
    out = np.full((z.size, bits), 255, np.uint8)
    f = finite(z)
    out[f] = orc.demap_hard(z[f], MODS[bits]).reshape(-1, bits)
    return out
