"""Pins tests/mrc_ref.py (the float32 restatement of the receive-diversity combining contract, include/ofdm_mi355x.h) by means
that do not depend on it: an fp64 evaluation of the same formulas, the single-branch case against csi_ref, the weighting rules,
every erasure rule of steps 1-4 -- and asserts the benefit the stage exists for, on the reference alone: two branches seen through
the oracle's receiver (estimated H) decode every block at a noise level where either branch alone loses at least 8 of 64."""
import numpy as np
import pytest

import channel_ref
import csi_ref
import mrc_cases as mc
import mrc_ref
import turbo_ref
from oracle import ofdm_oracle as orc
from test_csi_ref_host import wrong_blocks

MODS = ("QPSK", "16QAM", "64QAM")
EPS = 2.0 ** -24
L_MAX = 7 * 0.15430334996209191 + 1e-6       # the largest level of any of the three alphabets

# The bound of the float32 run against the fp64 run of the same formulas, to first order in eps = 2^-24 (one rounding).  The
# branches' terms may cancel in N, so the error of u is relative to X = sum |p_b| / A per axis, not to |u| (X >= |u|; X = |u| where
# the branches agree in sign, as they do on a link):
#   c = (a + rho)/w_den: 2 roundings; p = z*c: 1; N: B-1 additions; t: 1 and A: B-1 additions; u = N/A: 1
#     -> |du| <= (2B + 4) eps X
#   e = fl(fl(u - l)^2): |de| <= 2|u - l||du| + 3 eps e <= (2(2B + 4) + 3) eps (X + L)^2
#   d = fl(e1 - e0), each a minimum of such e (a minimum moves by no more than its terms do): |dd| <= (2(4B + 11) + 1) eps (X + L)^2
#   llr = fl(A d), A carrying (B + 1) eps: |dllr| <= (8B + 23) eps A (X + L)^2 + (B + 2) eps A |d| <= (9B + 25) eps A (X + L)^2
# One more eps covers the second-order terms.  The levels are the library's float32 ones in both runs.
def k_mrc(B):
    return 9 * B + 26


def x_abs(z, a, rho, s2):
    """X per symbol and axis in fp64 -> [n][2], and A [n]"""
    B, rows, row_len = z.shape
    ct = [mrc_ref.entries(a[b], rho, s2[b], np.float64) for b in range(B)]
    A = sum(np.tile(ct[b][1], rows) for b in range(B))
    xr = sum(np.abs(z[b].real.ravel().astype(np.float64)) * np.tile(ct[b][0], rows) for b in range(B)) / A
    xi = sum(np.abs(z[b].imag.ravel().astype(np.float64)) * np.tile(ct[b][0], rows) for b in range(B)) / A
    return np.stack([xr, xi], axis=1), A


# csi_ref's float32 run by the same count: u = z*((a + rho)/a) carries 3 eps -> e (2*3 + 3), d (2*9 + 1), llr = (a/w_den)*d 2 more
K_CSI = 22


def _syms(rng, shape, scale=0.9):
    return (scale * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("B", [1, 2, 3, 8])
@pytest.mark.parametrize("mod", MODS)
def test_float32_reference_against_fp64(mod, B):
    rng = np.random.default_rng(csi_ref.BPS[mod] + 10 * B)
    rows, row_len = 7, 57
    z = _syms(rng, (B, rows, row_len))
    a = rng.uniform(0.01, 2.0, (B, row_len)).astype(np.float32)
    s2 = rng.uniform(0.03, 0.3, B)
    l32, u32, w32, took = mrc_ref.combine(z, a, 0.03, mod, s2)
    l64, u64, w64, _ = mrc_ref.combine(z, a, 0.03, mod, s2, dtype=np.float64)
    assert l32.dtype == np.float32 and u32.dtype == np.complex64 and w32.dtype == np.float32 and took.all()
    assert (w64 > 0).all()
    assert (np.abs(w32 - w64) <= (B + 1) * EPS * w64).all()
    x, A = x_abs(z, a, 0.03, s2)
    assert np.allclose(A, w64, rtol=1e-12)
    assert (np.abs(u32.real - u64.real) <= (2 * B + 4) * EPS * x[:, 0]).all()
    assert (np.abs(u32.imag - u64.imag) <= (2 * B + 4) * EPS * x[:, 1]).all()
    bps = csi_ref.BPS[mod]
    scale = (w64[:, None] * (x + L_MAX) ** 2)[:, np.arange(bps) % 2].ravel()         # bit k is on axis k % 2
    err = np.abs(l32.astype(np.float64) - l64)
    assert (err <= k_mrc(B) * EPS * scale).all(), float(np.max(err / scale) / EPS)


@pytest.mark.parametrize("mod", MODS)
def test_one_branch_is_the_channel_state_weighted_llr(mod):
    """B = 1 with the noise given: the LLRs of csi_ref.demap_csi_segment, each side within its own bound of the exact value"""
    rng = np.random.default_rng(3 + csi_ref.BPS[mod])
    rows, row_len = 5, 60
    z = _syms(rng, (1, rows, row_len))
    a = rng.uniform(0.01, 2.0, (1, row_len)).astype(np.float32)
    nv = 0.07
    l_m, u, w, _ = mrc_ref.combine(z, a, 0.03, mod, [nv])
    l_c, s2, n, _ = csi_ref.demap_csi_segment(z[0], a[0], 0.03, mod, nv)
    assert s2 == nv and n == rows * row_len
    bps = csi_ref.BPS[mod]
    x = np.stack([np.abs(u.real), np.abs(u.imag)], axis=1).astype(np.float64)
    scale = (w[:, None].astype(np.float64) * (x + L_MAX) ** 2)[:, np.arange(bps) % 2].ravel()
    assert (np.abs(l_m.astype(np.float64) - l_c) <= (k_mrc(1) + K_CSI) * EPS * scale).all()


def test_a_branch_with_twice_the_noise_weighs_half():
    rng = np.random.default_rng(5)
    z = _syms(rng, (2, 3, 8))
    a = np.ones((2, 8), np.float32)                                                  # powers of two: every operation is exact
    _, u, w, _ = mrc_ref.combine(z, a, 0.0, "16QAM", [0.25, 0.5])
    z0, z1 = z[0].ravel().astype(np.complex128), z[1].ravel().astype(np.complex128)
    want = (4.0 * z0 + 2.0 * z1) / 6.0                                               # weights 1/0.25 and 1/0.5
    assert (w == np.float32(6.0)).all()
    assert np.max(np.abs(u - want)) <= 4 * EPS * np.max(np.abs(want))
    _, _, w1, _ = mrc_ref.combine(z[1:], a[1:], 0.0, "16QAM", [0.5])
    _, _, w0, _ = mrc_ref.combine(z[:1], a[:1], 0.0, "16QAM", [0.25])
    assert (w0 == 2 * w1).all()


@pytest.mark.parametrize("mod", MODS)
def test_two_equal_branches_give_u_of_either_and_twice_the_weight(mod):
    rng = np.random.default_rng(6)
    z1 = _syms(rng, (1, 4, 9))
    a1 = rng.uniform(0.05, 2.0, (1, 9)).astype(np.float32)
    l1, u1, w1, _ = mrc_ref.combine(z1, a1, 0.03, mod, [0.1])
    l2, u2, w2, _ = mrc_ref.combine(np.concatenate([z1, z1]), np.concatenate([a1, a1]), 0.03, mod, [0.1, 0.1])
    assert same_bits(u2, u1)                                                         # p + p and t + t are exact doublings
    assert same_bits(w2, (2 * w1).astype(np.float32))
    assert same_bits(l2, (2 * l1).astype(np.float32))


def _zero(v):
    return not np.asarray(v).view(np.uint32 if np.asarray(v).dtype == np.float32 else np.uint64).any()


@pytest.mark.parametrize("mod", MODS)
def test_erasure_rules(mod):
    """each rule of steps 1-4 takes one branch out of one symbol: the result is that of the other branches bit for bit"""
    bps = csi_ref.BPS[mod]
    rng = np.random.default_rng(7 + bps)
    B, rows, row_len = 3, 2, 6
    z = _syms(rng, (B, rows, row_len))
    a = rng.uniform(0.05, 2.0, (B, row_len)).astype(np.float32)
    s2 = [0.05, 0.08, 0.11]
    big = np.float32(3e38)
    nan, inf = np.nan, np.inf
    full = mrc_ref.combine(z, a, 0.03, mod, s2)
    assert full[3].all()
    # (what is damaged in branch 1, the symbols it drops out of)
    col = lambda j: [r * row_len + j for r in range(rows)]                           # noqa: E731
    cases = [("a", 2, 0.0, col(2)), ("a", 2, -1.0, col(2)), ("a", 2, nan, col(2)), ("a", 2, inf, col(2)),
             ("z", 4, 0j, [4]), ("z", 4, complex(nan, 0.1), [4]), ("z", 4, complex(0.1, inf), [4]), ("z", 4, complex(big, 0.1), [4]),  # p overflows
             ("s2", None, 0.0, range(rows * row_len)), ("s2", None, nan, range(rows * row_len)), ("s2", None, inf, range(rows * row_len)),
             ("s2", None, -0.1, range(rows * row_len)), ("s2", None, 1e300, range(rows * row_len)), ("s2", None, 1e-300, range(rows * row_len)),
             ("s2", None, 1e-44, range(rows * row_len))]                             # w_den a denormal: c overflows
    for what, at, val, out_of in cases:
        zz, aa, ss = z.copy(), a.copy(), list(s2)
        if what == "a":
            aa[1, at] = val
        elif what == "z":
            zz[1].reshape(-1)[at] = val
        else:
            ss[1] = val
        llr, sym, w, took = mrc_ref.combine(zz, aa, 0.03, mod, ss)
        assert np.isfinite(llr).all() and np.isfinite(sym.view(np.float32)).all() and np.isfinite(w).all(), (what, val)
        out_of = np.array(list(out_of))
        want_took = np.ones((B, rows * row_len), bool)
        want_took[1, out_of] = False
        assert np.array_equal(took, want_took), (what, val)
        others = mrc_ref.combine(zz[[0, 2]], aa[[0, 2]], 0.03, mod, [ss[0], ss[2]])   # branches 0 and 2 alone
        keep = np.ones(rows * row_len, bool)
        keep[out_of] = False
        for got, ref, alone, per in ((llr, full[0], others[0], bps), (sym, full[1], others[1], 1), (w, full[2], others[2], 1)):
            got, ref, alone = got.reshape(-1, per), ref.reshape(-1, per), alone.reshape(-1, per)
            assert same_bits(got[out_of], alone[out_of]), (what, val)
            assert same_bits(got[keep], ref[keep]), (what, val)
    # step 1, t > 0: c = 0.03/3e38 is finite and not 0, t = 1e-10/3e38 underflows to 0
    c, t, ok = mrc_ref.entries(np.array([1e-10, 1.0], np.float32), 0.03, 3e38)
    assert c[0] > 0 and t[0] == 0 and list(ok) == [False, True]
    # every branch out of symbol 4: +0 in all three outputs
    zz = z.copy()
    zz[:, 0, 4] = [0j, complex(nan, 1), complex(1, inf)]
    llr, sym, w, took = mrc_ref.combine(zz, a, 0.03, mod, s2)
    assert not took[:, 4].any() and _zero(llr[4 * bps:5 * bps]) and _zero(sym[4:5]) and _zero(w[4:5])
    assert llr[5 * bps:6 * bps].any() and w[5] > 0
    # no branch has a usable variance
    llr, sym, w, took = mrc_ref.combine(z, a, 0.03, mod, [0.0, 1e300, 1e-300])
    assert not took.any() and _zero(llr) and _zero(sym) and _zero(w)
    # step 4: the sums are finite, the quotient is not -> the symbol is not usable although branches took part
    z1 = np.full((2, 1, 1), complex(4e19, 4e19), np.complex64)
    a1 = np.full((2, 1), 1e-19, np.float32)
    llr, sym, w, took = mrc_ref.combine(z1, a1, 1.0, mod, [1.0, 1.0])                # N = 8e19, A = 2e-19: u overflows
    assert took.all() and _zero(llr) and _zero(sym) and _zero(w)
    # step 6: u finite, (u - l)^2 overflows -> the LLRs of that axis +0, the symbol and the weight stay
    z1 = np.full((1, 1, 1), complex(3e30, 0.1), np.complex64)
    llr, sym, w, took = mrc_ref.combine(z1, np.ones((1, 1), np.float32), 0.0, mod, [1.0])
    assert took.all() and w[0] == 1.0 and sym[0] == z1[0, 0, 0] and _zero(llr[0::2]) and llr[1::2].any()


# ------------------------------------------------------------------------------------------ the benefit, on the reference alone
def received_frames(noise_var):
    """the case's frames through the oracle's receiver, branch by branch -> (z [B][frames][9][60] complex64, a [B][frames][60]
    float32, info bits)"""
    info = mc.info_bits()
    coded = turbo_ref.encode_segments(info, mc.F1, mc.F2, mc.SEG_BITS)
    rows = [r for r in range(mc.N_SYM) if r % 4 != 3]
    bins = orc.bins_p(mc.KD, mc.N)
    tx = [orc.tx_modulate(coded[f], mc.N, mc.CP, mc.KS, mc.KD, mc.N_SYM, modulation=mc.MOD) for f in range(mc.N_FRAMES)]
    z = np.zeros((mc.N_BRANCH, mc.N_FRAMES, mc.N_DSYM, mc.KD), np.complex64)
    a = np.zeros((mc.N_BRANCH, mc.N_FRAMES, mc.KD), np.float32)
    for b in range(mc.N_BRANCH):
        noise = channel_ref.noise(mc.SEED_NOISE + b, mc.N_FRAMES, mc.FRAME_LEN, noise_var)
        for f in range(mc.N_FRAMES):
            y = np.convolve(tx[f], mc.TAPS[b])[:mc.FRAME_LEN - mc.LEAD]
            x = np.zeros(mc.FRAME_LEN, complex)
            x[mc.LEAD:mc.LEAD + len(y)] = y
            x += noise[f]
            o = orc.RxOracle(mc.N_SYM, mc.N, mc.CP, mc.KS, [1, 3], mc.KD, mc.SNR_ARG, mc.GATE, force_fp64=True)
            o.work(x.astype(np.complex64), np.zeros(mc.FRAME_LEN, np.complex64))
            z[b, f] = o.est_data_freq[rows]
            a[b, f] = csi_ref.csi_row(o.est_chan_freq_P[0].astype(np.complex64), bins)
    return z, a, info


def test_benefit_on_the_reference():
    for t in mc.TAPS:
        h2 = np.abs(np.fft.fft(t, mc.N)) ** 2
        assert h2.min() < 0.02 and h2.max() > 1.9                                    # each branch runs through a deep fade
    rho = np.float32(1.0 / 10.0 ** (mc.SNR_ARG / 20.0))
    lost = {}
    for name, nv in (("level", mc.NOISE_VAR), ("1 dB up", mc.NOISE_VAR_1DB)):
        z, a, info = received_frames(nv)
        est = np.array([[csi_ref.demap_csi_segment(z[b, f], a[b, f], rho, mc.MOD)[1] for f in range(mc.N_FRAMES)]
                        for b in range(mc.N_BRANCH)])
        lost[name + ", estimated"] = wrong_blocks(mrc_ref.combine_segments(z, a, rho, mc.MOD, est)[0], info)
        lost[name + ", given"] = wrong_blocks(mrc_ref.combine_segments(z, a, rho, mc.MOD, [nv] * mc.N_BRANCH)[0], info)
        if name == "level":
            for b in range(mc.N_BRANCH):
                one = np.stack([csi_ref.demap_csi_segment(z[b, f], a[b, f], rho, mc.MOD)[0] for f in range(mc.N_FRAMES)])
                lost["branch %d alone" % b] = wrong_blocks(one, info)
    print("wrong blocks of %d: %r" % (mc.N_FRAMES, lost))
    for name in ("level", "1 dB up"):
        assert lost[name + ", estimated"] == 0 and lost[name + ", given"] == 0
    assert lost["branch 0 alone"] >= 8 and lost["branch 1 alone"] >= 8
