"""Pins tests/csi_ref.py (the float32 restatement of the channel-state-weighted LLR contract, include/ofdm_mi355x.h) by means
that do not depend on it: an fp64 evaluation of the same formulas, the textbook QPSK form, the hard-decision regions of
orc.demap_hard, every erasure rule -- and asserts the benefit the stage exists for, on the reference alone: on a two-path channel
seen through the oracle's receiver (estimated H), the channel-weighted LLRs decode every block where the per-frame-sigma LLRs of
ofdm_demap_frames lose at least 8 of 64."""
import math

import numpy as np
import pytest

import channel_ref
import csi_cases as cc
import csi_ref
import turbo_ref
from oracle import ofdm_oracle as orc

TOL = 1e-5                                   # the bar of test_gpu_soft_frames.py: of the largest |llr|
MODS = ("QPSK", "16QAM", "64QAM")


def _syms(rng, n, scale):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("given", [False, True])
def test_float32_reference_against_fp64(mod, given):
    rng = np.random.default_rng(csi_ref.BPS[mod] + 10 * given)
    rows, row_len = 7, 57
    z = _syms(rng, rows * row_len, 0.9).reshape(rows, row_len)
    a = rng.uniform(0.01, 2.0, row_len).astype(np.float32)
    nv = 0.07 if given else None
    l32, s32, n32, _ = csi_ref.demap_csi_segment(z, a, 0.03, mod, nv)
    l64, s64, n64, _ = csi_ref.demap_csi_segment(z, a, 0.03, mod, nv, dtype=np.float64)
    assert l32.dtype == np.float32 and n32 == n64 == rows * row_len
    assert abs(s32 - s64) <= 1e-6 * s64
    if not given:                            # the same sigma2 on both sides: this check is about the LLR arithmetic
        l64 = csi_ref.llr_with_sigma2(z, a, 0.03, mod, float(np.float32(s32)), dtype=np.float64)
    assert np.max(np.abs(l32.astype(np.float64) - l64)) <= TOL * np.max(np.abs(l64))


def test_qpsk_textbook_form():
    """a = 1, rho = 0: llr = 2 sqrt(2) Re/Im(z) / sigma^2"""
    rng = np.random.default_rng(1)
    z = _syms(rng, 600, 1.0).reshape(10, 60)
    sigma2 = 0.2
    llr, s, n, _ = csi_ref.demap_csi_segment(z, np.ones(60, np.float32), 0.0, "QPSK", sigma2)
    want = np.stack([z.real.ravel(), z.imag.ravel()], axis=1).ravel().astype(np.float64) * (2.0 * math.sqrt(2.0) / sigma2)
    assert s == sigma2 and n == 600
    assert np.max(np.abs(llr - want)) <= TOL * np.max(np.abs(want))


@pytest.mark.parametrize("mod", MODS)
def test_sign_rule_equals_the_hard_decision_regions(mod):
    """bit = (llr < 0) of the unbiased symbol u = z*s lies in orc.demap_hard's regions (QPSK: the sign rule; the reference's
    outlier flip beyond sqrt(2) is BitRecovery's own and not part of a max-log LLR)"""
    rng = np.random.default_rng(2)
    n = 4000
    z = _syms(rng, n, 1.0)
    a = rng.uniform(0.05, 2.0, z.size).astype(np.float32)
    rho = np.float32(0.1)
    s = ((a + rho) / a).astype(np.float32)
    u = (z.real.astype(np.float32) * s + 1j * (z.imag.astype(np.float32) * s)).astype(np.complex64)
    if mod == "QPSK":
        keep = (np.abs(u.real) < 1.4) & (np.abs(u.imag) < 1.4) & (u.real != 0) & (u.imag != 0)
        z, a, u = z[keep], a[keep], u[keep]
        assert keep.sum() > n // 2
    usable, d, _, _ = csi_ref.symbols(z, a, rho, mod)
    assert usable.all()
    hard = orc.demap_hard(u, mod).reshape(z.size, -1)
    clear = np.abs(d) > 1e-5                 # a symbol on a decision edge may round either way
    assert clear.mean() > 0.99
    assert np.array_equal((d < 0)[clear], hard.astype(bool)[clear])


def test_bit_order_and_labels_against_the_mapper():
    """a noiseless symbol of every constellation point de-maps to the bits that made it"""
    for mod in MODS:
        bps = csi_ref.BPS[mod]
        bits = ((np.arange(1 << bps)[:, None] >> np.arange(bps - 1, -1, -1)[None, :]) & 1).astype(np.uint8)
        z = orc.map_bits(bits.ravel(), mod).astype(np.complex64).reshape(1, -1)
        g = np.float32(0.5)                  # the equaliser's shrink a/(a + rho) with a = rho
        llr, _, n, _ = csi_ref.demap_csi_segment(z * g, np.full(z.size, 0.25, np.float32), 0.25, mod, 0.1)
        assert n == z.size and np.array_equal((llr < 0).astype(np.uint8), bits.ravel()), mod


@pytest.mark.parametrize("mod", MODS)
def test_erasure_rules(mod):
    bps = csi_ref.BPS[mod]
    z0 = np.complex64(0.4 - 0.3j)
    big = np.float32(3e38)
    cases = [  # (z, a, rho, usable)
        (z0, 1.0, 0.03, True), (z0, 0.0, 0.03, False), (z0, -1.0, 0.03, False), (z0, np.nan, 0.03, False), (z0, np.inf, 0.03, False),
        (z0, 1e-42, 0.03, False),            # denormal a: s = (a + rho)/a overflows
        (z0, 1e-42, 0.0, True),              # ... but is 1 without the regulariser: usable, the weight a/sigma2 is tiny
        (np.complex64(0), 1.0, 0.03, False), (np.complex64(complex(np.nan, 0.1)), 1.0, 0.03, False),
        (np.complex64(complex(0.1, np.inf)), 1.0, 0.03, False), (np.complex64(complex(big, 0.1)), 1.0, 0.5, False),  # u overflows
        # u finite, (u.re - l)^2 overflows: usable, the LLRs of the real axis +0, e not finite and so not in the sum
        (np.complex64(complex(big, 0.1)), 1.0, 0.0, True),
        (np.complex64(0.0 + 0.2j), 1.0, 0.03, True),
    ]
    for z, a, rho, want in cases:
        zz = np.array([[z, z0]], np.complex64)
        llr, s2, n_given, _ = csi_ref.demap_csi_segment(zz, np.array([a, 1.0], np.float32), rho, mod, 0.05)
        assert np.isfinite(llr).all() and n_given == 1 + want, (z, a, rho)
        dead = llr[:bps] if not want else llr[0:bps:2] if abs(z) > 1e30 else llr[:0]
        assert not dead.any() and not np.signbit(dead).any(), (z, a, rho)
        assert llr[bps:].any()
        llr_e, s2_e, n_est, terms = csi_ref.demap_csi_segment(zz, np.array([a, 1.0], np.float32), rho, mod)
        assert np.isfinite(llr_e).all() and math.isfinite(s2_e) and n_est == 1 + (want and abs(z) < 1e30), (z, a, rho)
    # sigma2 = 0: a segment that sits on its constellation points, and a segment without a usable symbol
    lv = csi_ref.levels(bps)[0]
    pts = (np.full((1, 4), complex(lv[0], lv[0]))).astype(np.complex64)
    llr, s2, n, _ = csi_ref.demap_csi_segment(pts, np.ones(4, np.float32), 0.0, mod)
    assert s2 == 0.0 and n == 4 and not llr.any() and not np.signbit(llr).any()
    llr, s2, n, _ = csi_ref.demap_csi_segment(pts, np.zeros(4, np.float32), 0.0, mod)
    assert s2 == 0.0 and n == 0 and not llr.any() and not np.signbit(llr).any()
    # a given sigma2 that float32 cannot hold: every LLR +0
    for nv in (1e300, 1e-300):
        llr, s2, n, _ = csi_ref.demap_csi_segment(np.array([[z0]]), np.ones(1, np.float32), 0.03, mod, nv)
        assert s2 == nv and n == 1 and not llr.any() and not np.signbit(llr).any()


# ------------------------------------------------------------------------------------------ the benefit, on the reference alone
def received_frames(noise_var):
    """the case's frames through the oracle's receiver -> (z [frames][9][60] complex64, a [frames][60] float32, info bits)"""
    L = cc.N + cc.CP
    info = cc.info_bits()
    coded = turbo_ref.encode_segments(info, cc.F1, cc.F2, cc.SEG_BITS)
    rows = [r for r in range(cc.N_SYM) if r % 4 != 3]
    bins = orc.bins_p(cc.KD, cc.N)
    noise = channel_ref.noise(cc.SEED_NOISE, cc.N_FRAMES, cc.FRAME_LEN, noise_var)
    z = np.zeros((cc.N_FRAMES, cc.N_DSYM, cc.KD), np.complex64)
    a = np.zeros((cc.N_FRAMES, cc.KD), np.float32)
    for f in range(cc.N_FRAMES):
        tx = orc.tx_modulate(coded[f], cc.N, cc.CP, cc.KS, cc.KD, cc.N_SYM, modulation=cc.MOD)
        y = np.convolve(tx, cc.TAPS)[:cc.FRAME_LEN - cc.LEAD]
        x = np.zeros(cc.FRAME_LEN, complex)
        x[cc.LEAD:cc.LEAD + len(y)] = y
        x += noise[f]
        o = orc.RxOracle(cc.N_SYM, cc.N, cc.CP, cc.KS, [1, 3], cc.KD, cc.SNR_ARG, cc.GATE, force_fp64=True)
        o.work(x.astype(np.complex64), np.zeros(cc.FRAME_LEN, np.complex64))
        z[f] = o.est_data_freq[rows]
        a[f] = csi_ref.csi_row(o.est_chan_freq_P[0].astype(np.complex64), bins)
    assert L * cc.N_SYM + cc.LEAD + len(cc.TAPS) - 1 <= cc.FRAME_LEN
    return z, a, info


def wrong_blocks(llr, info):
    bits, _ = turbo_ref.decode_segments(llr, 1, cc.K, cc.F1, cc.F2, cc.N_ITER)
    return int((bits != info).any(axis=(1, 2)).sum())


def test_benefit_on_the_reference():
    h2 = np.abs(np.fft.fft(cc.TAPS, cc.N)) ** 2
    assert h2.min() < 0.02 and h2.max() > 1.9                      # the band runs through a deep fade
    rho = np.float32(1.0 / 10.0 ** (cc.SNR_ARG / 20.0))
    lost = {}
    for name, nv in (("level", cc.NOISE_VAR), ("1 dB up", cc.NOISE_VAR_1DB)):
        z, a, info = received_frames(nv)
        csi = np.stack([csi_ref.demap_csi_segment(z[f], a[f], rho, cc.MOD)[0] for f in range(cc.N_FRAMES)])
        lost[name] = wrong_blocks(csi, info)
        if name == "level":
            old = np.zeros_like(csi)
            for f in range(cc.N_FRAMES):
                _, s0, s1 = orc.soft_demap_qam(z[f].ravel(), cc.MOD)
                old[f] = (s0 - s1).astype(np.float32)
            lost["per-frame sigma"] = wrong_blocks(old, info)
    print("wrong blocks of %d: %r" % (cc.N_FRAMES, lost))
    assert lost["level"] == 0 and lost["1 dB up"] == 0
    assert lost["per-frame sigma"] >= 8
