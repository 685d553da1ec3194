"""tests/channel_ref.py without a GPU: the noise stream's statistics at the length the GPU test uses, its edges (the extreme
Philox words, windows, frames, the seed's two halves), a scalar re-evaluation in Python integers and the math module, and the
convolution against a direct double sum.

Statistics of noise(seed, frame 2, 2 097 667 samples, noise_var 0.25), as first computed on a CPU:

    quantity                  seed 1234    seed (7<<32)|5    bound asserted
    variance / 0.25 - 1       -5.2e-4      +2.5e-4           5e-3
    |mean|                     3.6e-4       3.0e-4           2e-3
    I/Q variance ratio - 1     8.5e-4       2e-5             1e-2
    |corr(I, Q)|               1.8e-4       5.0e-4           5e-3
    lag-1 correlation of I     5.6e-4       1.1e-3           5e-3
    largest |z| / sigma        5.36         5.85             -

Each bound is several times the estimator's own spread at n = 2.1e6 (variance and ratio ~1e-3, mean ~3.5e-4, the correlations
~7e-4), and far below what a broken generator gives (a shared word, a wrong angle unit or a repeated pair move them by O(0.1..1))."""
import math

import numpy as np
import pytest

import channel_ref as cr

LONG = 2 * 4096 * 256 + 515                # the first frame length at which the kernel's grid loops, last pair partial
SEEDS = (1234, (7 << 32) | 5)


@pytest.fixture(scope="module")
def long_noise():
    return {s: cr.noise(s, 1, LONG, 0.25, first_frame=2)[0] for s in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_statistics_of_a_long_frame(long_noise, seed):
    z = long_noise[seed]
    assert z.shape == (LONG,) and np.all(np.isfinite(z.real)) and np.all(np.isfinite(z.imag))
    ur, ua = cr.uniforms(seed, 1, LONG, first_frame=2)
    assert ur.max() < 1.0 and ua.max() < 1.0 and ur.min() > 0.0, "a u of this stream rounds to 1.0"
    st = cr.statistics(z, 0.25)
    print("seed %#x: %s" % (seed, ", ".join("%s %.3g" % kv for kv in st.items())))
    assert not cr.within_bounds(st), cr.within_bounds(st)
    assert 5.0 < st["peak"] < 6.76 + 1e-6                                  # sqrt(2 * 33 ln 2): the radius of the word 0


def test_recorded_figures(long_noise):
    """the table of the module docstring, to the digits it is written in"""
    want = {SEEDS[0]: dict(var=-5.2e-4, mean=3.6e-4, iq=8.5e-4, corr_iq=1.8e-4, lag1=5.6e-4, peak=5.36),
            SEEDS[1]: dict(var=2.5e-4, mean=3.0e-4, iq=2e-5, corr_iq=5.0e-4, lag1=1.1e-3, peak=5.85)}
    for seed in SEEDS:
        st = cr.statistics(long_noise[seed], 0.25)
        for k, v in want[seed].items():
            assert abs(abs(st[k]) - abs(v)) < (0.006 if k == "peak" else 0.6e-4), (hex(seed), k, st[k], v)


def test_the_extreme_words_give_a_finite_radius():
    u = cr.uniform([0, 0xFFFFFFFF, 0xFFFFFF7F, 0xFFFFFF80])
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.0)      # 2^32 - 1 rounds to 2^32, + 0.5 is absorbed
    assert u[2] == np.float32(1.0 - 2.0 ** -24) and u[3] == np.float32(1.0)          # the last word below 1, the first at it (tie to even)
    r = cr.radius(u)
    assert np.all(np.isfinite(r)) and abs(r[0] - 6.7637) < 1e-4 and r[1] == 0.0
    assert abs(r[2] - math.sqrt(2 * 2.0 ** -24)) < 1e-7                    # 3.45e-4: what one float32 ulp of u is worth next to 1


def test_the_float32_rounding_of_u_is_part_of_the_definition():
    """a float64 u differs from the float32 one by up to half an ulp: next to 1 that moves the radius by ~1e-4 sigma, which a
    comparison at that level would see"""
    w = np.array([0xFFFFFF7F, 0xFFFFFF80, 0x80000041, 12345], np.uint64)
    u64 = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    u32 = cr.uniform(w)
    assert np.any(u32.astype(np.float64) != u64)
    assert np.max(np.abs(cr.radius(u32) - np.sqrt(-2 * np.log(u64)))) > 5e-5
    # and the float32 expression is exactly: round(w) to 24 bits, + 0.5 rounded to 24 bits, scaled by a power of two
    for wi, ui in zip(w.tolist(), u32.tolist()):
        assert ui == float(np.float32(np.float32(wi) + np.float32(0.5))) * 2.0 ** -32


def _philox_scalar(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_scalar_philox_has_the_random123_known_answers():
    assert _philox_scalar((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert _philox_scalar((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert _philox_scalar((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


@pytest.mark.parametrize("seed", (0, 1234, (7 << 32) | 5))
def test_samples_equal_a_scalar_evaluation_of_the_definition(seed):
    nv = 0.25
    z = cr.noise(seed, 3, 1001, nv)
    sig = float(np.float32(math.sqrt(np.float32(nv) / np.float32(2))))
    for f, n in ((0, 0), (0, 1), (1, 0), (2, 1), (1, 500), (2, 777), (2, 1000)):
        w = _philox_scalar((n // 2, 0, f, 0), (seed & 0xFFFFFFFF, seed >> 32))
        u = [float((np.float32(x) + np.float32(0.5)) * np.float32(2.0 ** -32)) for x in w]
        ur, ua = u[2 * (n % 2)], u[2 * (n % 2) + 1]
        r = sig * math.sqrt(-2 * math.log(ur))
        want = complex(r * math.cos(2 * math.pi * ua), r * math.sin(2 * math.pi * ua))
        assert abs(z[f, n] - want) < 1e-14, (f, n)


@pytest.mark.parametrize("m", (1, 2, 7, 500, 1001))
def test_a_shorter_call_is_a_window_of_a_longer_one(m):
    full = cr.noise(99, 2, 1002, 1e-6)
    assert np.array_equal(cr.noise(99, 2, m, 1e-6), full[:, :m])


def test_frames_and_seed_halves_give_different_noise():
    z = cr.noise(5, 3, 64, 0.25)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.any(z[a] == z[b])
    assert np.array_equal(cr.noise(5, 1, 64, 0.25, first_frame=2)[0], z[2])
    hi = cr.noise((7 << 32) | 5, 3, 64, 0.25)
    assert not np.any(hi == z)
    assert cr.noise(5, 0, 64, 0.25).shape == (0, 64) and cr.noise(5, 3, 0, 0.25).shape == (3, 0)


def test_noise_scales_with_sigma_as_the_entry_point_rounds_it():
    a, b = cr.noise(1, 1, 100, 0.25), cr.noise(1, 1, 100, 1e-6)
    assert float(cr.sigma(1e-6)) == float(np.sqrt(np.float32(1e-6) / np.float32(2))) and cr.sigma(0.25).dtype == np.float32
    assert np.allclose(b / float(cr.sigma(1e-6)), a / float(cr.sigma(0.25)), rtol=1e-15, atol=0)


def test_conv_equals_a_direct_sum():
    rng = np.random.default_rng(11)
    for n_frames, in_len, n_taps, per_frame in ((1, 1, 9, False), (3, 7, 9, True), (2, 12, 2, True), (3, 5, 1, False)):
        x = rng.standard_normal((n_frames, in_len)) + 1j * rng.standard_normal((n_frames, in_len))
        t = rng.standard_normal((n_frames, n_taps)) + 1j * rng.standard_normal((n_frames, n_taps))
        taps = t if per_frame else t[0]
        for out_len in sorted({0, 1, max(0, in_len - 3), in_len, in_len + n_taps - 1}):
            y = cr.conv(x.astype(np.complex64), taps.astype(np.complex64), out_len)
            assert y.shape == (n_frames, out_len) and y.dtype == np.complex128
            for f in range(n_frames):
                h = (t[f] if per_frame else t[0]).astype(np.complex64).astype(np.complex128)
                xf = x[f].astype(np.complex64).astype(np.complex128)
                for n in range(out_len):
                    want = sum(h[l] * xf[n - l] for l in range(n_taps) if 0 <= n - l < in_len)
                    assert abs(y[f, n] - want) < 1e-12
    with pytest.raises(AssertionError):
        cr.conv(np.zeros((1, 4)), np.ones(3), 7)
