"""The loop-back channel of ofdm_channel_apply (include/ofdm_mi355x.h) restated in NumPy: the tapped-delay-line convolution in
complex128 and the AWGN stream as the header defines it, sample by sample.  This is the yardstick channel_kernel
(csrc/tx_kernels.hip) is held against; tests/test_channel_ref_host.py pins this file by independent means.  No device code, and
the library is not imported.

The noise is a pure function of (seed, frame index within the call, sample index within the frame).  Only the step from a Philox
word to the uniform u is float32 (one add, one multiply, both exact IEEE operations the device repeats bit for bit); everything
behind it is float64, so what the device differs by is the error of its float32 log / sqrt / sin / cos."""
import numpy as np

from oracle import ofdm_oracle as orc


def conv(x, taps, out_len):
    """x [n_frames][in_len], taps [n_taps] (shared) or [n_frames][n_taps] -> [n_frames][out_len] complex128: np.convolve per
    frame, the tail beyond out_len dropped."""
    x = np.atleast_2d(np.asarray(x)).astype(np.complex128)
    taps = np.asarray(taps).astype(np.complex128)
    n_frames, in_len = x.shape
    assert taps.ndim == 1 or taps.shape[0] == n_frames
    n_taps = taps.shape[-1]
    assert 0 <= out_len <= in_len + n_taps - 1
    y = np.zeros((n_frames, out_len), np.complex128)
    if in_len == 0:
        return y
    for f in range(n_frames):
        y[f] = np.convolve(x[f], taps if taps.ndim == 1 else taps[f])[:out_len]
    return y


def uniform(w):
    """Philox word(s) -> u in (0, 1]: (float32(w) + 0.5f) * 2^-32 in float32 (the conversion rounds to nearest even)."""
    w = np.asarray(w, dtype=np.uint64).astype(np.uint32)
    return (w.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def sigma(noise_var):
    """standard deviation per component, as the C entry point computes it: float32(sqrt(float32(noise_var) / 2))"""
    return np.sqrt(np.float32(noise_var) / np.float32(2))


def radius(u):
    """sqrt(-2 ln u) in float64 of the float32 u"""
    return np.sqrt(-2.0 * np.log(np.asarray(u).astype(np.float64)))


def uniforms(seed, n_frames, out_len, first_frame=0):
    """-> (u_radius, u_angle) float32 [n_frames][out_len]: sample n = 2p + i of frame f takes words 2i, 2i + 1 of
    philox4x32_10(counter = (p & 0xFFFFFFFF, p >> 32, f, 0), key = (seed & 0xFFFFFFFF, seed >> 32))."""
    seed = int(seed)
    n_pairs = (int(out_len) + 1) // 2
    p = np.arange(n_pairs, dtype=np.uint64)
    ur = np.empty((n_frames, 2 * n_pairs), np.float32)
    ua = np.empty((n_frames, 2 * n_pairs), np.float32)
    for i in range(n_frames):
        f = np.full(n_pairs, first_frame + i, np.uint64)
        w = orc.philox4x32_10(p & np.uint64(0xFFFFFFFF), p >> np.uint64(32), f, 0 * p, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        ur[i, 0::2], ua[i, 0::2], ur[i, 1::2], ua[i, 1::2] = (uniform(x) for x in w)
    return ur[:, :out_len], ua[:, :out_len]


def noise(seed, n_frames, out_len, noise_var, first_frame=0):
    """-> complex128 [n_frames][out_len], frames first_frame .. first_frame + n_frames - 1 of a call:
    sigma * sqrt(-2 ln u_radius) * exp(2 pi j u_angle)."""
    ur, ua = uniforms(seed, n_frames, out_len, first_frame)
    return float(sigma(noise_var)) * radius(ur) * np.exp(2j * np.pi * ua.astype(np.float64))


def statistics(z, noise_var):
    """the figures the tests bound, of one frame of noise: dict(var, mean, iq, corr_iq, lag1, peak)"""
    z = np.asarray(z).astype(np.complex128).ravel()
    i, q = z.real, z.imag
    return dict(var=float(np.mean(np.abs(z) ** 2) / noise_var - 1), mean=float(abs(np.mean(z))),
                iq=float(np.var(i) / np.var(q) - 1), corr_iq=float(abs(np.corrcoef(i, q)[0, 1])),
                lag1=float(abs(np.corrcoef(i[:-1], i[1:])[0, 1])), peak=float(np.max(np.abs(z)) / float(sigma(noise_var))))


# the bounds of the statistics of 2 097 667 samples (tests/test_channel_ref_host.py states where they come from)
BOUNDS = dict(var=5e-3, mean=2e-3, iq=1e-2, corr_iq=5e-3, lag1=5e-3)


def within_bounds(st):
    """-> list of the statistics outside BOUNDS (empty: all inside)"""
    return ["%s = %.3g (bound %g)" % (k, st[k], b) for k, b in BOUNDS.items() if not abs(st[k]) < b]
