"""tests/dft_spread_ref.py pinned without a GPU: the restated transforms against a direct matrix product, Parseval and the
spread -> despread identity, step 3's nu / beta^2 against a Monte-Carlo variance of the unbiased despread symbol, the erasure
rules, and the peak-to-average power ratio that is the reason for the waveform."""
import math

import numpy as np
import pytest

import dft_spread_ref as ref
from oracle import ofdm_oracle as orc

SIZES_SMALL = [m for m in range(1, 76) if ref.size_ok(m)]


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("M", SIZES_SMALL)
def test_transforms_equal_the_matrix_product(M):
    rng = np.random.default_rng(M)
    x = crandn(rng, 3, M)
    k = np.arange(M)
    F = np.exp(-2j * np.pi * np.outer(k, k) / M) / math.sqrt(M)
    assert np.allclose(ref.spread(x), x @ F.T, rtol=0, atol=1e-12 * M)
    assert np.allclose(ref.inverse(x), x @ F.conj().T, rtol=0, atol=1e-12 * M)


@pytest.mark.parametrize("M", [1, 12, 60, 75, 1200, 2187, 4096])
def test_parseval_and_identity(M):
    rng = np.random.default_rng(M)
    x = crandn(rng, 4, M)
    z = ref.spread(x)
    assert np.allclose(np.sum(np.abs(z) ** 2, axis=1), np.sum(np.abs(x) ** 2, axis=1), rtol=1e-12)
    assert np.allclose(ref.inverse(z), x, rtol=0, atol=1e-12)
    u, wt, erased = ref.despread_segment(z.astype(np.complex64), None, 0.0, 1.0)
    assert wt["beta32"] == 1 and wt["weight32"] == 1 and not erased.any()
    assert np.max(np.abs(u - x)) < 1e-6 * np.max(np.abs(x))


def test_size_rule():
    ok = [m for m in range(-2, 4200) if ref.size_ok(m)]
    assert len(ok) == 137 and ok[0] == 1 and ok[-1] == 4096 and 1200 in ok and 2400 in ok and 7 not in ok and 4200 not in ok


@pytest.mark.parametrize("sigma2,rho", [(0.05, 0.05), (0.05, 0.02), (0.01, 0.03)])
def test_weight_rule_predicts_the_error_variance(sigma2, rho):
    """The reference's 5-tap channel, M = 60, 20 000 rows of 16-QAM through the one-tap MMSE equaliser with regulariser rho at
    noise variance sigma2 (matched and mismatched): the error variance of the unbiased despread symbol is nu / beta^2 within 2 %."""
    M, rows = 60, 20000
    rng = np.random.default_rng(36211)
    taps = orc.REF_TAPS / np.linalg.norm(orc.REF_TAPS)
    H = np.fft.fft(taps, 64)[orc.bins_p(M, 64)]
    a = (np.abs(H) ** 2).astype(np.float32)
    x = orc.map_bits(rng.integers(0, 2, rows * M * 4), "16QAM").reshape(rows, M)
    y = H * ref.spread(x) + crandn(rng, rows, M) * math.sqrt(sigma2 / 2)
    z = np.conj(H) / (a.astype(np.float64) + float(np.float32(rho))) * y
    u, wt, erased = ref.despread_segment(z.astype(np.complex64), a, rho, sigma2)
    assert wt["usable"] and not erased.any()
    measured = float(np.mean(np.abs(u - x) ** 2))
    predicted = wt["nu"] / wt["beta"] ** 2
    print("sigma2 %.3g rho %.3g: measured %.5f predicted %.5f" % (sigma2, rho, measured, predicted))
    assert abs(measured - predicted) < 0.02 * predicted
    assert abs(float(wt["weight32"]) * predicted - 1) < 1e-6


def test_erasure_rules():
    rng = np.random.default_rng(5)
    M, rows = 12, 4
    a = rng.uniform(0.1, 2.0, M).astype(np.float32)
    z = crandn(rng, rows, M).astype(np.complex64)
    a[3], a[7] = 0.0, np.nan
    z[1, 5] = complex(np.nan, 1.0)
    z[2] = 0
    zp = ref.masked(z, a)
    assert not zp[:, 3].any() and not zp[:, 7].any() and zp[1, 5] == 0 and zp[0, 5] != 0 and np.isfinite(zp.view(np.float64)).all()
    u, wt, erased = ref.despread_segment(z, a, 0.03, 0.01)
    assert list(erased) == [False, False, True, False] and not u[2].any() and u[0].any() and wt["usable"]
    b = np.where(ref.usable_entries(a), a.astype(np.float64) / (a.astype(np.float64) + float(np.float32(0.03))), 0.0)
    assert abs(wt["beta"] - b.sum() / M) < 1e-15
    # a row that only holds entries the mask removes is an erasure as well
    z2 = np.zeros((1, M), np.complex64)
    z2[0, 3] = 1
    assert ref.despread_segment(z2, a, 0.03, 0.01)[2][0]
    # no usable entry, a variance that is not finite or an underflowing 1/beta: the segment is not usable, everything is +0
    for aa, s2 in ((np.zeros(M, np.float32), 0.01), (a, math.inf), (a, math.nan), (np.full(M, 1e-44, np.float32), 0.01)):
        u, wt, _ = ref.despread_segment(z, aa, 0.03, s2)
        assert not wt["usable"] and wt["beta32"] == 0 and wt["weight32"] == 0 and not u.any()
    # a huge variance keeps the symbols and takes the weight to +0
    u, wt, _ = ref.despread_segment(z, a, 0.03, 1e300)
    assert wt["usable"] and wt["weight32"] == 0 and wt["beta32"] > 0 and u[0].any()
    llr, bits = ref.outputs_from(u.astype(np.complex64), wt["weight32"], "64QAM")
    assert not llr.view(np.uint32).any()
    # outputs of zero symbols: +0 LLRs whatever the weight, the bits of a zero symbol
    llr, bits = ref.outputs_from(np.zeros(3, np.complex64), np.float32(2.0), "64QAM")
    assert not llr.view(np.uint32).any() and np.array_equal(bits, np.tile(orc.demap_hard(np.zeros(1, np.complex64), "64QAM"), 3))


def test_papr_is_at_least_2_db_below_plain_ofdm():
    """QPSK, M = 60 in a 256-point grid (4x oversampled), 20 000 symbols each: 99.9th percentile of the PAPR"""
    rng = np.random.default_rng(2)
    M, N, n = 60, 256, 20000
    x = orc.map_bits(rng.integers(0, 2, n * M * 2), "QPSK").reshape(n, M)
    bins = orc.bins_p(M, N)

    def papr_db(rows):
        g = np.zeros((n, N), np.complex128)
        g[:, bins] = rows
        p = np.abs(np.fft.ifft(g, axis=1)) ** 2
        return 10 * np.log10(p.max(axis=1) / p.mean(axis=1))

    plain, spread = papr_db(x), papr_db(ref.spread(x))
    q = [float(np.percentile(v, 99.9)) for v in (plain, spread)]
    print("PAPR median %.2f / %.2f dB, 99.9 %% %.2f / %.2f dB (plain / DFT-spread)" % (np.median(plain), np.median(spread), q[0], q[1]))
    assert q[0] - q[1] >= 2.0


# ------------------------------------------------------------------------------------------ the link case, on the reference alone
def received_frames(noise_var):
    """the case's frames, transform-precoded, through the oracle's receiver -> (z [frames][9][60] complex64 equalised rows,
    a [frames][60] float32 channel powers, info bits, coded bits [frames][SEG_BITS])"""
    import channel_ref
    import csi_ref
    import dft_spread_cases as dc
    import turbo_ref
    info = dc.info_bits()
    coded = turbo_ref.encode_segments(info, dc.F1, dc.F2, dc.SEG_BITS)
    rows = [r for r in range(dc.N_SYM) if r % 4 != 3]
    bins = orc.bins_p(dc.KD, dc.N)
    noise = channel_ref.noise(dc.SEED_NOISE, dc.N_FRAMES, dc.FRAME_LEN, noise_var)
    z = np.zeros((dc.N_FRAMES, dc.N_DSYM, dc.KD), np.complex64)
    a = np.zeros((dc.N_FRAMES, dc.KD), np.float32)
    for f in range(dc.N_FRAMES):
        spread = ref.spread(orc.map_bits(coded[f], dc.MOD).reshape(dc.N_DSYM, dc.KD))
        tx = orc.tx_modulate(None, dc.N, dc.CP, dc.KS, dc.KD, dc.N_SYM, modulation=dc.MOD, data_symbols=spread)
        y = np.convolve(tx, dc.TAPS)[:dc.FRAME_LEN - dc.LEAD]
        x = np.zeros(dc.FRAME_LEN, complex)
        x[dc.LEAD:dc.LEAD + len(y)] = y
        x += noise[f]
        o = orc.RxOracle(dc.N_SYM, dc.N, dc.CP, dc.KS, [1, 3], dc.KD, dc.SNR_ARG, dc.GATE, force_fp64=True)
        o.work(x.astype(np.complex64), np.zeros(dc.FRAME_LEN, np.complex64))
        z[f] = o.est_data_freq[rows]
        a[f] = csi_ref.csi_row(o.est_chan_freq_P[0].astype(np.complex64), bins)
    return z, a, info, coded


def link_result(noise_var):
    """-> (blocks lost of 64, error rate of the undecoded hard bits of the code blocks) of the restated chain at this noise
    level.  The filler zeros behind a frame's 3K + 12 coded bits are left out of the rate: a row of equal symbols is one spectral
    line after the precoder, the transmitter's per-symbol power normalisation rescales it, and its bits belong to no block."""
    import dft_spread_cases as dc
    import turbo_ref
    rho = np.float32(1.0 / 10.0 ** (dc.SNR_ARG / 20.0))
    z, a, info, coded = received_frames(noise_var)
    llr = np.zeros((dc.N_FRAMES, dc.SEG_BITS), np.float32)
    wrong, n_coded = 0, 3 * dc.K + 12
    for f in range(dc.N_FRAMES):
        u, wt, _ = ref.despread_segment(z[f], a[f], rho, float(rho))          # OFDM_DESPREAD_NOISE_RHO
        assert wt["usable"]
        llr[f], hard = ref.outputs_from(u.astype(np.complex64), wt["weight32"], dc.MOD)
        wrong += int(np.count_nonzero(hard[:n_coded] != coded[f][:n_coded]))
    bits, _ = turbo_ref.decode_segments(llr, 1, dc.K, dc.F1, dc.F2, dc.N_ITER)
    return int((bits != info).any(axis=(1, 2)).sum()), wrong / float(dc.N_FRAMES * n_coded)


def test_link_case_on_the_reference():
    import dft_spread_cases as dc
    assert ref.size_ok(dc.KD)
    res = {name: link_result(nv) for name, nv in (("level", dc.NOISE_VAR), ("1 dB up", dc.NOISE_VAR_1DB))}
    print("blocks lost of %d, undecoded bit error rate: %r" % (dc.N_FRAMES, res))
    assert res["level"][0] == 0 and res["1 dB up"][0] == 0
    assert res["level"][1] >= 0.01                                  # the decoder is exercised
