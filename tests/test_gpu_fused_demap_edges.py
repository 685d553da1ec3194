"""The fused de-mapper of ofdm_rx_demod_frames end to end at its decision edges (run with -m gpu).

Below 1024-pt the packed bits come from pack4 (4 list entries per lane); from 1024-pt on the dense output mapping hands a lane
pairs of entries and packs them with pack2, then exchanges halves through a quad permute; unpacked bits go through hard_bits.
tests/test_demap_rules.py pins those functions input by input; this file drives them through the whole kernel, on symbols
that sit exactly at 0+0j and on symbols whose equalised coordinates land on the thresholds.
"""
import numpy as np
import pytest

import demap_corpus as dc
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu
MOD_NAMES = ["QPSK", "16QAM", "64QAM"]
GEOM = {256: (18, 152), 1024: (72, 600), 2048: (144, 1200), 4096: (288, 2400)}       # N: (cp, Kd)


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


def _demod_both(om, rx, iq, n_frames, nds, Kd, bps):
    """-> (eq [n_frames, nds, Kd], packed bits unpacked [n_frames, nds*Kd*bps], unpacked bits [same]) of one frame batch"""
    fl = iq.shape[1]
    nb = n_frames * nds * Kd * bps
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    d_eq = om.DeviceBuffer(n_frames * nds * Kd * 8)
    d_eq2 = om.DeviceBuffer(n_frames * nds * Kd * 8)
    d_bp = om.DeviceBuffer(nb // 8)
    d_bu = om.DeviceBuffer(nb)
    rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_bp, om.BITS_PACKED, None)
    rx.demod_frames(d_iq, n_frames, fl, fl, d_eq2, d_bu, om.BITS_UNPACKED, None)
    eq = d_eq.download(np.complex64, n_frames * nds * Kd)
    assert np.array_equal(eq.view(np.uint32), d_eq2.download(np.complex64, n_frames * nds * Kd).view(np.uint32))
    bp = np.unpackbits(d_bp.download(np.uint8, nb // 8)).reshape(n_frames, -1)
    bu = d_bu.download(np.uint8, nb).reshape(n_frames, -1)
    return eq.reshape(n_frames, nds, Kd), bp, bu


@pytest.mark.parametrize("mod", MOD_NAMES)
@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_fused_demapper_on_exact_zero_symbols_all_paths(om, N, mod):
    """Ks < Kd: the data bins outside the sync span have H = 0 and equalise to exactly 0+0j, which must carry demap_hard(0)
    -- at 256-pt through pack4, from 1024-pt through pack2 and the dense exchange, and unpacked through hard_bits."""
    cp, Kd = GEOM[N]
    Ks, n_sym, n_frames = Kd // 2, 8, 2
    bps = orc.BITS_PER_SYMBOL[mod]
    nds = 6
    rng = np.random.default_rng(N + bps)
    bits = rng.integers(0, 2, (n_frames, nds * Kd * bps)).astype(np.uint8)
    iq = np.stack([orc.tx_modulate(bits[f], N, cp, Ks, Kd, n_sym, modulation=mod) for f in range(n_frames)]).astype(np.complex64)
    rx = om.RxEngine(n_sym, N, cp, Ks, (1, 3), Kd, 100, 0.7, modulation=mod)
    assert rx.data_symbols_per_frame(iq.shape[1]) == nds
    eq, bp, bu = _demod_both(om, rx, iq, n_frames, nds, Kd, bps)
    h = Kd // 2
    outside = np.r_[0:h - Ks // 2, h + Ks // 2:Kd]             # list entries of bins |k| > Ks/2
    inside = np.r_[h - Ks // 2:h + Ks // 2]
    assert not eq[:, :, outside].any() and eq[:, :, inside].all()
    want = orc.demap_hard(eq.ravel(), mod).reshape(n_frames, -1)
    assert np.array_equal(bp, want), "packed"
    assert np.array_equal(bu, want), "unpacked"
    zero_bits = orc.demap_hard(np.zeros(1, np.complex64), mod)
    w4 = want.reshape(n_frames, nds, Kd, bps)
    assert np.array_equal(w4[:, :, outside], np.broadcast_to(zero_bits, w4[:, :, outside].shape))
    assert np.array_equal(bu.reshape(n_frames, nds, Kd, bps)[:, :, inside], bits.reshape(n_frames, nds, Kd, bps)[:, :, inside])


def _edges(mod):
    return np.array(dc.thresholds(orc.BITS_PER_SYMBOL[mod]), np.float32)


def _near_edge(x, mod, k=2):
    """True where the float32 |x| lies within k ulps of one of the modulation's positive thresholds"""
    ax = np.abs(np.asarray(x, np.float32)).view(np.int32).astype(np.int64)
    e = _edges(mod).view(np.int32).astype(np.int64)
    return (np.abs(ax[..., None] - e) <= k).any(axis=-1)


def _oracle_eq(iq, N, cp, Kd, n_sym):
    o = orc.RxOracle(n_sym, N, cp, N - 2, [1, 3], Kd, 100, 0.7, force_fp64=True)
    o.work(iq, np.zeros(iq.size, np.complex64))
    return o.est_data_freq[[r for r in range(n_sym) if r % 4 != 3]]


def _threshold_frames(N, mod, n_frames, seed):
    """Frames whose equalised data coordinates sit ON the thresholds (noise-free, flat channel, Ks = N - 2).

    The receiver's equalised symbol is eq_k = A_k * d_k / rms(d) per data row: the per-symbol power normalisation divides by the
    row's rms, A_k (the MMSE gain times the lag de-rotation) depends on the sync symbol only.  A_k is read off an fp64 oracle run
    of random data; then a row carries target values T_k on half of its bins (a quarter for QPSK, whose threshold sqrt(2) is
    large) -- coordinates drawn from the thresholds, random signs -- and filler points on the rest, scaled so that the row of
    d_k = T_k / A_k has rms 1 exactly.  Its equalised symbols are then T_k up to fp64 rounding (checked with the oracle)."""
    cp, Kd = GEOM[N]
    n_sym = 8
    nds = 6
    bps = orc.BITS_PER_SYMBOL[mod]
    rng = np.random.default_rng(seed)
    zeros = np.zeros(nds * Kd * bps, np.uint8)
    d0 = orc.map_bits(rng.integers(0, 2, nds * Kd * bps), mod).reshape(nds, Kd)
    eq0 = _oracle_eq(orc.tx_modulate(zeros, N, cp, N - 2, Kd, n_sym, modulation=mod, data_symbols=d0).astype(np.complex64),
                     N, cp, Kd, n_sym)
    rms0 = np.sqrt(np.mean(np.abs(d0) ** 2, axis=1, keepdims=True))
    A = np.mean(eq0 * rms0 / d0, axis=0)
    assert np.max(np.abs(eq0 * rms0 / d0 - A)) < 1e-6 * np.max(np.abs(A))      # one gain per bin (up to the complex64 input)
    edges = _edges(mod).astype(np.float64)
    frac = 0.25 if mod == "QPSK" else 0.5
    iq, targets = [], []
    for _ in range(n_frames):
        T = np.empty((nds, Kd), np.complex128)
        D = np.empty((nds, Kd), np.complex128)
        for r in range(nds):
            thr = rng.permutation(Kd)[:int(frac * Kd)]
            fill = np.setdiff1d(np.arange(Kd), thr)
            sgn = rng.choice([-1.0, 1.0], (2, thr.size))
            cx, cy = rng.choice(edges, thr.size), rng.choice(edges, thr.size)
            if mod == "QPSK":                      # one coordinate on the edge, the other well inside
                other = rng.choice([0.25, 0.5], thr.size)
                on_x = rng.integers(0, 2, thr.size).astype(bool)
                cx, cy = np.where(on_x, cx, other), np.where(on_x, other, cy)
            T[r, thr] = sgn[0] * cx + 1j * sgn[1] * cy
            p = orc.map_bits(rng.integers(0, 2, fill.size * bps), mod)
            s_thr = np.sum(np.abs(T[r, thr] / A[thr]) ** 2)
            s_fill = np.sum(np.abs(p / A[fill]) ** 2)
            f = np.sqrt((Kd - s_thr) / s_fill)
            T[r, fill] = f * p
            D[r] = T[r] / A
        iq.append(orc.tx_modulate(zeros, N, cp, N - 2, Kd, n_sym, modulation=mod, data_symbols=D).astype(np.complex64))
        targets.append(T)
    return np.stack(iq), np.stack(targets)


# Coordinates per frame (6 data symbols) that the GPU's equalised output put within 2 ulps of a threshold: the lowest count
# measured over the modulations at each size (QPSK, 208 / 1558 / 3192 of 228 / 1800 / 3600 planted), halved.  The test must
# prove that it reached the edges.
MIN_NEAR = {256: 100, 2048: 750, 4096: 1500}


@pytest.mark.parametrize("mod", MOD_NAMES)
@pytest.mark.parametrize("N", [256, 2048, 4096])
def test_fused_demapper_on_threshold_coordinates(om, N, mod):
    """Noise-free flat channel, data built so that the equalised coordinates land on the modulation's thresholds: the fused
    bits (packed: pack4 / pack2 + exchange; unpacked: hard_bits) must equal orc.demap_hard of the kernel's own equalised output
    bit for bit, and enough coordinates per frame must lie within 2 ulps of a threshold."""
    cp, Kd = GEOM[N]
    n_sym, nds, n_frames = 8, 6, 2
    bps = orc.BITS_PER_SYMBOL[mod]
    iq, T = _threshold_frames(N, mod, n_frames, seed=N + bps)
    ref = _oracle_eq(iq[0], N, cp, Kd, n_sym)
    assert np.max(np.abs(ref - T[0])) < 1e-6                     # the fp64 receiver puts them on the edges (fp32 input)
    rx = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 100, 0.7, modulation=mod)
    eq, bp, bu = _demod_both(om, rx, iq, n_frames, nds, Kd, bps)
    want = orc.demap_hard(eq.ravel(), mod).reshape(n_frames, -1)
    assert np.array_equal(bp, want), "packed"
    assert np.array_equal(bu, want), "unpacked"
    near = [int(_near_edge(eq[f].real, mod).sum() + _near_edge(eq[f].imag, mod).sum()) for f in range(n_frames)]
    print("near-threshold coordinates per frame N=%d %s: %s" % (N, mod, near))
    assert min(near) >= MIN_NEAR[N], near
