"""GPU parity of the two code paths of the dense demod kernel (run with -m gpu).

From 1024-pt up `rx_demod_kernel` exists twice per constellation and bit layout: with the bin-list length compiled in (KD = 600 /
1200 / 2400, the LTE numerologies -- `DemodGeom<N>::KD_LTE`) and with the runtime `Kd` for everything else.  `launch_rx_demod_n`
picks by `rx.Kd`.  Both are held against the fp64 oracle here with the suite's `assert_close`, the bits exactly:

* the compiled-in `Kd`: every constellation x packed / unpacked / no bits, with and without the equalised-symbol output
  (BPSK has no packed layout: the API refuses an odd number of bits per symbol there);
* `Kd` +- 4, a small and two near-full `Kd` (N - 4 packed, N - 2 unpacked): the runtime-Kd kernel right beside the compiled-in one;
* guard-failed patterns and short-tail frames on the compiled-in path: rows of zeros, zero-padded rows, NaN rows, every row
  WRITTEN into 0xFF-poisoned buffers;
* a batch of more than twice the resident workgroups, so that the work queue and the compiled-in kernel meet: every frame of
  it must equal, bit for bit, the same frame demodulated in a small batch (no queue) that was checked against the oracle."""
import numpy as np
import pytest

from conftest import assert_close, poisoned
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

# (N, cp, compiled-in Kd, symbols per frame)
SIZES = [(1024, 72, 600, 12), (2048, 144, 1200, 12), (4096, 288, 2400, 8)]
MODS = ["BPSK", "QPSK", "16QAM", "64QAM"]
LAYOUTS = [(m, lay) for m in MODS for lay in ("packed", "unpacked") if not (m == "BPSK" and lay == "packed")]


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


def _frame(N, cp, Kd, n_sym, mod, lead, rng, fl, sigma=0.02):
    bps = orc.BITS_PER_SYMBOL[mod]
    bits = rng.integers(0, 2, (n_sym // 4) * 3 * Kd * bps).astype(np.uint8)
    tx = orc.channel_apply(orc.tx_modulate(bits, N, cp, N - 2, Kd, n_sym, modulation=mod), orc.REF_TAPS, N)
    pre = 0.3 * (rng.standard_normal(lead) + 1j * rng.standard_normal(lead))
    x = np.concatenate([pre, tx])[:fl]
    x = np.concatenate([x, np.zeros(fl - len(x))])
    return (x + sigma * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)


def _demod(om, N, cp, Kd, n_sym, mod, layout, iq, with_eq=True):
    """iq [n_frames, fl] through ofdm_rx_demod_frames into poisoned buffers -> (eq or None, bit rows or None, tsr)."""
    n_frames, fl = iq.shape
    bps = orc.BITS_PER_SYMBOL[mod]
    rx = om.RxEngine(n_sym, N, cp, N - 2, (1, 3), Kd, 30, 0.7, modulation=mod)
    rx.set_max_trials(0)
    nds = rx.data_symbols_per_frame(fl)
    nbits = n_frames * nds * Kd * bps
    packed = layout == "packed"
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    d_eq = poisoned(om, n_frames * nds * Kd * 8) if with_eq else None
    d_b = None if layout is None else poisoned(om, nbits // 8 if packed else nbits)
    d_tsr = poisoned(om, n_frames * 16)
    mode = om.BITS_NONE if layout is None else om.BITS_PACKED if packed else om.BITS_UNPACKED
    assert rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_b, mode, d_tsr) == nds
    eq = d_eq.download(np.complex64, n_frames * nds * Kd).reshape(n_frames, nds, Kd) if with_eq else None
    b = None
    if layout is not None:
        b = d_b.download(np.uint8, nbits // 8 if packed else nbits)
        b = (np.unpackbits(b) if packed else b).reshape(n_frames, nds, Kd * bps)
        assert b.max() <= 1, "bit rows left unwritten (0xFF poison)"
    return eq, b, d_tsr.download(np.int32, n_frames * 4).reshape(n_frames, 4)


def _against_oracle(N, cp, Kd, n_sym, mod, iq, eq, b, tsr):
    """EVERY row of every frame against the oracle: zero rows, zero-padded rows and NaN rows included.  -> (zero rows, padded rows)"""
    n_frames, fl = iq.shape
    nds = eq.shape[1]
    n_rows = fl // (N + cp)
    keep = [r for r in range(max(n_sym, n_rows)) if r % 4 != 3][:nds]
    seen_zero = seen_pad = 0
    for f in range(n_frames):
        o = orc.RxOracle(max(n_sym, n_rows), N, cp, N - 2, [1, 3], Kd, 30, 0.7, force_fp64=True)
        with np.errstate(all="ignore"):
            o.work(iq[f], np.zeros(fl, np.complex64))
        assert tsr[f, 3] == 1 and tsr[f, 0] == o.time_synch_ref[0] and tsr[f, 1] == o.time_synch_ref[1], (f, tsr[f], o.time_synch_ref)
        ref = o.est_data_freq[keep]
        nan_ref = ~np.isfinite(ref).all(axis=1)
        nan_gpu = ~np.isfinite(eq[f]).all(axis=1)
        assert np.array_equal(nan_ref, nan_gpu), (f, nan_ref, nan_gpu)
        zero_ref = ~nan_ref & ~ref.any(axis=1)
        assert not eq[f][zero_ref].any(), "frame %d: rows %s must be zeros" % (f, np.nonzero(zero_ref)[0])
        live = ~nan_ref & ~zero_ref
        assert_close(eq[f][live], ref[live], "N %d Kd %d %s frame %d" % (N, Kd, mod, f))
        t0 = int(o.time_synch_ref[0])
        seen_pad += sum(1 for r in np.nonzero(live)[0] if t0 + (r // 3 * 4 + 1 + r % 3) * (N + cp) + N > fl)
        seen_zero += int(zero_ref.sum())
        if b is not None:
            ok = ~nan_ref
            assert np.array_equal(b[f][ok].ravel(), orc.demap_hard(eq[f][ok].ravel(), mod)), "frame %d: bits" % f
            zb = orc.demap_hard(np.zeros(Kd, np.complex64), mod)
            for r in np.nonzero(zero_ref)[0]:
                assert np.array_equal(b[f][r], zb)
    return seen_zero, seen_pad


def _two_frames(N, cp, Kd, n_sym, mod, seed):
    rng = np.random.default_rng(seed)
    fl = n_sym * (N + cp) + 7
    return np.stack([_frame(N, cp, Kd, n_sym, mod, 0, rng, fl), _frame(N, cp, Kd, n_sym, mod, 5, rng, fl)])


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("N,cp,Kd,n_sym", SIZES)
def test_compiled_in_kd_every_output_combination(om, N, cp, Kd, n_sym, mod):
    iq = _two_frames(N, cp, Kd, n_sym, mod, N + len(mod))
    eq0, none, tsr = _demod(om, N, cp, Kd, n_sym, mod, None, iq)                      # equalised symbols only
    assert none is None
    _against_oracle(N, cp, Kd, n_sym, mod, iq, eq0, None, tsr)
    for m, layout in LAYOUTS:
        if m != mod:
            continue
        eq, b, tsr = _demod(om, N, cp, Kd, n_sym, mod, layout, iq)
        assert np.array_equal(eq, eq0), "%s: the symbols depend on the bit layout" % layout
        _against_oracle(N, cp, Kd, n_sym, mod, iq, eq, b, tsr)
        none, b_only, _ = _demod(om, N, cp, Kd, n_sym, mod, layout, iq, with_eq=False)      # bits without the symbol output
        assert none is None and np.array_equal(b_only, b), "%s: the bits depend on whether the symbols are written" % layout


@pytest.mark.parametrize("N,cp,Kd0,n_sym", SIZES)
def test_runtime_kd_beside_the_compiled_in_one(om, N, cp, Kd0, n_sym):
    cases = [(Kd0 - 4, "16QAM", "packed"), (Kd0 + 4, "QPSK", "packed"), (Kd0 + 4, "64QAM", "unpacked"), (Kd0 - 4, "BPSK", "unpacked"),
             (64, "16QAM", "packed"), (64, "QPSK", None), (N - 4, "64QAM", "packed"), (N - 2, "QPSK", "unpacked"), (N - 2, "16QAM", None)]
    for Kd, mod, layout in cases:
        iq = _two_frames(N, cp, Kd, n_sym, mod, N + Kd)
        eq, b, tsr = _demod(om, N, cp, Kd, n_sym, mod, layout, iq)
        _against_oracle(N, cp, Kd, n_sym, mod, iq, eq, b, tsr)
        if layout is not None:
            none, b_only, _ = _demod(om, N, cp, Kd, n_sym, mod, layout, iq, with_eq=False)
            assert np.array_equal(b_only, b), (Kd, mod, layout)


def _edge_frames(N, cp, Kd, n_sym, mod, seed):
    L = N + cp
    rng = np.random.default_rng(seed)
    fl = n_sym * L + 7
    return np.stack([
        _frame(N, cp, Kd, n_sym, mod, 0, rng, fl),                                   # aligned: every pattern fits
        _frame(N, cp, Kd, n_sym, mod, 2 * L + cp + 16, rng, fl),                     # last pattern fails the guard: rows of zeros
        _frame(N, cp, Kd, n_sym, mod, 3 * L + 3, rng, fl),                           # the same, other offset
        _frame(N, cp, Kd, n_sym, mod, L // 2, rng, fl),                              # guard passes, last window zero-padded
    ])


@pytest.mark.parametrize("mod,layout", [("QPSK", "unpacked"), ("16QAM", "packed"), ("64QAM", "packed"), ("BPSK", "unpacked"), ("QPSK", None)])
@pytest.mark.parametrize("N,cp,Kd,n_sym", SIZES)
def test_compiled_in_kd_zero_fill_and_short_tail(om, N, cp, Kd, n_sym, mod, layout):
    iq = _edge_frames(N, cp, Kd, n_sym, mod, N * 3 + len(mod))
    eq, b, tsr = _demod(om, N, cp, Kd, n_sym, mod, layout, iq)
    zeros, padded = _against_oracle(N, cp, Kd, n_sym, mod, iq, eq, b, tsr)
    assert zeros >= 6 and padded >= 1                                                # two frames x one failed pattern of three rows


# Frames per batch so that the launch has more than twice the resident workgroups and the queue is on.  One chunk per frame at
# these frame lengths; resident workgroups = workgroups per CU x 256 CUs: at most 3 per CU at 2048 / 4096-pt (LDS: 47.7 / 52.8 KB
# of 160 KB) and at most 8 at 1024-pt (two waves per workgroup, 16 waves per CU at three to four waves per SIMD).
QUEUE_FRAMES = {1024: 4200, 2048: 1700, 4096: 1700}


@pytest.mark.parametrize("mod,layout", [("16QAM", "packed"), ("QPSK", "unpacked")])
@pytest.mark.parametrize("N,cp,Kd,n_sym", SIZES)
def test_compiled_in_kd_under_the_work_queue(om, N, cp, Kd, n_sym, mod, layout):
    base = _edge_frames(N, cp, Kd, n_sym, mod, N * 5 + len(mod))
    eq0, b0, tsr0 = _demod(om, N, cp, Kd, n_sym, mod, layout, base)
    _against_oracle(N, cp, Kd, n_sym, mod, base, eq0, b0, tsr0)
    n = QUEUE_FRAMES[N]
    pick = np.arange(n) % len(base)
    eq, b, tsr = _demod(om, N, cp, Kd, n_sym, mod, layout, base[pick])
    assert np.array_equal(tsr, tsr0[pick])
    assert np.array_equal(eq.view(np.uint32), eq0[pick].view(np.uint32)), "a frame of the large batch differs from the small batch"
    assert np.array_equal(b, b0[pick])
