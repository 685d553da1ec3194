"""Seeded hostile inputs of the sync search, shared by tests/test_sync_hostile_ref_host.py (which asserts on the fp64 oracle alone
that every batch sits where it claims) and tests/test_gpu_sync_hostile.py (which holds the screened search to the exhaustive one
and to the oracle on the same arrays).  Plain NumPy, no GPU.  Every function is deterministic.

One base frame per batch.  A frame is `lead | base`, cut to the buffer: every frame of a batch carries the same transmitted
samples and the same noise realisation from the frame start on, only the lead differs.  The channel's strongest tap is its
second, so the first acceptable trial is the one whose window starts one sample after the frame start (P = lead - cp + 1,
lag = cp): that window and every later one hold no lead sample, so the oracle's peak there is ONE fp64 number per batch (m*),
and the engine's gate is planted next to it: m* (1 - d) / MM, the hit passes by d.  For a gate that FAILS by d the planted trial
is the one with the largest peak among hit .. hit + cp (they all see the first sync symbol whole, 1e-4 .. 1e-3 apart), so that
the whole symbol fails -- the best trial by d, the others by more -- and the first trial of the second sync symbol decides."""
import functools
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import ofdm_oracle as orc

# N -> (cp, Kd, n_sym): the sizes of tests/test_gpu_sync_scan.py; 256 is the size of the host test and of the stream test
SIZES = {64: (16, 60, 8), 256: (64, 180, 8), 512: (36, 300, 8), 1024: (72, 600, 8), 2048: (144, 1200, 8), 4096: (288, 2400, 4)}
D_VALUES = (1e-4, 3e-4, 1e-3)
KINDS = ("control", "burst", "dc", "nyq", "gain", "fall")
BURST_DB = (30.0, 34.0, 38.0, 42.0)
OFFSETS = (3.0, 10.0, 25.0)                                  # dc / nyq amplitude in units of the signal rms (1: tx_cp_norm)
GAINS = (1e-4, 1e4)
SIGMA = 0.03                                                 # the frame's noise level (per component)
# The first sync symbol carries 2.5 times the noise of the rest (a front end that is still settling).  Its peaks sit ~4e-3 below those
# of the second sync symbol, so where the planted trial FAILS its gate the whole first symbol fails with it and the first trial of
# the second sync symbol decides, clear of every planted gate.
FIRST_SYMBOL_NOISE = 2.5
N_LEN, N_GAP = 8, 8                                          # burst lengths x quiet gaps
OFFSET_PHASE = np.exp(0.7j)
# seed of the base frame per N, chosen on the CPU so that no trial from the hit on other than the planted and the deciding one
# comes within 1e-4 of any planted gate (asserted in test_sync_hostile_ref_host.py)
BASE_SEED = {64: 0, 256: 0, 512: 0, 1024: 0, 2048: 0, 4096: 0}

Batch = namedtuple("Batch", "N cp Kd n_sym_tx kind iq leads blen gap level hit")


# ------------------------------------------------------------------------------------------ the kernel's geometry, restated
def scan_block(N, cp):
    """csrc/rx_sync_scan.hpp: scan_block_n -- trials per anchor of the screened search (Ks = N - 2, pattern (1, 3))"""
    P = 8 if N == 64 else 16
    T = N // P
    QM = 2 if T >= 256 else 3 if T >= 128 else 4 if T >= 64 else 6 if T >= 32 else min(P, 12)
    B = min(QM * T - cp, min(QM * T, 256))
    return B if B >= 16 else 0


GUARD_NW, GUARD_E = 1e-4, 1e-3                               # rx_sync_scan.hpp: nwj > 1e-4 wbound, ej > 1e-3 nwj


def anchor_of(hit, B):
    """the anchor of the block that screens trial `hit` in a search that nothing disturbed before: anchors at 0, B, 2 B, ..."""
    return (int(hit) // B) * B


def guard_weak(x, N, cp, P0, j, B):
    """The two fixed guard ratios of the screen, restated in fp64: is trial P0 + j of the block anchored at P0 "weak", i.e.
    handed to the exact evaluation without a look at the recurrence?  (The block's own B trials; the long block of the cold
    test only ever lowers the first ratio.)"""
    x = np.asarray(x, np.complex128)
    n = np.arange(N)

    def sums(P):
        w = x[P + cp:P + cp + N]
        nw = N * np.sum(np.abs(w) ** 2)
        return nw, nw - abs(np.sum(w)) ** 2 - abs(np.sum(w * (-1.0) ** n)) ** 2
    nw0, _ = sums(P0)
    wbound = nw0 + N * np.sum(np.abs(x[P0 + cp + N:P0 + cp + N + B - 1]) ** 2)
    nwj, ej = sums(P0 + j)
    return not (nwj > GUARD_NW * wbound) or not (ej > GUARD_E * nwj)


# ------------------------------------------------------------------------------------------ the oracle's trial, many at once
def peaks(x, N, cp, trials):
    """fp64 peak and lag of RxOracle.sync_trial (Ks = N - 2, one sync symbol) at each trial of `trials`: the same sums, with
    the cp + 1 lag correlations taken from one inverse FFT (pinned to sync_trial itself in test_sync_hostile_ref_host.py).
    -> (m [n] float64, lag [n] int)"""
    trials = np.asarray(trials, np.int64)
    Ks = N - 2
    bins = orc.bins_p(Ks, N)
    zc = np.conj(orc.zadoff_chu(Ks, 23))
    x = np.asarray(x, np.complex128)
    m = np.zeros(len(trials))
    lag = np.zeros(len(trials), np.int64)
    win = np.lib.stride_tricks.sliding_window_view(x, N)
    step = max(1, (1 << 18) // N)

    def chunk(s):
        t = trials[s:s + step]
        y = np.fft.fft(win[t + cp], axis=1)[:, bins]
        p_est = np.sqrt(Ks / np.sum(np.abs(y) ** 2, axis=1))
        Z = np.zeros((len(t), N), complex)
        Z[:, bins] = y * zc
        c = np.abs(np.fft.ifft(Z, axis=1)[:, :cp + 1]) * N * p_est[:, None]
        lag[s:s + step] = np.argmax(c, axis=1)
        m[s:s + step] = np.max(c, axis=1)
    starts = range(0, len(trials), step)
    if len(starts) > 2:                                      # (NumPy's FFT releases the interpreter lock)
        with ThreadPoolExecutor(4) as pool:
            list(pool.map(chunk, starts))
    else:
        for s in starts:
            chunk(s)
    return m, lag


# ------------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def base(N):
    """-> (bits, samples [fl] complex128: channel output plus the frame's noise, from the frame start on); read-only"""
    cp, Kd, n_sym = SIZES[N]
    n_sym_tx = n_sym + 4
    fl = n_sym_tx * (N + cp) + 7
    rng = np.random.default_rng(9000 + 16 * N + BASE_SEED[N])
    bits = rng.integers(0, 2, (n_sym_tx // 4) * 3 * Kd * 2).astype(np.uint8)
    tx = orc.channel_apply(orc.tx_modulate(bits, N, cp, N - 2, Kd, n_sym_tx), orc.REF_TAPS, N)[:fl]
    env = np.where(np.arange(fl) < N + cp, FIRST_SYMBOL_NOISE, 1.0)
    y = tx + SIGMA * env * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))
    bits.setflags(write=False)
    y.setflags(write=False)
    return bits, y


def _cnoise(rng, n, rms):
    return rms * np.sqrt(0.5) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def _shape(N, cp):
    """the N_LEN x N_GAP burst shapes: lengths cp + 1 .. cp + B, so the burst leaves the window at trial 1 .. B of a search that
    starts at the buffer's first sample (anchors at 0, B, ...), and per length gaps from 0 to what is left of that block -- the
    hit follows in the block the burst left, at every phase -- and one gap of B - 1, into the next block"""
    B = scan_block(N, cp)
    n_gap = N_GAP
    ex = np.round(np.linspace(1, B, N_LEN)).astype(int)
    bl, gp = [], []
    for e in ex:
        room = max(B - 2 - e, 0)                             # hit = e + gap + 1 <= B - 1
        g = np.unique(np.round(np.linspace(0, room, n_gap - 1)).astype(int)).tolist()
        g += [B - 1] * (n_gap - len(g))
        bl += [cp + e] * n_gap
        gp += g
    return np.array(bl), np.array(gp)


@functools.lru_cache(maxsize=None)
def batch(N, kind):
    """-> Batch of N_LEN * N_GAP frames (the kinds without a burst shape at N >= 2048: half as many, the oracle's trials cost
    N log N each) [n][fl] complex64; read-only.  level[f]: the burst's dB / the offset's amplitude / the
    gain of frame f (0 where the kind has none); hit[f] = leads[f] - cp + 1, the planted trial."""
    cp, Kd, n_sym = SIZES[N]
    n_sym_tx = n_sym + 4
    fl = n_sym_tx * (N + cp) + 7
    B = scan_block(N, cp)
    _, y = base(N)
    rng = np.random.default_rng(9100 + 16 * N + KINDS.index(kind))
    blen, gap = _shape(N, cp)
    nf = len(blen)
    level = np.zeros(nf)
    if kind in ("burst", "fall"):
        leads = blen + gap
    else:
        # leads spread over cp .. cp + B + 7: the hit at every phase of the first block, at the second anchor and just behind it
        nf = nf if N < 2048 else nf // 2
        leads = cp + np.round(np.linspace(0, B + 7, nf)).astype(int)
        blen, gap, level = np.zeros(nf, int), np.zeros(nf, int), np.zeros(nf)
    iq = np.zeros((nf, fl), np.complex64)
    sgn = (-1.0) ** np.arange(fl)
    for f in range(nf):
        ld = int(leads[f])
        if kind == "burst":
            level[f] = BURST_DB[(f // N_GAP + f % N_GAP) % len(BURST_DB)]        # every level meets every length and gap class
            pre = np.concatenate([_cnoise(rng, blen[f], 10 ** (level[f] / 20)), _cnoise(rng, gap[f], SIGMA * np.sqrt(2))])
        elif kind == "fall":
            pre = _cnoise(rng, ld, SIGMA * np.sqrt(2))
            z = f % 4
            if z:
                pre[ld - z:] = 0
        else:
            pre = _cnoise(rng, ld, 1.0)
        x = np.concatenate([pre, y])[:fl]
        if kind == "dc":
            level[f] = OFFSETS[f % len(OFFSETS)]
            x = x + level[f] * OFFSET_PHASE
        elif kind == "nyq":
            level[f] = OFFSETS[f % len(OFFSETS)]
            x = x + level[f] * OFFSET_PHASE * sgn
        elif kind == "gain":
            level[f] = GAINS[f % len(GAINS)]
            x = x * level[f]
        iq[f] = x.astype(np.complex64)
    out = Batch(N, cp, Kd, n_sym_tx, kind, iq, leads, blen, gap, level, leads - cp + 1)
    for a in out[5:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tail(N, full=False):
    """-> (m, lag) of the oracle's trials hit .. hit + 4 L + cp on the base frame as the engine receives it (complex64): the
    windows that hold no lead sample, one profile for every frame of every batch.  Unless `full`, the trials hit + cp + 2 ..
    hit + 4 L - 2 -- windows over the data symbols, which test_sync_hostile_ref_host.py pins far below every gate on the full
    profile -- are not evaluated and read 0.  (The offset kinds share it: DC and Nyquist
    are not among the Ks = N - 2 bins and a gain cancels in the normalisation; what the complex64 rounding of the shifted
    samples moves is bounded in test_sync_hostile_ref_host.py.)  read-only"""
    cp = SIZES[N][0]
    _, y = base(N)
    x = np.concatenate([np.zeros(cp), y]).astype(np.complex64)             # a lead of cp samples puts the planted trial at 1
    n = 4 * (N + cp) + cp + 1
    k = np.arange(n) if full else np.concatenate([np.arange(cp + 2), np.arange(4 * (N + cp) - 1, n)])
    m, lag = np.zeros(n), np.zeros(n, np.int64)
    m[k], lag[k] = peaks(x, N, cp, 1 + k)
    assert lag[0] == cp
    m.setflags(write=False)
    lag.setflags(write=False)
    return m, lag


def planted(N, passing):
    """-> k: the planted trial is hit + k.  Passing: the first acceptable trial itself.  Failing: the trial of the first sync
    symbol with the largest peak (hit .. hit + cp all see the same symbol), so that the whole symbol fails with it."""
    cp = SIZES[N][0]
    return 0 if passing else int(np.argmax(tail(N)[0][:cp + 1]))


def gate(N, d, passing):
    """scale_factor_gate that the planted trial passes (passing) or fails by d"""
    return tail(N)[0][planted(N, passing)] * (1 - d if passing else 1 + d) / (N - 2)


def tail_decision(N, d, passing, margin=1e-4):
    """-> (k, clean): the first trial hit + k from the hit on that passes gate(N, d, passing) (-1: none), and whether every
    trial before it other than the planted one misses the gate, and a later accepted one passes it, by more than `margin`"""
    mt, _ = tail(N)
    g = gate(N, d, passing) * (N - 2)
    acc = np.nonzero(mt > g)[0]
    if not len(acc):
        return -1, False
    k = int(acc[0])
    rel = mt[:k + 1] / g - 1
    return k, bool(not (np.abs(np.delete(rel, [planted(N, passing), k])) <= margin).any() and (k == 0 or rel[k] > margin))


@functools.lru_cache(maxsize=None)
def lead_profile(N, kind):
    """-> per frame (m, lag) of the oracle's trials 0 .. hit - 1, the windows that hold lead samples; read-only"""
    b = batch(N, kind)
    out = []
    for f in range(len(b.iq)):
        m, lag = peaks(b.iq[f], N, b.cp, np.arange(int(b.hit[f])))
        m.setflags(write=False)
        lag.setflags(write=False)
        out.append((m, lag))
    return out


def expected(N, kind, d, passing, margin=1e-4):
    """-> (trial [n], lag [n], peak [n], clean [n] bool): the oracle's first accepted trial of every frame under gate(N, d,
    passing) (-1: none up to hit + 4 L + cp), and whether the frame is CLEAN: the planted trial misses or passes the gate by d
    (it does by construction), an accepted later trial passes by more than `margin` relative, and every other trial up to the
    accepted one misses the gate by more than `margin`."""
    b = batch(N, kind)
    mt, lt = tail(N)
    g = gate(N, d, passing) * (N - 2)
    nf = len(b.iq)
    trial, lag, peak, clean = np.full(nf, -1), np.zeros(nf, int), np.zeros(nf), np.zeros(nf, bool)
    k, tail_clean = tail_decision(N, d, passing, margin)
    for f, (m, lg) in enumerate(lead_profile(N, kind)):
        hit = int(b.hit[f])
        acc = np.nonzero(m > g)[0]
        if len(acc):
            trial[f], lag[f], peak[f] = acc[0], lg[acc[0]], m[acc[0]]
            continue                                                         # a lead trial that passes: never clean
        if k >= 0:
            trial[f], lag[f], peak[f] = hit + k, lt[k], mt[k]
        clean[f] = tail_clean and not (np.abs(m / g - 1) <= margin).any()
    return trial, lag, peak, clean
