"""Seeded frames for sync/data patterns other than [1, 3], and the fp64 oracle's rows for them (plain NumPy, no GPU).

The batch receiver demodulates n_pat = floor(floor(frame_len / L) / (S + D)) patterns of a frame and writes n_pat * D rows; row
p * D + n is the reference's est_data_freq[p * (S + D) + n].  `oracle_rows` reads exactly those rows from orc.RxOracle, whatever
the pattern: the oracle's work() ends with the reference's literal-row-3 delete and a reshape that raises for most patterns other
than [1, 3], but time_synch_ref and est_data_freq are complete by then.

A case is one numerology with one pattern and one constellation; `frames(case)` gives its few frames, one per row kind:

  aligned   a lead of three samples: every pattern fits the frame, every row is live
  guard     the lead moves the last pattern's pointer past the reference's once-per-pattern guard (SynchAndChanEst.py:223):
            that pattern keeps its zero rows
  tail      the last pattern passes the guard, one of its windows lies partly past the frame's end (np.fft.fft zero-pads it) and
            `r` further windows lie wholly past it (an all-zero window: 0 * inf = NaN rows)
  lag       a second small lead: the same trial wins with another lag

For S >= 2 the oracle synchronises only on a transmit signal that sends the ZC segment each sync symbol is correlated against
(tx_modulate(zc_segments=True)); it then applies the reference's pointer rule ptr_p = t0 + S*L*(p*(S+D) + 1), which is right
for pattern 0 only: pattern 1 reads misplaced (but well-defined) windows and later patterns fail the guard.  The leads of
those cases are chosen so that pattern 1 is whole, partly padded and partly past the end in turn.

The oracle searches trial by trial, so the leads are capped at the large sizes (LEAD_CAP): there the guard frame is left out where
it would need (D - 1) * L samples of lead, and the zero rows come from the (1, 1) and S >= 2 cases instead."""
import functools
from collections import namedtuple

import numpy as np

from oracle import ofdm_oracle as orc

# P: patterns the batch demodulates per frame (at least two for D = 13, at least four for S >= 2; n_dsym = P * D is no multiple of
#    the kernel's symbols per trip -- 8 / 4 / 2 at 64 / 256 / 512-pt -- in at least one case per size below 1024-pt)
# partial: frame_len additionally holds a trailing partial pattern of S + 1 symbols that the batch must ignore
# min_*: rows of each kind the case's frames must hold, summed over the frames; live counts the padded rows too (asserted on the
#    oracle alone by test_pattern_cases_host.py, so that the GPU test cannot pass vacuously)
Case = namedtuple("Case", "N cp Kd S D mod P partial min_live min_zero min_pad min_nan")

CASES = [
    Case(64, 16, 60, 1, 1, "BPSK", 9, False, 26, 1, 0, 0),
    Case(64, 16, 60, 1, 2, "QPSK", 5, True, 38, 2, 1, 0),
    Case(64, 16, 60, 1, 6, "16QAM", 3, True, 62, 6, 1, 4),
    Case(64, 16, 60, 1, 13, "QPSK", 3, False, 133, 13, 1, 10),
    Case(64, 16, 60, 2, 3, "QPSK", 4, False, 23, 24, 2, 1),
    Case(64, 16, 60, 3, 1, "16QAM", 4, False, 5, 7, 0, 0),
    Case(256, 18, 152, 1, 1, "16QAM", 7, False, 20, 1, 0, 0),
    Case(256, 18, 152, 1, 6, "QPSK", 3, True, 62, 6, 1, 4),
    Case(256, 18, 152, 1, 13, "BPSK", 2, False, 81, 13, 1, 10),
    Case(512, 36, 300, 1, 2, "16QAM", 3, False, 22, 2, 1, 0),
    Case(512, 36, 300, 1, 13, "QPSK", 3, False, 139, 13, 1, 4),
    Case(1024, 72, 600, 1, 1, "QPSK", 5, False, 14, 1, 0, 0),
    Case(1024, 72, 600, 1, 6, "16QAM", 2, False, 32, 0, 1, 4),
    Case(1024, 72, 600, 1, 13, "64QAM", 2, False, 74, 0, 1, 4),
    Case(1024, 72, 600, 2, 3, "QPSK", 4, False, 18, 18, 0, 0),
    Case(1024, 72, 604, 1, 6, "QPSK", 2, False, 32, 0, 1, 4),
    Case(2048, 144, 1200, 1, 1, "64QAM", 4, False, 11, 1, 0, 0),
    Case(2048, 144, 1200, 1, 6, "QPSK", 2, False, 34, 0, 1, 2),
    Case(4096, 288, 2400, 1, 6, "64QAM", 2, False, 24, 0, 1, 0),
]

# longest lead (samples) the oracle's trial-by-trial search is asked to walk through, per FFT size
LEAD_CAP = {64: 1 << 30, 256: 1 << 30, 512: 8000, 1024: 4600, 2048: 4600, 4096: 4400}
R_MAX = {64: 10, 256: 10}                  # windows wholly past the end in the tail frame; 4 elsewhere (fewer where the cap says so)
GATE = 0.7


def case_id(c):
    return "%d-%d-S%dD%d-%s" % (c.N, c.Kd, c.S, c.D, c.mod)


def snr_of(c):
    """The block's snr argument: 30 as in the suite's other tests; 100 (an all but unbiased MMSE equaliser) for the QAM cases, whose
    live rows must de-map to the sent bits."""
    return 100 if c.mod in ("16QAM", "64QAM") else 30


def sigma_of(c):
    return 0.01 if c.mod == "64QAM" else 0.02


def frame_len(c):
    L = c.N + c.cp
    return c.P * (c.S + c.D) * L + ((c.S + 1) * L if c.partial else 0) + 7


def leads(c):
    """[(kind, lead)] of the case's frames.  With t0 the accepted trial's time_synch_ref[0], lead <= t0 <= lead + cp."""
    L = c.N + c.cp
    extra = (c.S + 1) * L if c.partial else 0
    cap = LEAD_CAP[c.N]
    if c.S > 1:
        # pattern 1 points at t0 + S*L*(S+D+1): whole / its last window partly past the end / wholly past it, where that is a
        # different frame (D > 1) and the lead fits the cap; fl = P*(S+D)*L + 7
        out = [("aligned", 3)]
        if c.D > 1:
            past = frame_len(c) - 7 - c.S * L * (c.S + c.D + 1) - c.D * L      # lead - cp - 30 at which the last window ends at fl + 23
            for kind, ld in (("tail", past + c.cp + 30), ("tail", past + L + c.cp + 30)):
                if 0 < ld <= cap:
                    out.append((kind, ld))
        if len(out) == 1:
            out.append(("late", 2 * L + 11))       # pattern 1 whole, a lead of whole symbols
        return out + [("lag", c.cp // 2 + 5)]
    out = [("aligned", 3)]
    # guard of the last pattern: t0 + L*((P-1)*(1+D) + 1) + N - 1 <= fl fails iff t0 > (D-1)*L + cp + 8 + extra
    gf = (c.D - 1) * L + c.cp + 16 + extra
    if gf <= cap and c.N < 4096:
        out.append(("guard", gf))
    if c.D >= 2:
        # t0 = r*L + cp + 30 + extra + e, 0 <= e <= cp: window D-r-1 of the last pattern ends 23 + e samples past the end, windows
        # D-r .. D-1 start past it
        r = min(c.D - 2, R_MAX.get(c.N, 4))
        while r > 0 and r * L + c.cp + 30 + extra > cap:
            r -= 1
        out.append(("tail", r * L + c.cp + 30 + extra))
    if c.N < 4096:
        out.append(("lag", c.cp // 2 + 5))
    return out


def make_frame(c, lead, rng):
    """One frame of the case: `lead` samples of noise, then P patterns through REF_TAPS, cut or zero-filled to frame_len(c), mild
    noise on top.  -> (iq [frame_len] complex64, bits [P*D][Kd*bps])"""
    bps = orc.BITS_PER_SYMBOL[c.mod]
    fl = frame_len(c)
    sigma = sigma_of(c)
    b = rng.integers(0, 2, c.P * c.D * c.Kd * bps).astype(np.uint8)
    tx = orc.tx_modulate(b, c.N, c.cp, c.N - 2, c.Kd, c.P * (c.S + c.D), synch_dat=(c.S, c.D), modulation=c.mod, zc_segments=c.S > 1)
    tx = orc.channel_apply(tx, orc.REF_TAPS, c.N)
    pre = 0.3 * (rng.standard_normal(lead) + 1j * rng.standard_normal(lead))
    x = np.concatenate([pre, tx])[:fl]
    x = np.concatenate([x, np.zeros(fl - len(x))])
    iq = (x + sigma * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    return iq, b.reshape(c.P * c.D, c.Kd * bps)


@functools.lru_cache(maxsize=None)
def _build(c):
    rng = np.random.default_rng(c.N * 1000 + c.Kd + 37 * c.S + c.D)
    made = [make_frame(c, lead, rng) for _, lead in leads(c)]
    iq = np.stack([x for x, _ in made])
    iq.setflags(write=False)
    return iq, tuple(b for _, b in made)


def frames(c):
    """[n_frames][frame_len] complex64, read-only: one frame per entry of leads(c), each through REF_TAPS with mild noise."""
    return _build(c)[0]


def sent_bits(c):
    """per frame: [P*D][Kd*bps] the bits of the transmitted data symbols, in transmit order"""
    return _build(c)[1]


def oracle_rows(iq, N, cp, Ks, S, D, Kd, snr, gate):
    """One frame through the fp64 oracle -> (time_synch_ref[3], rows [n_pat*D][Kd] complex128): row p*D + n is
    est_data_freq[p*(S+D) + n].  time_synch_ref[2] = int(peak) is positive iff a trial was accepted."""
    iq = np.asarray(iq)
    fl, L, SD = len(iq), N + cp, S + D
    n_pat = fl // L // SD
    # one pattern more than the batch demodulates: the oracle's loop also visits a trailing partial pattern
    o = orc.RxOracle((n_pat + 1) * SD, N, cp, Ks, [S, D], Kd, snr, gate, force_fp64=True)
    with np.errstate(all="ignore"):
        try:
            o.work(iq, np.zeros(fl, np.complex64))
        except (ValueError, IndexError):          # the literal-row-3 delete and the reshape behind it (SynchAndChanEst.py:249-255)
            pass
    keep = [p * SD + n for p in range(n_pat) for n in range(D)]
    return np.array(o.time_synch_ref, dtype=np.float64), o.est_data_freq[keep].copy()


@functools.lru_cache(maxsize=None)
def reference(c):
    """per frame (tsr[3], rows), computed once per process and read-only"""
    out = []
    for x in frames(c):
        tsr, rows = oracle_rows(x, c.N, c.cp, c.N - 2, c.S, c.D, c.Kd, snr_of(c), GATE)
        tsr.setflags(write=False)
        rows.setflags(write=False)
        out.append((tsr, rows))
    return tuple(out)


def row_kinds(c, tsr, rows):
    """-> boolean [n_pat*D] arrays (nan, zero, padded, live) of one frame's oracle rows.  `padded` is the subset of `live` whose
    window, placed by the reference's pointer rule, reaches past the frame's end."""
    L, SD, fl = c.N + c.cp, c.S + c.D, frame_len(c)
    nan = ~np.isfinite(rows).all(axis=1)
    zero = ~nan & ~rows.any(axis=1)
    live = ~nan & ~zero
    r = np.arange(len(rows))
    start = int(tsr[0]) + c.S * L * ((r // c.D) * SD + 1) + L * (r % c.D)
    padded = live & (start + c.N > fl)
    return nan, zero, padded, live
