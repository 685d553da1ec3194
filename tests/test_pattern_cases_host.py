"""The cases of tests/pattern_cases.py are what they claim, shown on the fp64 oracle alone (CPU): test_gpu_patterns.py compares the
batch receiver with these rows, and must not be able to pass because a frame holds no row of the kind it is there for."""
import numpy as np
import pytest

import pattern_cases as pc
from oracle import ofdm_oracle as orc

IDS = [pc.case_id(c) for c in pc.CASES]
NS = {64: 8, 128: 8, 256: 4, 512: 2, 1024: 1, 2048: 1, 4096: 1}      # symbols per trip of the demod kernel (DemodGeom<N>::NS)


def test_case_list_covers_what_it_must():
    have = {(c.N, c.cp, c.Kd, (c.S, c.D)) for c in pc.CASES}
    need = ([(64, 16, 60, p) for p in ((1, 1), (1, 2), (1, 6), (1, 13), (2, 3), (3, 1))] +
            [(256, 18, 152, p) for p in ((1, 1), (1, 6), (1, 13))] + [(512, 36, 300, p) for p in ((1, 2), (1, 13))] +
            [(1024, 72, 600, p) for p in ((1, 1), (1, 6), (1, 13), (2, 3))] + [(1024, 72, 604, (1, 6))] +
            [(2048, 144, 1200, p) for p in ((1, 1), (1, 6))] + [(4096, 288, 2400, (1, 6))])
    assert not set(need) - have
    assert len(set(IDS)) == len(IDS)
    assert {c.mod for c in pc.CASES} == {"BPSK", "QPSK", "16QAM", "64QAM"}
    assert not any((c.S, c.D) == (1, 3) for c in pc.CASES)
    for N in (64, 256, 512):
        assert any(c.N == N and (c.P * c.D) % NS[N] for c in pc.CASES), "%d-pt: every n_dsym is a multiple of the trip" % N
        assert any(c.N == N and NS[N] % c.D for c in pc.CASES) and any(c.N == N and c.D > NS[N] for c in pc.CASES)
    assert any(c.partial for c in pc.CASES)
    for c in pc.CASES:
        L = c.N + c.cp
        fl = pc.frame_len(c)
        assert fl % L == 7 and fl // L // (c.S + c.D) == c.P, "frame_len: whole patterns (+ the partial one) + 7 samples"
        assert (fl // L) % (c.S + c.D) == (c.S + 1 if c.partial else 0)
        assert c.P >= (4 if c.S > 1 else 2 if c.D == 13 else 1)
        assert 2 <= len(pc.leads(c)) <= 5 and len(pc.frames(c)) == len(pc.leads(c))
        assert len({ld for _, ld in pc.leads(c)}) == len(pc.leads(c))
        assert pc.frames(c).dtype == np.complex64 and pc.frames(c).shape[1] == fl
        assert max(ld for _, ld in pc.leads(c)) <= pc.LEAD_CAP[c.N]


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_case_holds_the_rows_it_declares(c):
    ref = pc.reference(c)
    bits = pc.sent_bits(c)
    tot = np.zeros(4, int)
    lags = set()
    wrong_later = 0                             # S >= 2: whole rows of later patterns, all of them misplaced
    for f, ((kind, lead), (tsr, rows)) in enumerate(zip(pc.leads(c), ref)):
        assert rows.shape == (c.P * c.D, c.Kd)
        assert tsr[2] > 0, "frame %d (%s): no sync" % (f, kind)
        assert lead <= tsr[0] <= lead + c.cp, (f, kind, lead, tsr)
        lags.add((int(tsr[0]), int(tsr[1])))
        nan, zero, padded, live = pc.row_kinds(c, tsr, rows)
        tot += [live.sum(), zero.sum(), padded.sum(), nan.sum()]
        pat = np.arange(len(rows)) // c.D
        if c.S == 1:
            # the frame is of its kind
            if kind in ("aligned", "lag"):
                assert live.all() and not padded.any(), (f, kind)
            if kind == "guard":
                assert zero[pat == c.P - 1].all() and live[pat < c.P - 1].all(), (f, kind)
            if kind == "tail":
                assert live[pat < c.P - 1].all() and live[c.D * (c.P - 1)] and padded.sum() == 1, (f, kind)
                assert nan.sum() >= (2 if c.D >= 6 and c.N < 4096 else 0), (f, kind)
            ok = live & ~padded
        else:
            ok = pat == 0                       # the reference's pointer rule is right for pattern 0 only
            assert live[ok].all() and not padded[ok].any()
            later = np.nonzero(live & ~padded & (pat > 0))[0]
            right = [r for r in later if np.array_equal(orc.demap_hard(rows[r], c.mod), bits[f][r])]
            assert not right, "frame %d: rows %s of a later pattern de-map to their sent bits -- not the reference's pointer rule" % (f, right)
            wrong_later += len(later)
            assert zero[pat >= 2].all() and zero.any(), "frame %d: patterns 2.. must fail the guard" % f
        got = orc.demap_hard(rows[ok].ravel(), c.mod).reshape(int(ok.sum()), -1)
        assert np.array_equal(got, bits[f][ok]), "frame %d (%s): live rows do not de-map to the sent bits" % (f, kind)
    assert tuple(tot) == (c.min_live, c.min_zero, c.min_pad, c.min_nan), tot
    assert len(lags) == len(ref), "two frames share (t0, lag)"
    assert c.S == 1 or wrong_later >= 1, "no later pattern with whole, misplaced windows"


def test_wrapper_on_the_reference_pattern():
    """[1, 3]: the rows oracle_rows returns are the o.est_data_freq[rows] the suite's other tests read (rows 3, 7, .. dropped)."""
    N, cp, Kd, n_sym = 64, 16, 60, 12
    L = N + cp
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 9 * Kd * 2).astype(np.uint8)
    tx = orc.channel_apply(orc.tx_modulate(bits, N, cp, N - 2, Kd, n_sym), orc.REF_TAPS, N)
    fl = n_sym * L + 7
    lead = 2 * L + cp + 16                      # the last pattern fails the guard: zero rows are compared too
    x = np.concatenate([0.3 * (rng.standard_normal(lead) + 1j * rng.standard_normal(lead)), tx])[:fl]
    iq = (x + 0.02 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    o = orc.RxOracle(n_sym, N, cp, N - 2, [1, 3], Kd, 30, 0.7, force_fp64=True)
    o.work(iq, np.zeros(fl, np.complex64))
    keep = [r for r in range(n_sym) if r % 4 != 3]
    tsr, rows = pc.oracle_rows(iq, N, cp, N - 2, 1, 3, Kd, 30, 0.7)
    assert np.array_equal(tsr, o.time_synch_ref)
    assert np.array_equal(rows, o.est_data_freq[keep])
    assert rows[:6].any(axis=1).all() and not rows[6:].any()
