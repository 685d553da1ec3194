"""tests/sync_hostile_cases.py, the corpus of tests/test_gpu_sync_hostile.py, held to what it claims on the fp64 oracle alone (no
GPU): where the planted trial sits, that it passes or misses its gate by d while every other trial stays clear of the gate, that
the vectorised trial evaluation is RxOracle.sync_trial, and that the strong bursts really reach the screen's recurrence instead
of its exact fallback."""
import numpy as np
import pytest

import sync_hostile_cases as hc
from oracle import ofdm_oracle as orc

CAP = 0.05                                                   # share of a batch that may miss its claim on the reference alone
HOST_SIZES = (64, 256, 512)                                  # lead trials frame by frame (the larger sizes: in the GPU test)


def _oracle(N, g=0.7):
    cp, Kd, n_sym = hc.SIZES[N]
    return orc.RxOracle(n_sym + 4, N, cp, N - 2, [1, 3], Kd, 30, g, force_fp64=True)


def test_block_length_is_the_kernels():
    """scan_block_n of csrc/rx_sync_scan.hpp at the sizes of the corpus"""
    assert [hc.scan_block(N, hc.SIZES[N][0]) for N in (64, 256, 512, 1024, 2048, 4096)] == [48, 128, 156, 184, 240, 224]
    assert hc.scan_block(64, 60) == 0                        # cp too long for one block


@pytest.mark.parametrize("N", (64, 256))
def test_vectorised_trials_are_sync_trial(N):
    cp = hc.SIZES[N][0]
    o = _oracle(N)
    for kind in ("burst", "dc"):
        b = hc.batch(N, kind)
        for f in (0, 17, len(b.iq) - 1):
            tr = np.unique(np.concatenate([np.arange(0, int(b.hit[f]) + cp + 1, 7), [int(b.hit[f]) - 1, int(b.hit[f])]]))
            m, lag = hc.peaks(b.iq[f], N, cp, tr)
            for i, P in enumerate(tr):
                dm = np.abs(o.sync_trial(b.iq[f], int(P))[0])
                assert abs(m[i] - dm.max()) <= 1e-10 * dm.max() and lag[i] == int(np.argmax(dm)), (kind, f, P)


@pytest.mark.parametrize("N", sorted(hc.SIZES))
def test_base_frame_leaves_every_planted_gate_one_clean_decision(N):
    """From the hit on every frame of every batch sees the same windows.  Passing gates: the hit decides.  Failing gates: the
    whole first sync symbol fails, the planted trial by d and the rest by more than 1e-4, the data symbols stay far below, and
    the first trial of the second sync symbol passes by more than 1e-4."""
    cp = hc.SIZES[N][0]
    L = N + cp
    mt, lt = hc.tail(N, full=True)
    ms, ls = hc.tail(N)
    part = ms > 0
    assert lt[0] == cp and part.sum() == 2 * cp + 4 and np.array_equal(ms[part], mt[part]) and np.array_equal(ls[part], lt[part])
    for d in hc.D_VALUES:
        assert hc.tail_decision(N, d, True) == (0, True)
        assert hc.tail_decision(N, d, False) == (4 * L, True) and lt[4 * L] == cp
        g = hc.gate(N, d, False) * (N - 2)
        assert abs(g / mt[hc.planted(N, False)] - 1 - d) < 1e-12 and (mt[cp + 1:4 * L] < 0.6 * g).all()
        assert abs(hc.gate(N, d, True) * (N - 2) / mt[0] - 1 + d) < 1e-12


@pytest.mark.parametrize("N", HOST_SIZES)
@pytest.mark.parametrize("kind", hc.KINDS)
def test_every_batch_sits_where_it_claims(N, kind):
    cp = hc.SIZES[N][0]
    b = hc.batch(N, kind)
    nf = len(b.iq)
    assert nf == hc.N_LEN * hc.N_GAP <= 64 and len(hc.batch(2048, kind).iq) in (nf, nf // 2) and (b.hit == b.leads - cp + 1).all() and b.hit.min() >= 1
    # the frames differ in their leads only: from the frame start on they hold the same samples (the offset kinds: per level
    # and, for the alternating offset, per parity of the lead)
    for f in range(1, nf):
        same = [g for g in range(f) if b.level[g] == b.level[f] and (kind != "nyq" or (b.leads[g] - b.leads[f]) % 2 == 0)]
        if same:
            n = b.iq.shape[1] - int(max(b.leads[f], b.leads[same[0]]))
            assert np.array_equal(b.iq[f, b.leads[f]:b.leads[f] + n], b.iq[same[0], b.leads[same[0]]:b.leads[same[0]] + n])
    # ... and the shared profile of those windows is each frame's own, on sync_trial itself: the planted trials
    o = _oracle(N)
    mt, lt = hc.tail(N)
    for f in range(nf):
        for k in (0, hc.planted(N, False)):
            dm = np.abs(o.sync_trial(b.iq[f], int(b.hit[f]) + k)[0])
            assert abs(dm.max() / mt[k] - 1) < 2e-6 and int(np.argmax(dm)) == lt[k], (f, k)
    for d in hc.D_VALUES:
        for passing in (True, False):
            trial, lag, peak, clean = hc.expected(N, kind, d, passing)
            assert (trial >= 0).all() and clean.sum() >= nf - int(CAP * nf), (d, passing, np.nonzero(~clean)[0])
            k = 0 if passing else 4 * (N + cp)
            assert (trial[clean] == b.hit[clean] + k).all() and (lag[clean] == cp).all()


@pytest.mark.parametrize("N", HOST_SIZES)
def test_burst_frames_have_the_shape_the_screen_is_held_against(N):
    """The hit is blen - cp + gap + 1; before it no trial comes near the gate (the window holds burst samples, or sees the
    channel's first tap only); for some frames of every level the burst leaves the window and the hit follows inside ONE
    screening block; and by the kernel's own two guard ratios most frames of 34 dB and more are not "weak" at the hit, so
    the screen, not its exact fallback, takes the decision there."""
    cp = hc.SIZES[N][0]
    B = hc.scan_block(N, cp)
    b = hc.batch(N, "burst")
    assert (b.hit == b.blen - cp + b.gap + 1).all()
    assert b.blen.min() == cp + 1 and b.blen.max() == cp + B and b.gap.min() == 0 and b.gap.max() == B - 1
    assert len(set(zip(b.blen.tolist(), b.gap.tolist()))) >= len(b.iq) - 8       # (the longest bursts leave no room for eight gaps)
    g = hc.gate(N, 1e-3, True) * (N - 2)
    for m, _ in hc.lead_profile(N, "burst"):
        assert (m <= 0.6 * g).all()
    one_block = (b.blen - cp) // B == b.hit // B              # burst exit and hit behind the same anchor
    weak = np.array([hc.guard_weak(b.iq[f], N, cp, hc.anchor_of(b.hit[f], B), int(b.hit[f]) - hc.anchor_of(b.hit[f], B), B)
                     for f in range(len(b.iq))])
    for db in hc.BURST_DB:
        sel = b.level == db
        assert sel.sum() == len(b.iq) // len(hc.BURST_DB) and (one_block & sel).sum() >= 8, db
    strong = b.level >= 34
    assert (~weak & strong).sum() * 2 >= strong.sum()
    assert (~weak & strong & one_block).sum() >= 20          # ... and among them frames whose block starts inside the burst


def test_guard_ratios_fire_where_the_kernel_says():
    """a window of exact zeros and a window that is all offset are weak; a plain signal window is not"""
    N, cp = 256, 64
    B = hc.scan_block(N, cp)
    x = np.array(hc.base(N)[1][:4 * N])
    assert not hc.guard_weak(x, N, cp, 0, 5, B)
    assert hc.guard_weak(np.concatenate([1e3 * x[:cp + 20], np.zeros(3 * N)]), N, cp, 0, 30, B)
    assert hc.guard_weak(x + 40.0, N, cp, 0, 5, B) and not hc.guard_weak(x + 25.0, N, cp, 0, 5, B)
