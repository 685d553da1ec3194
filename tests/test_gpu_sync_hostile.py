"""The screened sync search held to the exhaustive one and to the fp64 oracle on hostile leads with the accept decision made
marginal on purpose (run with -m gpu).

tests/sync_hostile_cases.py builds the frames: a noise burst 30 .. 42 dB above the signal that leaves the window inside a
screening block, a DC or alternating offset of up to 25 times the signal rms, the whole buffer scaled by 1e-4 or 1e4, a quiet lead
that ends in exact zeros, and a control lead of the signal's own level -- in front of ONE base frame per size, with the engine's
gate planted d = 1e-4, 3e-4 or 1e-3 below (the hit passes) or above (the first sync symbol fails, the second decides) the oracle's
peak.  tests/test_sync_hostile_ref_host.py pins on the oracle alone that every other trial stays more than 1e-4 clear of the
gate, so the exact trial functions (2e-6 apart, a few 1e-6 from fp64) take the oracle's decision and the screen, whose thresholds
sit 2e-4 below the gate, has to hand them every trial that matters: `time_synch_ref`, bits and finite patterns equal between the
two searches, arrays to 2e-6, position and lag the oracle's.  Each test prints one line per lead kind: frames, how many of them
the screen's own guard ratios call weak at the planted trial (those take the exact fallback), the worst error between the
searches."""
import numpy as np
import pytest

import sync_hostile_cases as hc
from conftest import poisoned, relerr
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 2e-6                                                   # between the two searches (tests/test_gpu_sync_scan.py)
WORK_MACS = 2e7                                              # a sampled frame gets the oracle's full search below this cost


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


def _run(om, rx, d_iq, n_frames, fl, Kd, exhaustive):
    assert rx.set_sync_search(exhaustive) == (not exhaustive)
    nds = rx.data_symbols_per_frame(fl)
    d_eq = poisoned(om, n_frames * nds * Kd * 8)             # 0xFF: a row the kernels do not write cannot pass as zeros
    d_b = poisoned(om, n_frames * nds * Kd * 2)
    d_tsr = poisoned(om, n_frames * 16)
    rx.demod_frames(d_iq, n_frames, fl, fl, d_eq, d_b, om.BITS_UNPACKED, d_tsr)
    eq = d_eq.download(np.complex64, n_frames * nds * Kd).reshape(n_frames, nds, Kd)
    b = d_b.download(np.uint8, n_frames * nds * Kd * 2).reshape(n_frames, -1)
    tsr = d_tsr.download(np.int32, n_frames * 4).reshape(n_frames, 4)
    H = np.stack([rx.frame_state(f)["chan_freq"] for f in range(n_frames)])
    return eq, b, tsr, H


def _weak_at_hit(b):
    B = hc.scan_block(b.N, b.cp)
    return np.array([hc.guard_weak(b.iq[f], b.N, b.cp, hc.anchor_of(b.hit[f], B), int(b.hit[f]) - hc.anchor_of(b.hit[f], B), B)
                     for f in range(len(b.iq))])


@pytest.mark.parametrize("N", (64, 512, 1024, 2048, 4096))
def test_batch_screen_takes_the_exhaustive_decisions_at_planted_gates(om, N):
    """T < 32 with several frames per workgroup (64), T = 32 (512), T = 64 with MX = 2 (1024), T = 128 with MX = 3 (2048),
    T = 256 with MX = 5 (4096): per lead kind, d and sign one screened and one exhaustive launch over the kind's 64 (or 32) frames."""
    cp, Kd, n_sym = hc.SIZES[N]
    n_sym_tx = n_sym + 4
    L = N + cp
    problems = []
    sync_cache = {}
    for kind in hc.KINDS:
        b = hc.batch(N, kind)
        nf, fl = b.iq.shape
        d_iq = om.DeviceBuffer(b.iq.nbytes).upload(b.iq)
        worst = 0.0
        rng = np.random.default_rng(N + hc.KINDS.index(kind))
        for d in hc.D_VALUES:
            for passing in (True, False):
                tag = (N, kind, d, "pass" if passing else "fail")
                g = hc.gate(N, d, passing)
                rx = om.RxEngine(n_sym_tx, N, cp, N - 2, (1, 3), Kd, 30, g)
                eq_s, b_s, tsr_s, H_s = _run(om, rx, d_iq, nf, fl, Kd, exhaustive=False)
                eq_x, b_x, tsr_x, H_x = _run(om, rx, d_iq, nf, fl, Kd, exhaustive=True)
                rx.close()
                # ---- screened against exhaustive: at every d, every kind
                if not np.array_equal(tsr_s, tsr_x):
                    bad = np.nonzero((tsr_s != tsr_x).any(axis=1))[0]
                    problems.append((tag, "tsr differs", [(int(f), int(b.hit[f]), float(b.level[f]), tsr_s[f].tolist(), tsr_x[f].tolist())
                                                          for f in bad[:6]], len(bad)))
                    continue
                if not np.array_equal(b_s, b_x):
                    problems.append((tag, "bits differ"))
                fin = np.isfinite(eq_x)
                if not np.array_equal(fin, np.isfinite(eq_s)):
                    problems.append((tag, "finite patterns differ"))
                    continue
                e_eq, e_h = relerr(np.where(fin, eq_s, 0), np.where(fin, eq_x, 0)), relerr(H_s, H_x)
                worst = max(worst, e_eq, e_h)
                if not (e_eq < TOL and e_h < TOL):
                    problems.append((tag, "arrays", e_eq, e_h))
                # ---- against the oracle
                trial, lag, peak, clean = hc.expected(N, kind, d, passing)
                if clean.sum() < nf - int(0.05 * nf):
                    problems.append((tag, "corpus: frames off their claim", np.nonzero(~clean)[0].tolist()))
                if not (tsr_s[:, 3].sum() == (trial >= 0).sum() > 0):      # (a batch in which nobody finds anything cannot pass)
                    problems.append((tag, "accepted", int(tsr_s[:, 3].sum()), int((trial >= 0).sum())))
                if kind in ("dc", "nyq") and d != 1e-3:
                    continue
                for f in np.nonzero(clean)[0]:
                    want = (trial[f] + cp, lag[f], int(peak[f]))
                    if not (tsr_s[f, 3] == 1 and tsr_s[f, 0] == want[0] and tsr_s[f, 1] == want[1] and abs(tsr_s[f, 2] - want[2]) <= 1):
                        problems.append((tag, "oracle", int(f), int(b.hit[f]), float(b.level[f]), tsr_s[f].tolist(), want))
                # the oracle itself: its full search on sampled frames where that is affordable, its trial function at the
                # accepted trial and the one before it on every other clean frame
                o = orc.RxOracle(n_sym_tx, N, cp, N - 2, [1, 3], Kd, 30, g, force_fp64=True)
                sampled = set(rng.choice(nf, 3, replace=False).tolist())
                for f in np.nonzero(clean)[0]:
                    if f in sampled and (trial[f] + 1) * (cp + 1) * (N - 2) < WORK_MACS:
                        o.corr_obs, o.count = -1, 0
                        o.time_synch_ref[:] = 0
                        with np.errstate(all="ignore"):                      # (rows past the buffer's end divide 0 by 0)
                            o.work(b.iq[f], np.zeros(fl, np.complex64))
                        got = (int(o.time_synch_ref[0]) - cp, int(o.time_synch_ref[1]), float(o.time_synch_ref[2]))
                        if not (got[0] == trial[f] and got[1] == lag[f] and got[2] == int(peak[f])):
                            problems.append((tag, "corpus against RxOracle.work", int(f), got, (trial[f], lag[f], peak[f])))
                    else:
                        for P in (int(trial[f]) - 1, int(trial[f])):
                            if (kind, f, P) not in sync_cache:
                                dm = np.abs(o.sync_trial(b.iq[f], P)[0])
                                sync_cache[kind, f, P] = (float(dm.max()), int(np.argmax(dm)))
                        (m0, _), (m1, l1) = sync_cache[kind, f, int(trial[f]) - 1], sync_cache[kind, f, int(trial[f])]
                        if not (m0 <= g * (N - 2) < m1 and l1 == lag[f] and abs(m1 / peak[f] - 1) < 2e-6):
                            problems.append((tag, "corpus against RxOracle.sync_trial", int(f), m0, m1, l1))
        print("sync-hostile batch N=%d %-7s frames %d  weak at the planted trial %d  worst |screened - exhaustive| %.2e" % (
            N, kind, nf, int(_weak_at_hit(b).sum()), worst))
        d_iq.free()
    for p in problems:
        print("PROBLEM", p)
    assert not problems, "%d problems, first: %r" % (len(problems), problems[0])


@pytest.mark.parametrize("passing", (True, False))
@pytest.mark.parametrize("N", (256, 2048))
def test_stream_block_screen_takes_the_exhaustive_decisions_at_planted_gates(om, N, passing):
    """`work()` on host buffers, the segmented instantiation of the screened search: two 38 dB burst buffers whose burst leaves
    the window in the block of the hit, then a control buffer, with the gate planted d = 3e-4 below the hit (passing) or above
    the first sync symbol's best trial (failing: the second sync symbol decides).  A screened and an exhaustive engine must
    leave the same report, `time_synch_ref` and output items, and state rows within 2e-6; the first call's position and lag
    are the oracle's."""
    cp, Kd, n_sym = hc.SIZES[N]
    n_sym_tx = n_sym + 4
    L = N + cp
    d = 3e-4
    B = hc.scan_block(N, cp)
    bb, bc = hc.batch(N, "burst"), hc.batch(N, "control")
    one_block = ((bb.blen - cp) // B == bb.hit // B) & (bb.level == 38.0) & ~_weak_at_hit(bb)
    picks = np.nonzero(one_block)[0]
    assert len(picks) >= 2
    bufs = [bb.iq[picks[0]], bb.iq[picks[-1]], bc.iq[len(bc.iq) // 2]]
    g = hc.gate(N, d, passing)
    scr = om.RxEngine(n_sym_tx, N, cp, N - 2, (1, 3), Kd, 100, g)
    exh = om.RxEngine(n_sym_tx, N, cp, N - 2, (1, 3), Kd, 100, g)
    assert scr.set_sync_search(False) is True and exh.set_sync_search(True) is False
    trial, lag, peak, clean = hc.expected(N, "burst", d, passing)
    assert clean[picks[0]]
    n_det = 0
    for i, x in enumerate(bufs):
        x = x[:n_sym_tx * L].copy()
        out_s, out_x = np.zeros(len(x), np.complex64), np.zeros(len(x), np.complex64)
        n_s, n_x = scr.work(x, out_s), exh.work(x, out_x)
        rs, rx_ = scr.report, exh.report
        assert n_s == n_x, (i, n_s, n_x)
        for fld in ("detected", "trials_run", "count", "corr_obs", "n_data_items"):
            assert getattr(rs, fld) == getattr(rx_, fld), (i, fld, getattr(rs, fld), getattr(rx_, fld))
        assert list(rs.time_synch_ref) == list(rx_.time_synch_ref), (i, list(rs.time_synch_ref), list(rx_.time_synch_ref))
        n_det += rs.detected
        if i == 0:
            f = picks[0]
            assert rs.detected == 1 and rs.time_synch_ref[0] == trial[f] + cp and rs.time_synch_ref[1] == lag[f]
            assert abs(rs.time_synch_ref[2] - int(peak[f])) <= 1
        if n_s > 0:
            assert np.array_equal(np.isfinite(out_s[:n_s]), np.isfinite(out_x[:n_s]))
            ok = np.isfinite(out_x[:n_s])
            assert relerr(out_s[:n_s][ok], out_x[:n_s][ok]) < TOL, i
        for row in (0, 1):
            a, c = scr.state(row), exh.state(row)
            for k in ("chan_freq", "chan_time", "synch_freq", "eq_gain"):
                assert relerr(a[k], c[k]) < TOL, (i, row, k)
    assert n_det >= 1
    print("sync-hostile stream N=%d %s: buffers %d, detected %d" % (N, "pass" if passing else "fail", len(bufs), n_det))
