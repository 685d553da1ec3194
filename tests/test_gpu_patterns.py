"""The frame-batched receiver on sync/data patterns other than [1, 3] (run with -m gpu).

ofdm_rx_demod_frames is written for any synch_dat = [S, D]; the rest of the GPU suite runs its demod kernel on (1, 3) only.  Here
the cases of tests/pattern_cases.py -- (1, 1), (1, 2), (1, 6), (1, 13), (2, 3), (3, 1) over the FFT sizes, with aligned, guard-failed,
zero-padded and NaN rows shown to be present by test_pattern_cases_host.py -- are held against the fp64 oracle row for row with the
suite's own assert_close, then the same frames are run in the launcher's other chunk regimes (a chunk of several trips below
1024-pt, the work queue from 1024-pt up), through every composite call, and end to end on the device.

For S >= 2 kernel and oracle both restate the reference's pointer rule ptr_p = t0 + S*L*(p*(S+D) + 1): pattern 0 decodes, pattern
1 reads misplaced windows, later patterns fail the guard -- garbage rows included, the two must agree."""
import numpy as np
import pytest

import pattern_cases as pc
import pilot_ref as pr
from conftest import assert_close, poisoned, relerr
from oracle import ofdm_oracle as orc
from test_gpu_demod_kd_paths import QUEUE_FRAMES

pytestmark = pytest.mark.gpu

IDS = [pc.case_id(c) for c in pc.CASES]
NS = {64: 8, 256: 4, 512: 2, 1024: 1, 2048: 1, 4096: 1}              # symbols per trip of the demod kernel (DemodGeom<N>::NS)
POISON32 = np.uint32(0xFFFFFFFF)


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def cur(torch):
    return torch.cuda.current_stream().cuda_stream


def engine(om, c, mod=None):
    rx = om.RxEngine(c.P * (c.S + c.D), c.N, c.cp, c.N - 2, (c.S, c.D), c.Kd, pc.snr_of(c), pc.GATE, modulation=mod or c.mod)
    rx.set_max_trials(0)
    return rx


def can_pack(c):
    return c.Kd % 4 == 0 and orc.BITS_PER_SYMBOL[c.mod] % 2 == 0


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------------------------------ 1. every case against the oracle
def demod(om, rx, c, d_iq, n, with_eq=True, layout=None):
    """demod_frames into 0xFF-poisoned buffers -> (eq [n][nds][Kd] or None, bit bytes [n][nds][..] or None, tsr [n][4])"""
    fl = pc.frame_len(c)
    bps = orc.BITS_PER_SYMBOL[c.mod]
    nds = c.P * c.D
    assert rx.data_symbols_per_frame(fl) == nds
    nb = n * nds * c.Kd * bps // (8 if layout == "packed" else 1)
    d_eq = poisoned(om, n * nds * c.Kd * 8) if with_eq else None
    d_b = poisoned(om, nb) if layout else None
    d_tsr = poisoned(om, n * 16)
    mode = om.BITS_NONE if layout is None else om.BITS_PACKED if layout == "packed" else om.BITS_UNPACKED
    assert rx.demod_frames(d_iq, n, fl, fl, d_eq, d_b, mode, d_tsr) == nds
    eq = d_eq.download(np.complex64, n * nds * c.Kd).reshape(n, nds, c.Kd) if with_eq else None
    b = d_b.download(np.uint8, nb).reshape(n, nds, -1) if layout else None
    return eq, b, d_tsr.download(np.int32, n * 4).reshape(n, 4)


def against_oracle(c, eq, tsr):
    """every row of every frame: the NaN rows are the oracle's, zero rows are zeros, live rows (padded ones included) pass
    assert_close, nothing is left as poison.  -> per frame the boolean row masks (nan, zero)"""
    masks = []
    assert not (eq.view(np.uint32) == POISON32).any(), "rows left unwritten (0xFF poison)"
    for f, (t, rows) in enumerate(pc.reference(c)):
        assert tsr[f, 3] == 1 and tsr[f, 0] == t[0] and tsr[f, 1] == t[1], (f, tsr[f], t)
        nan, zero, padded, live = pc.row_kinds(c, t, rows)
        assert np.array_equal(~np.isfinite(eq[f]).all(axis=1), nan), (f, np.nonzero(nan)[0])
        assert not eq[f][zero].any(), "frame %d: rows %s must be zeros" % (f, np.nonzero(zero)[0])
        fig = assert_close(eq[f][live], rows[live], "%s frame %d" % (pc.case_id(c), f))
        print("%s frame %d (%s): %d live (%d padded) %d zero %d NaN rows; max %.2e rms %.2e elem %.2e" % (
            pc.case_id(c), f, pc.leads(c)[f][0], live.sum(), padded.sum(), zero.sum(), nan.sum(), *fig))
        masks.append((nan, zero))
    return masks


def bits_against_eq(c, eq, b, layout, masks):
    """the bits are orc.demap_hard of the device's own eq on every non-NaN row; a zero row gives demap_hard(0)"""
    zb = orc.demap_hard(np.zeros(c.Kd, np.complex64), c.mod)
    for f, (nan, zero) in enumerate(masks):
        ok = np.nonzero(~nan)[0]
        want = orc.demap_hard(eq[f][ok].ravel(), c.mod).reshape(len(ok), -1)
        assert np.array_equal(want[zero[ok]], np.tile(zb, (int(zero.sum()), 1)))
        if layout == "packed":
            want = np.packbits(want, axis=1)
        else:
            assert b[f][ok].max() <= 1, "bit rows left unwritten (0xFF poison)"
        assert np.array_equal(b[f][ok], want), "%s frame %d: %s bits" % (pc.case_id(c), f, layout)


def all_outputs(om, rx, c, d_iq, n):
    """every output combination of one handle; the cross-combination identities are asserted on the way"""
    eq0, none, tsr = demod(om, rx, c, d_iq, n)
    assert none is None
    out = dict(eq=eq0, tsr=tsr)
    for layout in ("unpacked", "packed") if can_pack(c) else ("unpacked",):
        eq, b, t = demod(om, rx, c, d_iq, n, layout=layout)
        assert np.array_equal(bits_of(eq), bits_of(eq0)), "%s: the symbols depend on the bits output" % layout
        assert np.array_equal(t, tsr)
        none, b_only, t = demod(om, rx, c, d_iq, n, with_eq=False, layout=layout)
        assert none is None and np.array_equal(b_only, b), "%s: the bits depend on whether the symbols are written" % layout
        assert np.array_equal(t, tsr)
        out[layout] = b
    return out


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_every_row_against_the_oracle(om, c):
    iq = pc.frames(c)
    n = len(iq)
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    rx = engine(om, c)
    got = all_outputs(om, rx, c, d_iq, n)
    masks = against_oracle(c, got["eq"], got["tsr"])
    for layout in ("unpacked", "packed"):
        if layout in got:
            bits_against_eq(c, got["eq"], got[layout], layout, masks)
    if c.S == 1:
        # the default is the screened search; the exhaustive one must give the same trial, lag and every output byte
        assert rx.set_sync_search(False) is True
        assert rx.set_sync_search(True) is False
        again = all_outputs(om, rx, c, d_iq, n)
        for k in got:
            assert np.array_equal(bits_of(again[k]), bits_of(got[k])), "exhaustive search: %s differs" % k
    else:
        assert rx.set_sync_search(False) is False, "S >= 2 has no screened search"


# ------------------------------------------------------------------------------------------ 2. chunk regimes
def regime_cases():
    """per size class one D that does not divide the kernel's symbols per trip and one D above it (the same case where one D is both);
    at 1024-pt the compiled-in and the runtime Kd"""
    pick = {(64, 60): (6, 13), (256, 152): (6, 13), (512, 300): (13,), (1024, 600): (6, 13), (1024, 604): (6,), (2048, 1200): (6,),
            (4096, 2400): (6,)}
    out = [c for c in pc.CASES if c.S == 1 and c.D in pick.get((c.N, c.Kd), ())]
    assert len(out) == sum(len(v) for v in pick.values())
    return out


def dev_demod(om, torch, c, d_iq, n, layout):
    rx = engine(om, c)
    fl = pc.frame_len(c)
    nds = c.P * c.D
    row = nds * c.Kd * orc.BITS_PER_SYMBOL[c.mod]
    eq = torch.full((n, nds * c.Kd * 2), -1, dtype=torch.int32, device="cuda")               # 0xFFFFFFFF
    b = torch.full((n, row // 8 if layout == "packed" else row), 255, dtype=torch.uint8, device="cuda")
    tsr = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    mode = om.BITS_PACKED if layout == "packed" else om.BITS_UNPACKED
    assert rx.demod_frames(d_iq, n, fl, fl, eq, b, mode, tsr, stream=cur(torch)) == nds
    torch.cuda.synchronize()
    return eq, b, tsr


@pytest.mark.parametrize("c", regime_cases(), ids=pc.case_id)
def test_large_batch_equals_small_batch(om, torch, c):
    """The few frames of a case run one trip per chunk (the launcher's "few frames: finer" rule).  Gathered into a batch of
    n_frames * trips >= 3 * 4096 they run as whole-frame chunks of several trips below 1024-pt; with QUEUE_FRAMES frames from
    1024-pt up the launch has more than twice the resident workgroups and the work queue is on.  Every frame of the large batch
    must equal the same frame of the small batch -- checked against the oracle above -- bit for bit."""
    layout = "packed" if can_pack(c) else "unpacked"
    host = pc.frames(c)
    base = torch.from_numpy(np.array(host).view(np.float32)).cuda()              # a writable copy: the shared frames are read-only
    trips = -(-c.P * c.D // NS[c.N])
    if c.N < 1024:
        assert trips > 1 and (NS[c.N] % c.D or c.D > NS[c.N])
    n = QUEUE_FRAMES[c.N] if c.N >= 1024 else -(-3 * 4096 // trips)
    eq0, b0, tsr0 = dev_demod(om, torch, c, base, len(host), layout)
    want_tsr = np.array([[t[0], t[1], t[2], 1] for t, _ in pc.reference(c)], dtype=np.int32)
    assert np.array_equal(tsr0.cpu().numpy()[:, [0, 1, 3]], want_tsr[:, [0, 1, 3]])
    pick = torch.arange(n, device="cuda") % len(host)
    big = base[pick].contiguous()
    eq, b, tsr = dev_demod(om, torch, c, big, n, layout)
    assert torch.equal(tsr, tsr0[pick]), "tsr"
    assert torch.equal(eq, eq0[pick]), "a frame of the large batch differs from the small batch"
    assert torch.equal(b, b0[pick]), "bits"
    assert not bool((eq == -1).any()), "rows left unwritten (0xFF poison)"


# ------------------------------------------------------------------------------------------ 3. composites follow the pattern
COMPOSITE = [c for c in pc.CASES if (c.N, c.Kd, c.S, c.D) in ((64, 60, 1, 6), (1024, 600, 1, 6))]
PILOTS = {64: [-21, -7, 7, 21], 1024: [s * 37 * m for m in range(1, 8) for s in (-1, 1)]}


def composite_frames(c, seed):
    """aligned / no sync at all / last pattern fails the guard / a second lag -> [4][frame_len] complex64"""
    rng = np.random.default_rng(seed)
    L, fl = c.N + c.cp, pc.frame_len(c)
    late = (c.D - 1) * L + c.cp + 16 + ((c.S + 1) * L if c.partial else 0)
    iq = np.stack([pc.make_frame(c, lead, rng)[0] for lead in (3, 0, late, c.cp // 2 + 5)])
    iq[1] = (0.3 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    return iq


class Outs:
    """named 0xFF-poisoned device buffers; read() downloads them all as bytes"""

    def __init__(self, om, **sizes):
        self.n = {k: max(8, int(v)) for k, v in sizes.items()}
        self.d = {k: poisoned(om, v) for k, v in self.n.items()}

    def __getitem__(self, k):
        return self.d[k]

    def read(self):
        return {k: v.download(np.uint8, self.n[k]) for k, v in self.d.items()}


def same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s: %s differs from the stage-by-stage sequence" % (what, k)


def plain(om, rx, c, d_iq, n):
    """demod_frames with unpacked bits -> Outs(eq, bits, tsr), and what the frames must look like"""
    fl, nds, bps = pc.frame_len(c), c.P * c.D, orc.BITS_PER_SYMBOL[c.mod]
    K = rx.cfg.num_data_bins
    p = Outs(om, eq=n * nds * K * 8, bits=n * nds * K * bps, tsr=n * 16)
    assert rx.demod_frames(d_iq, n, fl, fl, p["eq"], p["bits"], om.BITS_UNPACKED, p["tsr"]) == nds
    return p


def check_frame_kinds(c, p, n):
    r = p.read()
    nds = c.P * c.D
    tsr = r["tsr"].view(np.int32).reshape(n, 4)
    eq = r["eq"].view(np.complex64).reshape(n, nds, -1)
    assert list(tsr[:, 3]) == [1, 0, 1, 1][:n] + [1] * (n - 4), tsr
    assert not eq[1].any(), "the frame without a sync must be zero rows"
    assert eq[2, :nds - c.D].any(axis=1).all() and not eq[2, nds - c.D:].any(), "frame 2 must end in one guard-failed pattern"
    assert np.isfinite(eq).all() and eq[0].any(axis=1).all()


@pytest.mark.parametrize("c", COMPOSITE, ids=pc.case_id)
def test_composites_equal_their_stage_sequence(om, c):
    """demod_frames_soft / _csi / _despread / _mrc / _track against the sequence include/ofdm_mi355x.h defines for each, on the
    same handle, bit for bit; then the averaged estimate of set_chan_average(-1) against the stand-alone stage."""
    mod, bps = c.mod, orc.BITS_PER_SYMBOL[c.mod]
    fl, nds, Kd, N = pc.frame_len(c), c.P * c.D, c.Kd, c.N
    iq = composite_frames(c, 11 + c.N)
    n = len(iq)
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    rx = engine(om, c)
    n_eq, n_b = n * nds * Kd, n * nds * Kd * bps
    rho = rx.csi_rho

    p = plain(om, rx, c, d_iq, n)
    check_frame_kinds(c, p, n)
    base = p.read()

    def shared(o):
        return {k: o[k] for k in ("eq", "bits", "tsr")}

    # soft: demod_frames, then demap_frames over d_eq with one segment per frame
    a = Outs(om, soft0=n_b * 4, soft1=n_b * 4, llr=n_b * 4, sigma=n * 8)
    rx.demap_frames(p["eq"], n, nds * Kd, nds * Kd, mod, a["soft0"], a["soft1"], a["llr"], a["sigma"])
    b = Outs(om, eq=n_eq * 8, bits=n_b, tsr=n * 16, soft0=n_b * 4, soft1=n_b * 4, llr=n_b * 4, sigma=n * 8)
    assert rx.demod_frames_soft(d_iq, n, fl, fl, b["eq"], b["soft0"], b["soft1"], b["llr"], b["sigma"], b["bits"], om.BITS_UNPACKED,
                                b["tsr"]) == nds
    got = b.read()
    same(base, shared(got), "soft")
    same(a.read(), got, "soft")

    # csi: demod_frames, csi_frames(CSI_ROWS_ALL), demap_csi_frames
    d_a = poisoned(om, n * Kd * 4)
    rx.demod_frames(d_iq, n, fl, fl, p["eq"], p["bits"], om.BITS_UNPACKED, p["tsr"])
    rx.csi_frames(n, d_a)
    a = Outs(om, llr=n_b * 4, sigma2=n * 8, n_used=n * 8)
    rx.demap_csi_frames(p["eq"], n, nds, Kd, nds * Kd, d_a, Kd, rho, mod, a["llr"], a["sigma2"], a["n_used"])
    b = Outs(om, eq=n_eq * 8, bits=n_b, tsr=n * 16, llr=n_b * 4, sigma2=n * 8, n_used=n * 8)
    assert rx.demod_frames_csi(d_iq, n, fl, fl, b["eq"], b["llr"], b["sigma2"], b["n_used"], d_bits=b["bits"],
                               bits_mode=om.BITS_UNPACKED, d_tsr=b["tsr"]) == nds
    got = b.read()
    same(base, shared(got), "csi")
    same(a.read(), got, "csi")
    used = got["n_used"].view(np.int64)
    assert list(used) == [nds * Kd, 0, (nds - c.D) * Kd, nds * Kd], used          # the guard-failed pattern's D rows are erasures

    # despread, M = Kd: demod_frames, csi_frames into the workspace, dft_despread_frames
    sizes = dict(sym=n_eq * 8, llr=n_b * 4, dbits=n_b, beta=n * 4, weight=n * 4)
    rx.demod_frames(d_iq, n, fl, fl, p["eq"], p["bits"], om.BITS_UNPACKED, p["tsr"])
    rx.csi_frames(n, d_a)
    a = Outs(om, **sizes)
    rx.dft_despread_frames(p["eq"], n, nds, Kd, nds * Kd, d_a, Kd, rho, mod, a["sym"], a["llr"], a["dbits"], om.BITS_UNPACKED, a["beta"],
                           a["weight"])
    b = Outs(om, eq=n_eq * 8, tsr=n * 16, **sizes)
    assert rx.demod_frames_despread(d_iq, n, fl, fl, b["eq"], b["sym"], b["llr"], b["dbits"], om.BITS_UNPACKED, b["beta"], b["weight"],
                                    d_tsr=b["tsr"]) == nds
    got = b.read()
    assert np.array_equal(got["eq"], base["eq"]) and np.array_equal(got["tsr"], base["tsr"])
    same(a.read(), got, "despread")

    # track: the sync search of demod_frames, then chan_track_frames
    sizes = dict(eq=n_eq * 8, bits=n_b, csi=n_eq * 4, H=n * c.P * N * 8, takes=n * c.P * 4)
    a, b = Outs(om, **sizes), Outs(om, tsr=n * 16, **sizes)
    assert rx.chan_track_frames(d_iq, n, fl, fl, p["tsr"], om.TRACK_LINEAR, 0, 0, a["eq"], a["bits"], om.BITS_UNPACKED, a["csi"], a["H"],
                                a["takes"]) == nds
    assert rx.demod_frames_track(d_iq, n, fl, fl, om.TRACK_LINEAR, b["eq"], b["bits"], om.BITS_UNPACKED, b["csi"], b["H"], b["takes"],
                                 b["tsr"]) == nds
    got = b.read()
    assert np.array_equal(got["tsr"], base["tsr"])
    same(a.read(), got, "track")
    takes = got["takes"].view(np.int32).reshape(n, c.P)
    # the sync symbol of the guard-failed pattern lies inside the frame: it takes part, only its data rows are zeros
    assert takes[0].all() and takes[2].all() and takes[3].all() and not takes[1].any(), takes

    # mrc, two branches: frame f of branch b at index b * nf + f
    nf = 2
    d_s2 = poisoned(om, n * 8)
    rx.demod_frames(d_iq, n, fl, fl, p["eq"], p["bits"], om.BITS_UNPACKED, p["tsr"])
    rx.csi_frames(n, d_a)
    given = [0.02, 0.03]
    per = nf * nds * Kd
    a = Outs(om, llr=per * bps * 4, sym=per * 8, weight=per * 4)
    rx.combine_csi_frames(p["eq"], 2, nf, nds, Kd, nds * Kd, d_a, Kd, rho, mod, noise_var=given, d_llr=a["llr"], d_sym_out=a["sym"],
                          d_weight=a["weight"])
    b = Outs(om, eq=n_eq * 8, tsr=n * 16, llr=per * bps * 4, sym=per * 8, weight=per * 4)
    assert rx.demod_frames_mrc(d_iq, 2, nf, fl, fl, b["eq"], given, b["llr"], b["sym"], b["weight"], d_s2, b["tsr"]) == nds
    got = b.read()
    assert np.array_equal(got["eq"], base["eq"]) and np.array_equal(got["tsr"], base["tsr"])
    same(a.read(), got, "mrc")
    w = got["weight"].view(np.float32).reshape(nf, nds, Kd)
    # combined frame 0 = (aligned, guard-failed), frame 1 = (no sync, second lag): every entry is carried by one branch at least
    assert (w > 0).all()
    assert np.array_equal(d_s2.download(np.float64, n), np.repeat(np.array(given), nf))

    # the averaged estimate: frame_state of a call with set_chan_average(-1) = the stand-alone stage on the call's tsr
    rx.set_chan_average(-1)
    q = plain(om, rx, c, d_iq, n)
    assert np.array_equal(q.read()["tsr"], base["tsr"])
    sa = Outs(om, H=n * N * 8, gain=n * Kd * 8, n_used=n * 4)
    rx.chan_average_frames(d_iq, n, fl, fl, q["tsr"], -1, sa["H"], sa["gain"], None, sa["n_used"])
    r = sa.read()
    H, g, used = r["H"].view(np.complex64).reshape(n, N), r["gain"].view(np.complex64).reshape(n, Kd), r["n_used"].view(np.int32)
    assert list(used) == [c.P, 0, c.P, c.P], used                                 # every sync symbol that lies inside the frame
    for f in (0, 2, 3):
        st = rx.frame_state(f)
        assert np.array_equal(bits_of(st["chan_freq"]), bits_of(H[f])) and np.array_equal(bits_of(st["gain"]), bits_of(g[f])), f
    rx.set_chan_average(0)
    same(base, plain(om, rx, c, d_iq, n).read(), "averaging switched off again")


@pytest.mark.parametrize("c", COMPOSITE, ids=pc.case_id)
@pytest.mark.parametrize("mode", [pr.CPE, pr.CPE_SLOPE])
def test_pilot_composite_follows_the_pattern(om, c, mode):
    """demod_frames_pilots = demod_frames, then pilot_track_frames(rows_per_pattern = D), bit for bit; the pilot outputs of the call
    against tests/pilot_ref.py on the call's own d_eq, at the bars of test_gpu_pilot_frames.py (1e-5 norm-relative; the carrier
    offset within 1e-6 relative + 1e-9)."""
    TOL = 1e-5
    N, cp, K, D, mod = c.N, c.cp, c.Kd, c.D, c.mod
    locs = PILOTS[N]
    Kd, bps, L = K - len(locs), orc.BITS_PER_SYMBOL[mod], N + cp
    fl, nds, n_sym = pc.frame_len(c), c.P * D, c.P * (1 + D)
    leads = (7, 0, (D - 1) * L + cp + 16 + ((c.S + 1) * L if c.partial else 0), cp // 2 + 5)
    iq = np.stack([pr.make_frame(N, cp, K, locs, mod, n_sym, 0.004, 0.005, seed=3 + f, lead=ld, frame_len=fl, sync_every=D)[0]
                   for f, ld in enumerate(leads)]).astype(np.complex64)
    rng = np.random.default_rng(5)
    iq[1] = (0.3 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    n = len(iq)
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    rx = engine(om, c)
    rx.set_pilots(locs, 1.0)
    p = plain(om, rx, c, d_iq, n)
    check_frame_kinds(c, p, n)
    base = p.read()
    sizes = dict(data=n * nds * Kd * 8, pbits=n * nds * Kd * bps, cpe=n * nds * 8, slope=n * nds * 4, cfo=n * 8)
    a, b = Outs(om, **sizes), Outs(om, eq=n * nds * K * 8, tsr=n * 16, **sizes)
    slope = (lambda o: o["slope"]) if mode == pr.CPE_SLOPE else (lambda o: None)
    rx.pilot_track_frames(p["eq"], n, nds, nds * K, D, mode, a["data"], a["pbits"], om.BITS_UNPACKED, a["cpe"], slope(a), a["cfo"])
    assert rx.demod_frames_pilots(d_iq, n, fl, fl, b["eq"], mode, b["data"], b["pbits"], om.BITS_UNPACKED, b["cpe"], slope(b), b["cfo"],
                                  d_tsr=b["tsr"]) == nds
    got = b.read()
    assert np.array_equal(got["eq"], base["eq"]) and np.array_equal(got["tsr"], base["tsr"])
    same(a.read(), got, "pilots")
    eq = got["eq"].view(np.complex64).reshape(n, nds, K)
    ref = pr.track_rows(eq, locs, 1.0, mode)
    data, cpe = got["data"].view(np.complex64).reshape(n, nds, Kd), got["cpe"].view(np.complex64).reshape(n, nds)
    figs = dict(data=relerr(data, ref["data"]), cpe=relerr(cpe, ref["cpe"]))
    if mode == pr.CPE_SLOPE:
        figs["slope"] = relerr(got["slope"].view(np.float32).reshape(n, nds), ref["slope"])
    print("%s mode %d:" % (pc.case_id(c), mode), {k: "%.3g" % v for k, v in figs.items()})
    assert all(v < TOL for v in figs.values()), figs
    cfo = got["cfo"].view(np.float64)
    for f in range(n):
        want = pr.cfo_estimate(ref["U"][f], ref["usable"][f], D, N, cp)
        print("frame %d: cfo %r, reference %r" % (f, cfo[f], want))
        if np.isnan(want):
            assert np.isnan(cfo[f]), (f, cfo[f])
        else:
            assert abs(cfo[f] - want) <= 1e-6 * abs(want) + 1e-9, (f, cfo[f], want)
    assert np.isnan(cfo[1]) and abs(cfo[0] - 0.004) < 1e-3, "frame 0 carries an offset of 0.004 subcarrier spacings"
    assert np.array_equal(got["pbits"].reshape(n, nds, -1), pr.hard_bits(data, mod).reshape(n, nds, -1))


# ------------------------------------------------------------------------------------------ 4. device loopback, S = 1
@pytest.mark.parametrize("N,cp,Kd,pattern,mod,P,n", [(64, 16, 60, (1, 13), "QPSK", 2, 300), (512, 36, 300, (1, 1), "16QAM", 5, 200),
                                                    (2048, 144, 1200, (1, 6), "64QAM", 2, 200)])
def test_device_loopback(om, N, cp, Kd, pattern, mod, P, n):
    """TxEngine(pattern) -> channel (one tap, noise_var 1e-6) -> RxEngine(pattern) with packed bits: no bit error.

    S = 1 only.  For S >= 2 TxEngine sends ZC segment 0 in every sync symbol, as the reference transmitter does (its synch_state
    never advances), while the receivers correlate sync symbol LL with segment LL: that is not the zc_segments=True signal the
    receiver locks to, so the S >= 2 cases of this file run on host-generated IQ only."""
    S, D = pattern
    L, bps = N + cp, orc.BITS_PER_SYMBOL[mod]
    n_sym = P * (S + D)
    fl = n_sym * L
    txe = om.TxEngine(N, cp, N - 2, Kd, pattern, mod)
    rxe = om.RxEngine(n_sym, N, cp, N - 2, pattern, Kd, 100, 0.7, modulation=mod)
    nb = txe.bits_per_frame(n_sym)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds == P * D and nb == nds * Kd * bps and nb % 8 == 0
    bits = np.random.default_rng(N + D).integers(0, 2, (n, nb)).astype(np.uint8)
    d_bits = om.DeviceBuffer(bits.nbytes).upload(bits)
    d_ref = om.DeviceBuffer(n * nb // 8).upload(np.packbits(bits, axis=1))
    d_tx, d_rx = om.DeviceBuffer(n * fl * 8), om.DeviceBuffer(n * fl * 8)
    taps = np.array([0.8 - 0.6j], np.complex64)
    d_t = om.DeviceBuffer(taps.nbytes).upload(taps)
    txe.modulate_frames(d_bits, n, n_sym, d_tx)
    txe.channel(d_tx, n, fl, fl, d_t, 1, d_rx, fl, fl, noise_var=1e-6, seed=N)
    d_rx.download(np.uint8, 8)                   # waits for the device: the two handles work on streams of their own
    d_out = poisoned(om, n * nb // 8)
    d_tsr = poisoned(om, n * 16)
    assert rxe.demod_frames(d_rx, n, fl, fl, None, d_out, om.BITS_PACKED, d_tsr) == nds
    tsr = d_tsr.download(np.int32, n * 4).reshape(n, 4)
    assert tsr[:, 3].all() and (tsr[:, 0] == cp).all(), "every frame must find its sync at the first trial"
    d_cnt = om.DeviceBuffer(8).upload(np.zeros(1, np.uint64))
    om.count_bit_errors(d_out, d_ref, n * nb // 8, d_cnt)
    assert int(d_cnt.download(np.uint64, 1)[0]) == 0
