"""GPU parity of the frame-batched CFO-search receiver (ofdm_fo_demod_frames): every frame of a batch is the first work() call
of a fresh SynchEstAndFO / SynchEstFOAndDSSS / table-mode instance.  Yardsticks: the recorded reference runs (callN = 1), the
stream path (a fresh ofdm_fo_work per frame) and oracle.FoOracle.

Tolerances as in test_gpu_fo.py: time_synch_ref[:, 0:2] exact, [:, 2] within +-1, fp32 outputs 1e-5 norm-relative against the
references; against the stream path, which runs the same device functions, the tables are exact and the floats within 1e-6."""
import numpy as np
import pytest

from conftest import poisoned, relerr
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
SAME = 1e-6
R = 100


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


def _check_table(got, ref):
    assert np.array_equal(got[:, 0:2], ref[:, 0:2])
    assert np.max(np.abs(got[:, 2] - ref[:, 2])) <= 1


def _fo_block(case, fo_range, **kw):
    import OFDMReceiver
    return OFDMReceiver.SynchEstAndFO(case, list(fo_range), "/tmp/ofdm_fo_", "cest", 0, **kw)


def _dsss_block(case, fo_range, **kw):
    import OFDMReceiver
    return OFDMReceiver.SynchEstFOAndDSSS(case, list(fo_range), "/tmp/ofdm_fo_", "cest", 0, **kw)


def _table_block(p):
    import RXOFDM
    return RXOFDM.synch_and_chan_est(int(p[0]), int(p[1]), int(p[2]), int(p[3]), [int(p[4]), int(p[5])], int(p[6]), float(p[7]),
                                     "/tmp/", "x", 0, 0, table_mode=True)


def _tx(blk, n_sym, rng, cfo_hz=0.0, fs=1.0, fading=False):
    """The receiver's own numerology through the oracle transmitter (root-37 ZC, segment form): IQ and the sent bits."""
    N, cp, Ks, Kd = blk.nfft, blk.cp_len, blk.num_synch_bins, blk.num_data_bins
    S, D = blk.synch_dat
    n_data = sum(1 for s in range(n_sym) if s % (S + D) >= S)
    bits = rng.integers(0, 2, n_data * Kd * 2)
    tx = orc.tx_modulate(bits, N, cp, Ks, Kd, n_sym, synch_dat=(S, D), zc_root=37, zc_segments=True, zc_parity_of_bins=True)
    if fading:
        tx = orc.channel_apply(tx, orc.REF_TAPS, N)[:len(tx) + 8]
    return tx * np.exp(1j * 2 * np.pi * cfo_hz / fs * np.arange(len(tx))), bits


def _same(got, ref):
    """Stream-path yardstick: the same non-finite entries (an empty data window normalises by 1/0 in both paths, FO:341),
    the finite ones within SAME."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    m = np.isfinite(ref)
    return relerr(got[m], ref[m]) <= SAME


def _make_input(case, cfo_hz, lead, fading, seed):
    """test_gpu_fo.py's input: the same seed gives the same samples."""
    n_symb, fs, N, sd, Kd = orc.FO_CASES[case]
    S, D = sd
    cp = N // 4
    rng = np.random.default_rng(seed)
    n_data = sum(1 for s in range(n_symb) if s % (S + D) >= S)
    bits = rng.integers(0, 2, n_data * Kd * 2)
    tx = orc.tx_modulate(bits, N, cp, N - 2, Kd, n_symb, synch_dat=(S, D), zc_root=37, zc_segments=True, zc_parity_of_bins=True)
    if fading:
        tx = orc.channel_apply(tx, orc.REF_TAPS, N)[:len(tx) + 8]
    rx = tx * np.exp(1j * 2 * np.pi * cfo_hz / fs * np.arange(len(tx)))
    return np.concatenate([np.zeros(lead), rx, np.zeros(2 * cp)]).astype(np.complex64)


def _fit(x, lead, length):
    out = np.zeros(length, np.complex64)
    x = np.concatenate([np.zeros(lead), x])[:length]
    out[:len(x)] = x
    return out


def _fresh(blk_factory, iq):
    """Stream path on a fresh handle: status, tsr, fo_idx and the state arrays after its first work() call."""
    blk = blk_factory()
    e = blk._engine
    rc = e.work(iq, np.zeros(len(iq), np.complex64))
    st = e.state()
    st["status"] = rc if rc < 0 else e.report.n_sync
    st["fo_idx"] = e.report.dmax_tmp_ind
    if e.dsss:
        st["data_freq_d"] = e.despread()
    e.close()
    return st


# ------------------------------------------------------------------------------------------ 1. pinned to the reference
GOLDEN_CASES = [("ref_fo.npz", t) for t in ("c0", "c3", "c6", "c9")] + [("ref_dsss.npz", t) for t in ("d1", "d3")] + \
               [("ref_rxofdm_table.npz", t) for t in ("chain", "s2")]


@pytest.mark.parametrize("fname,tag", GOLDEN_CASES)
def test_batch_equals_recorded_first_calls(golden, fname, tag):
    g = golden(fname)
    if fname == "ref_fo.npz":
        blk = _fo_block(int(g[tag + "_meta"][0]), g[tag + "_fo_range"])
    elif fname == "ref_dsss.npz":
        blk = _dsss_block(int(g[tag + "_meta"][0]), g[tag + "_fo_range"])
    else:
        blk = _table_block(g[tag + "_par"])
    iq = g[tag + "_iq"].astype(np.complex64)
    fl = len(iq)
    L = blk.nfft + blk.cp_len
    rng = np.random.default_rng(sum(map(ord, tag)))
    golden_at = (1, 4, 6)
    batch = np.zeros((8, fl), np.complex64)
    for f in range(8):
        if f in golden_at:
            batch[f] = iq
        else:
            x, _ = _tx(blk, fl // L + 1, rng)
            batch[f] = _fit(x, int(rng.integers(0, L)), fl)
    res = blk.demod_frames(batch)
    k = tag + "_call1_"
    n_sync = int(np.count_nonzero(g[k + "tsr"][:, 0]))
    assert n_sync >= 1
    for f in golden_at:
        assert res["status"][f] == n_sync
        _check_table(res["time_synch_ref"][f], g[k + "tsr"])
        if k + "fo_idx" in g:
            assert res["dmax_tmp_ind"][f] == int(g[k + "fo_idx"][0])
        assert relerr(res["est_chan_freq_P"][f], g[k + "H"]) < TOL
        for name, key in (("est_chan_time", "htime"), ("est_synch_freq", "esf"), ("est_data_freq_d", "edfd")):
            if k + key in g:
                assert relerr(res[name][f], g[k + key]) < TOL, name
        assert relerr(res["est_data_freq"][f], g[k + "edf"]) < TOL
    for f in range(8):
        assert res["status"][f] >= 0
        assert np.array_equal(res["hard_bits"][f].ravel(), orc.demap_hard(res["est_data_freq"][f].ravel(), "QPSK"))
    # the block's own stream state is untouched: its first work() call still is call 1 of the recording
    assert blk.count == 0 and blk.cor_obs == -1
    blk.work([iq], [np.zeros(fl, np.complex64)])
    _check_table(blk.time_synch_ref, g[k + "tsr"])


# ------------------------------------------------------------------------------------------ 2. equal to the stream path
@pytest.mark.parametrize("case,fo_range,cfo_hz,fading,seed", [
    (1, [-22000, -9000, 0, 9000, 22000], 9000.0, False, 22),
    (5, [0, 20000, 41000], -41000.0, True, 23),
    (7, [-30000, 0, 30000, 61000], -30000.0, True, 27),
    (8, [-57000, 0], 57000.0, False, 21),
])
def test_batch_equals_fresh_stream_calls(case, fo_range, cfo_hz, fading, seed):
    """64 frames: frame 0 is the well-conditioned input of test_gpu_fo.py (also checked against the oracle), the others have
    per-frame leads and carrier offsets drawn from -fo_range, so that frames pick different candidates; every frame against
    a fresh ofdm_fo_work."""
    n_symb, fs, N = orc.FO_CASES[case][:3]
    L = N + N // 4
    blk = _fo_block(case, fo_range, py2_rotators=False)
    rng = np.random.default_rng(seed)
    n_frames = 64
    first = _make_input(case, cfo_hz, 4, fading, seed)
    fl = len(first)
    offs = [-float(rng.choice(fo_range)) for _ in range(n_frames - 1)]
    batch = np.stack([first] + [_fit(_tx(blk, n_symb, rng, o, fs, fading)[0], int(rng.integers(0, L)), fl) for o in offs])
    res = blk.demod_frames(batch)
    assert len(set(res["dmax_tmp_ind"].tolist())) >= 2 or len(fo_range) == 1
    for f in range(n_frames):
        st = _fresh(lambda: _fo_block(case, fo_range, py2_rotators=False), batch[f])
        assert res["status"][f] == st["status"] >= 1
        assert np.array_equal(res["time_synch_ref"][f], st["time_synch_ref"].astype(np.int32))
        assert res["dmax_tmp_ind"][f] == st["fo_idx"]
        for name, key in (("est_chan_freq_P", "chan_freq"), ("est_chan_time", "chan_time"), ("est_synch_freq", "synch_freq"),
                          ("est_data_freq", "data_freq")):
            assert _same(res[name][f], st[key]), (f, name)
    o = orc.FoOracle(case, fo_range, py2_rotators=False)                  # frame 0 against the fp64 oracle (well-conditioned)
    o.work(batch[0], np.zeros(fl, np.complex64))
    _check_table(res["time_synch_ref"][0], o.time_synch_ref)
    assert res["dmax_tmp_ind"][0] == o.dmax_tmp_ind
    assert relerr(res["est_chan_freq_P"][0], o.est_chan_freq_P) < TOL
    assert relerr(res["est_chan_time"][0], o.est_chan_time) < TOL
    assert relerr(res["est_synch_freq"][0], o.est_synch_freq) < TOL
    assert relerr(res["est_data_freq"][0], o.est_data_freq) < TOL


# ------------------------------------------------------------------------------------------ device-buffer driver
def _run_engine(om, eng, batch, bits_mode, want_despread=False):
    """FoEngine.demod_frames on poisoned device buffers (0xFF: a row the kernels do not write shows up)."""
    n, fl = batch.shape
    c = eng.cfg
    N, Kd, mm = c.nfft, c.num_data_bins, c.synch_S * c.num_synch_bins
    nb = n * R * (Kd * 2 if bits_mode == om.BITS_UNPACKED else Kd // 4)
    b = dict(status=poisoned(om, n * 4), tsr=poisoned(om, n * R * 12), fo=poisoned(om, n * 4), edf=poisoned(om, n * R * Kd * 8),
             bits=poisoned(om, nb), H=poisoned(om, n * R * N * 8), ht=poisoned(om, n * R * N * 8), esf=poisoned(om, n * R * mm * 8))
    if want_despread:
        b["edfd"] = poisoned(om, n * R * eng.n_spread * 8)
    d_iq = om.DeviceBuffer(batch.nbytes).upload(np.ascontiguousarray(batch, np.complex64))
    assert eng.demod_frames(d_iq, n, fl, fl, b["status"], d_tsr=b["tsr"], d_fo_idx=b["fo"], d_data_freq=b["edf"], d_bits=b["bits"],
                            bits_mode=bits_mode, d_data_freq_d=b.get("edfd"), d_chan_freq=b["H"], d_chan_time=b["ht"],
                            d_synch_freq=b["esf"]) == R
    out = dict(status=b["status"].download(np.int32, n), tsr=b["tsr"].download(np.int32, n * R * 3).reshape(n, R, 3),
               fo_idx=b["fo"].download(np.int32, n), data_freq=b["edf"].download(np.complex64, n * R * Kd).reshape(n, R, Kd),
               bits=b["bits"].download(np.uint8, nb).reshape(n, R, -1),
               chan_freq=b["H"].download(np.complex64, n * R * N).reshape(n, R, N),
               chan_time=b["ht"].download(np.complex64, n * R * N).reshape(n, R, N),
               synch_freq=b["esf"].download(np.complex64, n * R * mm).reshape(n, R, mm))
    if want_despread:
        out["data_freq_d"] = b["edfd"].download(np.complex64, n * R * eng.n_spread).reshape(n, R, -1)
    return out


# ------------------------------------------------------------------------------------------ 3. bits
def test_batch_bits_with_matching_candidates(om):
    """Frames whose offset the rotators cancel (as test_fo_block_recovers_bits_with_matching_candidate, offsets a whole number
    of cycles per symbol period) with per-frame leads: packed and unpacked bits equal demap_hard(data_freq), and zero bit
    errors on every frame the fp64 reference recovers exactly (at least half of them).
    One handle per offset: the reference rotates every sync of a frame by the LAST trial's pick and estimates with the LAST
    candidate (FO:268-274, 339), so a matched estimate and a matched data rotation need that candidate in both places.
    A mixed batch over a handle with all candidates still de-maps its own data_freq exactly."""
    case = 2
    n_symb, fs, N, sd, Kd = orc.FO_CASES[case]
    L = N + N // 4
    rng = np.random.default_rng(11)
    offsets = (12000.0, -24000.0, 36000.0)
    assert all((o * L) % fs == 0 for o in offsets)
    fl = n_symb * L + 480 + 2 * (N // 4)
    for o in offsets:
        blk = _fo_block(case, [-o], py2_rotators=False)
        frames, sent = [], []
        for f in range(6):
            x, bits = _tx(blk, n_symb, rng, o, fs)
            frames.append(_fit(x, 240 * (f % 3), fl))                   # leads lcm(stride, L) apart: the same window alignment
            sent.append(bits)
        batch = np.stack(frames)
        up = _run_engine(om, blk._engine, batch, om.BITS_UNPACKED)
        pk = _run_engine(om, blk._engine, batch, om.BITS_PACKED)
        clean = 0
        for f in range(6):
            n_sync = int(up["status"][f])
            assert n_sync == n_symb // 2 and up["fo_idx"][f] == 0
            assert np.array_equal(up["bits"][f].ravel(), orc.demap_hard(up["data_freq"][f].ravel(), "QPSK"))
            assert np.array_equal(np.unpackbits(pk["bits"][f].ravel()), up["bits"][f].ravel())
            # the fp64 reference: where it recovers every bit, so must the batch (on some frames the reference's own first
            # gate-passing window costs one data symbol a few dozen bits)
            ob = orc.FoOracle(case, [-o], py2_rotators=False)
            ob.work(batch[f], np.zeros(fl, np.complex64))
            ref_err = int(np.count_nonzero(orc.demap_hard(ob.est_data_freq[:n_sync].ravel(), "QPSK") != sent[f][:n_sync * Kd * 2]))
            err = int(np.count_nonzero(up["bits"][f][:n_sync].ravel() != sent[f][:n_sync * Kd * 2]))
            if ref_err == 0:
                assert err == 0, (o, f)
                clean += 1
        assert clean >= 3
    blk = _fo_block(case, [-o for o in offsets], py2_rotators=False)
    batch = np.stack([_fit(_tx(blk, n_symb, rng, offsets[f % 3], fs)[0], 240 * (f % 3), fl) for f in range(9)])
    up = _run_engine(om, blk._engine, batch, om.BITS_UNPACKED)
    pk = _run_engine(om, blk._engine, batch, om.BITS_PACKED)
    assert np.array_equal(up["bits"].ravel(), orc.demap_hard(up["data_freq"].ravel(), "QPSK"))
    assert np.array_equal(np.unpackbits(pk["bits"].reshape(9, -1), axis=1), up["bits"].reshape(9, -1))


# ------------------------------------------------------------------------------------------ 4. error isolation, zero rows
def test_batch_isolates_the_101st_sync_and_writes_zero_rows(om):
    case = 0
    n_symb, fs, N, sd, Kd = orc.FO_CASES[case]
    L = N + N // 4
    blk = _fo_block(case, [0.0])
    rng = np.random.default_rng(3)
    long_iq, _ = _tx(blk, 2 * 104, rng)                                     # 104 sync patterns: a 101st sync (FO:294-296)
    fl = len(long_iq) + 2 * (N // 4)
    quiet = (1e-3 * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)
    frames = []
    for f in range(6):
        if f == 2:
            frames.append(_fit(long_iq, 0, fl))
        elif f == 4:
            frames.append(quiet)
        else:
            frames.append(_fit(_tx(blk, n_symb, rng)[0], int(rng.integers(0, L)), fl))
    batch = np.stack(frames)
    res = _run_engine(om, blk._engine, batch, om.BITS_UNPACKED)
    assert res["status"][2] == om._lib.OFDM_ERR_INDEX
    st = _fresh(lambda: _fo_block(case, [0.0]), batch[2])
    assert st["status"] == om._lib.OFDM_ERR_INDEX                                  # the stream path raises there too
    assert res["status"][4] == 0
    q = _fresh(lambda: _fo_block(case, [0.0]), batch[4])
    assert res["fo_idx"][4] == q["fo_idx"] == 0
    for key in ("tsr", "data_freq", "chan_freq", "chan_time", "synch_freq"):
        assert not res[key][4].any(), key
    for f in (0, 1, 3, 4, 5):
        st = _fresh(lambda: _fo_block(case, [0.0]), batch[f])
        assert res["status"][f] == st["status"]
        assert np.array_equal(res["tsr"][f], st["time_synch_ref"].astype(np.int32))
        assert res["fo_idx"][f] == st["fo_idx"]
        for key in ("data_freq", "chan_freq", "chan_time", "synch_freq"):
            assert np.isfinite(res[key][f]).all(), (f, key)               # every row written (poison is NaN)
            assert _same(res[key][f], st[key]), (f, key)
        assert set(np.unique(res["bits"][f]).tolist()) <= {0, 1}
        assert np.array_equal(res["bits"][f].ravel(), orc.demap_hard(res["data_freq"][f].ravel(), "QPSK"))
        n = int(res["status"][f])
        assert not res["tsr"][f][n:].any() and not res["data_freq"][f][n:].any() and not res["chan_freq"][f][n:].any()


def test_batch_despread_equals_fresh_stream_calls(om):
    """SynchEstFOAndDSSS: despread rows of every frame equal a fresh stream call's, zero rows included."""
    case, fo_range = 4, [-24000.0, 0.0, 24000.0]                          # 2 cycles per symbol period: the 3 sync symbols add up
    n_symb, fs, N, sd, Kd, dsss = orc.DSSS_CASES[case]
    L = N + N // 4
    blk = _dsss_block(case, fo_range, py2_rotators=False)
    rng = np.random.default_rng(8)
    fl = n_symb * L + L
    batch = np.stack([_fit(_tx(blk, n_symb, rng, -fo_range[f % 3], fs)[0], int(rng.integers(0, L)), fl) for f in range(12)])
    res = _run_engine(om, blk._engine, batch, om.BITS_PACKED, want_despread=True)
    for f in range(12):
        st = _fresh(lambda: _dsss_block(case, fo_range, py2_rotators=False), batch[f])
        assert res["status"][f] == st["status"] >= 1
        assert np.array_equal(res["tsr"][f], st["time_synch_ref"].astype(np.int32))
        assert _same(res["data_freq"][f], st["data_freq"])
        assert _same(res["data_freq_d"][f], st["data_freq_d"])


# ------------------------------------------------------------------------------------------ 5. asynchronous, capturable
def test_batch_is_graph_capturable_and_stream_ordered(om):
    """After ofdm_fo_reserve the call only enqueues on the caller's stream: captured into a hipGraph and replayed twice, the
    outputs equal the eager call's."""
    import torch
    case, fo_range = 6, [-24000.0, 0.0, 24000.0]
    n_symb, fs, N, sd, Kd = orc.FO_CASES[case]
    L = N + N // 4
    blk = _fo_block(case, fo_range, py2_rotators=False)
    rng = np.random.default_rng(9)
    n, fl = 16, n_symb * L + L
    batch = np.stack([_fit(_tx(blk, n_symb, rng, -fo_range[f % 3], fs, True)[0], int(rng.integers(0, L)), fl) for f in range(n)])
    eng = blk._engine
    eng.reserve(n, fl)
    d_iq = torch.from_numpy(batch.view(np.float32).reshape(n, fl, 2)).cuda()
    outs = dict(d_status=torch.zeros(n, dtype=torch.int32, device="cuda"),
                d_tsr=torch.zeros((n, R, 3), dtype=torch.int32, device="cuda"),
                d_fo_idx=torch.zeros(n, dtype=torch.int32, device="cuda"),
                d_data_freq=torch.zeros((n, R, Kd, 2), dtype=torch.float32, device="cuda"),
                d_bits=torch.zeros((n, R, Kd // 4), dtype=torch.uint8, device="cuda"),
                d_chan_freq=torch.zeros((n, R, N, 2), dtype=torch.float32, device="cuda"))
    s = torch.cuda.Stream()

    def call(stream):
        eng.demod_frames(d_iq, n, fl, fl, outs["d_status"], d_tsr=outs["d_tsr"], d_fo_idx=outs["d_fo_idx"],
                         d_data_freq=outs["d_data_freq"], d_bits=outs["d_bits"], bits_mode=om.BITS_PACKED,
                         d_chan_freq=outs["d_chan_freq"], stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    assert int(eager["d_status"].min()) >= 1
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert not outs["d_status"].any()                                     # capture enqueues nothing
    for _ in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], eager[k]), k
