"""The LTE tail-biting convolutional codec of the frame-batched path on the GPU (-m gpu): ofdm_tx_tbcc_encode_frames and
ofdm_tbcc_decode_frames against tests/tbcc_ref.py (the contract in NumPy float32), bit for bit and metric for metric.

Inputs of the end-to-end cases (E2E): the noise of each case was chosen on the CPU first.  The fp64 chain -- information bits ->
tbcc_ref.encode_segments -> oracle tx_modulate -> reference taps -> complex noise of variance nv -> a fresh RxOracle (snr 100) ->
oracle.bit_recovery (QPSK) / oracle.soft_demap_qam -> llr = soft0 - soft1 -> tbcc_ref.decode -- with 16 symbols per frame and
seed 1 gave, at the listed nv and at 1.5 dB more noise:

    N     constellation  K     nv (dB)   frames  raw BER listed / +1.5 dB   block errors listed / +1.5 dB
    64    QPSK           40    -13.0     8       1.7 % / 3.1 %              0 / 96    0 / 96      (12 / 96 at +3 dB)
    1024  16-QAM         256   -13.5     3       3.1 % / 5.0 %              0 / 111   0 / 111     (2 / 111 at +3 dB)
    2048  64-QAM         1024  -18.0     2       5.1 % / 6.9 %              0 / 56    0 / 56      (0 / 56 at +3 dB, 4 / 56 at +4.5 dB)

The raw error rate is that of the hard decisions of the same LLRs against the coded bits (the taps fade some bins, and no
interleaver spreads them).  No block is left out: the taps are handed over zero-padded to cp + 1 entries so that the channel
delivers a frame cp samples longer than its symbols, every pattern passes the reference's guard (asserted: 0 zero rows) and the
sync lies at the frame's start."""
import numpy as np
import pytest

import tbcc_ref
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

GEOM = {64: (16, 60), 1024: (72, 600), 2048: (144, 1200)}       # N: (cp, Kd)
BPS = {"QPSK": 2, "16QAM": 4, "64QAM": 6}
KS = (24, 40, 96, 256, 1024, 2048)
N_SYM = 16
#       N     constellation  K     noise_var            frames
E2E = [(64, "QPSK", 40, 10 ** -1.3, 8),
       (1024, "16QAM", 256, 10 ** -1.35, 3),
       (2048, "64QAM", 1024, 10 ** -1.8, 2)]
POISON = 0xA5


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


@pytest.fixture(scope="module")
def rx0(om, torch):
    """any receiver handle serves the decoder (it reads LLR buffers, not the handle's numerology)"""
    return om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)


@pytest.fixture(scope="module")
def tx0(om, torch):
    return om.TxEngine(64, 16, 62, 60)


def pack_msb(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=-1, bitorder="big")


def gpu_encode(om, tx, info, seg_bits, info_mode, coded_mode, tail=16):
    """info [n_seg][bps][K] -> the coded buffer's bytes [n_seg][seg_bytes] and the `tail` bytes behind it (poisoned before)"""
    n_seg, bps, K = info.shape
    src = pack_msb(info) if info_mode == om.BITS_PACKED else info
    seg_bytes = seg_bits // 8 if coded_mode == om.BITS_PACKED else seg_bits
    d_info = om.DeviceBuffer(max(src.nbytes, 1)).upload(src)
    d_coded = om.DeviceBuffer(n_seg * seg_bytes + tail).upload(np.full(n_seg * seg_bytes + tail, POISON, np.uint8))
    tx.tbcc_encode_frames(d_info, n_seg, bps, K, d_coded, seg_bits, info_mode=info_mode, coded_mode=coded_mode)
    raw = d_coded.download(np.uint8, n_seg * seg_bytes + tail)
    return raw[:n_seg * seg_bytes].reshape(n_seg, seg_bytes), raw[n_seg * seg_bytes:], d_coded


def gpu_decode(om, rx, llr_seg, bps, K, packed=False, d_llr=None, stride=None):
    """llr_seg [n_seg][stride] float32 (or a device buffer + n_seg, stride) -> bits [n_seg][bps][K], metric, tb_ok, raw bit bytes"""
    if d_llr is None:
        llr_seg = np.ascontiguousarray(llr_seg, np.float32)
        n_seg, stride = llr_seg.shape
        d_llr = om.DeviceBuffer(llr_seg.nbytes).upload(llr_seg)
    else:
        n_seg = llr_seg
    nb = n_seg * bps
    nbytes = nb * (K // 8 if packed else K)
    d_bits = om.DeviceBuffer(nbytes).upload(np.full(nbytes, POISON, np.uint8))
    d_m = om.DeviceBuffer(nb * 4).upload(np.full(nb, np.nan, np.float32))
    d_ok = om.DeviceBuffer(nb * 4).upload(np.full(nb, -7, np.int32))
    rx.tbcc_decode_frames(d_llr, n_seg, stride, bps, K, d_bits=d_bits, bits_mode=om.BITS_PACKED if packed else om.BITS_UNPACKED,
                          d_metric=d_m, d_tb_ok=d_ok)
    raw = d_bits.download(np.uint8, nbytes)
    bits = (np.unpackbits(raw.reshape(nb, K // 8), axis=1, bitorder="big") if packed else raw.reshape(nb, K)).reshape(n_seg, bps, K)
    return bits, d_m.download(np.float32, nb).reshape(n_seg, bps), d_ok.download(np.int32, nb).reshape(n_seg, bps), raw


def check_decode(om, rx, llr_blocks, K, packed=False):
    """blocks [n][3K] as one segment each -> GPU == reference exactly; returns the reference's outputs"""
    bits, metric, ok, _ = gpu_decode(om, rx, llr_blocks, 1, K, packed)
    rb, rm, rok = tbcc_ref.decode(llr_blocks)
    assert np.array_equal(bits[:, 0], rb), "decoded bits differ from the reference in %d blocks" % int(np.any(bits[:, 0] != rb, axis=1).sum())
    assert np.array_equal(ok[:, 0], rok)
    assert np.array_equal(metric[:, 0], rm), "path metrics differ: max |d| = %g" % float(np.max(np.abs(metric[:, 0] - rm)))
    return rb, rm, rok


# ------------------------------------------------------------------------------------------ GPU against the reference
@pytest.mark.parametrize("coded_packed", (False, True), ids=("coded1", "coded8"))
@pytest.mark.parametrize("info_packed", (False, True), ids=("info1", "info8"))
@pytest.mark.parametrize("K,bps,n_seg", ((24, 5, 7), (40, 3, 5), (256, 2, 3), (2048, 1, 2)))
def test_encoder_equals_reference_and_writes_the_filler(om, tx0, K, bps, n_seg, info_packed, coded_packed):
    rng = np.random.default_rng(K + bps)
    info = rng.integers(0, 2, (n_seg, bps, K)).astype(np.uint8)
    # filler behind the blocks; segment sizes in bytes that are no multiple of 4 (whole-word stores must not cross a segment)
    seg_bits = bps * 3 * K + (40 if coded_packed else 45)
    want = tbcc_ref.encode_segments(info, seg_bits)
    got, tail, _ = gpu_encode(om, tx0, info, seg_bits, om.BITS_PACKED if info_packed else om.BITS_UNPACKED,
                              om.BITS_PACKED if coded_packed else om.BITS_UNPACKED)
    if coded_packed:
        want = pack_msb(want)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert np.all(tail == POISON), "the encoder wrote behind its last segment"


@pytest.mark.parametrize("K,n_blocks", ((40, 400), (256, 200), (1024, 50)))
def test_decoder_equals_reference_on_seeded_noisy_llrs(om, rx0, K, n_blocks):
    """the LLRs of tests/test_tbcc_ref_host.py (seed 1, Es/N0 = 2 dB and 0 dB): bits, tb_ok and the float32 metric, exactly"""
    for esn0 in (2.0, 0.0):
        rng = np.random.default_rng(1)
        c = rng.integers(0, 2, (n_blocks, K)).astype(np.uint8)
        llr = tbcc_ref.awgn_llrs(tbcc_ref.encode(c), esn0, rng)
        rb, _, _ = check_decode(om, rx0, llr, K)
        assert np.array_equal(rb, c)
    check_decode(om, rx0, llr, K, packed=True)


@pytest.mark.parametrize("K", KS)
def test_decoder_equals_reference_on_nan_inf_and_ties(om, rx0, K):
    rng = np.random.default_rng(K)
    c = rng.integers(0, 2, (6, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(tbcc_ref.encode(c), 1.0, rng)
    llr[1, rng.integers(0, 3 * K, K // 4)] = np.nan
    llr[2, rng.integers(0, 3 * K, K // 4)] = np.inf
    llr[2, rng.integers(0, 3 * K, K // 4)] = -np.inf
    llr[3] = rng.integers(-1, 2, 3 * K).astype(np.float32)                    # small integers: exact ties on most steps
    llr[4] = 0.0
    llr[5] = np.nan
    rb, rm, rok = check_decode(om, rx0, llr, K)
    assert not rb[4].any() and not rb[5].any() and rm[4] == 0 and rm[5] == 0 and rok[4] == 1
    noiseless = (1.0 - 2.0 * tbcc_ref.encode(c)).astype(np.float32)
    rb, rm, rok = check_decode(om, rx0, noiseless, K, packed=True)
    assert np.array_equal(rb, c) and np.all(rok == 1) and np.all(rm == np.float32(3 * (K + 192)))


@pytest.mark.parametrize("K", (40, 256, 2048))
def test_a_block_alone_in_a_batch_at_a_stride_and_on_a_repeated_call(om, rx0, K):
    rng = np.random.default_rng(5 + K)
    n = 12
    c = rng.integers(0, 2, (n, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(tbcc_ref.encode(c), 0.0, rng)
    alone = [gpu_decode(om, rx0, llr[i:i + 1], 1, K) for i in range(n)]
    b1, m1, ok1, raw1 = gpu_decode(om, rx0, llr.reshape(1, n * 3 * K), n, K)                     # one segment of 12 blocks
    wide = np.full((4, 3 * 3 * K + 37), np.nan, np.float32)                                       # 4 segments of 3, larger stride
    wide[:, :9 * K] = llr.reshape(4, 9 * K)
    b2, m2, ok2, raw2 = gpu_decode(om, rx0, wide, 3, K)
    b3, m3, ok3, raw3 = gpu_decode(om, rx0, wide, 3, K)                                           # repeated call
    assert raw1.tobytes() == raw2.tobytes() == raw3.tobytes()
    assert m1.tobytes() == m2.tobytes() == m3.tobytes() and ok1.tobytes() == ok2.tobytes() == ok3.tobytes()
    for i in range(n):
        assert alone[i][3].tobytes() == raw1[i * K:(i + 1) * K].tobytes(), i
        assert alone[i][1].tobytes() == m1.ravel()[i:i + 1].tobytes() and alone[i][2].ravel()[0] == ok1.ravel()[i]
    bp, mp, okp, _ = gpu_decode(om, rx0, wide, 3, K, packed=True)
    assert np.array_equal(bp, b2) and mp.tobytes() == m2.tobytes() and np.array_equal(okp, ok2)


# ------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("case", E2E, ids=lambda c: "%d-%s-K%d" % (c[0], c[1], c[2]))
def test_encode_modulate_channel_demod_decode(om, torch, case):
    """Fails without the codec.  Random information bits -> encode -> modulate_frames -> channel + AWGN -> demod_frames_soft ->
    decode: the decoded bits are tbcc_ref's on that call's LLRs and the transmitted information bits, while the hard bits of
    the same call are wrong in at least 1 % of the coded positions."""
    N, mod, K, nv, n = case
    cp, Kd = GEOM[N]
    L, bps = N + cp, BPS[mod]
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    rxe = om.RxEngine(N_SYM, N, cp, N - 2, (1, 3), Kd, 100, 0.7, modulation=mod)
    rxe.set_max_trials(0)
    seg_bits = txe.bits_per_frame(N_SYM)
    nblk = om.tbcc_blocks(seg_bits, K)
    assert nblk == seg_bits // (3 * K) and nblk >= 12
    rng = np.random.default_rng(N)
    info = rng.integers(0, 2, (n, nblk, K)).astype(np.uint8)
    coded, _, d_coded = gpu_encode(om, txe, info, seg_bits, om.BITS_UNPACKED, om.BITS_UNPACKED, tail=0)
    assert np.array_equal(coded, tbcc_ref.encode_segments(info, seg_bits))
    fl_tx, fl = N_SYM * L, N_SYM * L + cp
    d_tx, d_rx = om.DeviceBuffer(n * fl_tx * 8), om.DeviceBuffer(n * fl * 8)
    taps = np.zeros(cp + 1, np.complex64)
    taps[:5] = orc.REF_TAPS / np.linalg.norm(orc.REF_TAPS)
    d_t = om.DeviceBuffer(taps.nbytes).upload(taps)
    txe.modulate_frames(d_coded, n, N_SYM, d_tx)
    txe.channel(d_tx, n, fl_tx, fl_tx, d_t, len(taps), d_rx, fl, fl, noise_var=nv, seed=11)
    nds = rxe.data_symbols_per_frame(fl)
    assert nds * Kd * bps == seg_bits
    d_eq, d_llr = om.DeviceBuffer(n * nds * Kd * 8), om.DeviceBuffer(n * seg_bits * 4)
    d_hb, d_tsr = om.DeviceBuffer(n * seg_bits), om.DeviceBuffer(n * 16)
    assert rxe.demod_frames_soft(d_rx, n, fl, fl, d_eq, d_llr=d_llr, d_bits=d_hb, bits_mode=om.BITS_UNPACKED, d_tsr=d_tsr) == nds
    eq = d_eq.download(np.complex64, n * nds * Kd).reshape(n, nds, Kd)
    assert d_tsr.download(np.int32, n * 4).reshape(n, 4)[:, 3].all()
    assert int((~eq.any(axis=2)).sum()) == 0, "every pattern passes the guard with these frames: no block is left out"
    llr = d_llr.download(np.float32, n * seg_bits).reshape(n, seg_bits)
    hard = d_hb.download(np.uint8, n * seg_bits).reshape(n, seg_bits)
    used = nblk * 3 * K
    raw_ber = float((hard[:, :used] != coded[:, :used]).mean())
    bits, metric, ok, _ = gpu_decode(om, rxe, n, nblk, K, d_llr=d_llr, stride=seg_bits)
    rb, rm, rok = tbcc_ref.decode_segments(llr, nblk, K)
    wrong = int(np.any(bits != info, axis=2).sum())
    print("N=%d %s K=%d nv=%.4g: raw BER %.4f, %d blocks, %d wrong, tb_ok %d" % (N, mod, K, nv, raw_ber, n * nblk, wrong, int(ok.sum())))
    assert np.array_equal(bits, rb) and np.array_equal(metric, rm) and np.array_equal(ok, rok)
    assert raw_ber >= 0.01, "the uncoded decisions should be wrong in at least 1 %% of the coded positions: %.4f" % raw_ber
    assert wrong == 0, "%d of %d blocks differ from the transmitted information bits" % (wrong, n * nblk)


def pilot_frame(bits, N, cp, K, locs, mod, eps, noise, rng, lead=7):
    """tests/pilot_ref.make_frame for GIVEN bits: map -> grid with pilots -> IFFT -> CP -> mux -> reference channel -> lead ->
    carrier offset eps (subcarrier spacings) -> noise per component"""
    L, Kd = N + cp, K - len(locs)
    sym = orc.map_bits(bits, mod).reshape(-1, Kd)
    rows = orc.tx_stage_cp(orc.tx_stage_ifft(orc.tx_stage_grid(sym, N, Kd, locs, 1.0 + 0j)), cp)
    tx = orc.tx_stage_mux(rows, N, cp, 23, 3, N - 2).ravel()
    fl = N_SYM * L + cp
    x = np.concatenate([np.zeros(lead), orc.channel_apply(tx, orc.REF_TAPS, N)])[:fl]
    x = x * np.exp(2j * np.pi * eps * np.arange(fl) / N)
    return (x + noise * (rng.standard_normal(fl) + 1j * rng.standard_normal(fl))).astype(np.complex64)


def test_decode_behind_the_pilot_tracking_receiver(om, torch):
    """1024-pt QPSK with 14 pilots at a carrier offset of 0.01 subcarrier spacings: the LLRs of the TRACKED data symbols decode
    to the transmitted information bits (noise 0.02 per component, the level tests/test_gpu_pilot_frames.py uses for this
    numerology)."""
    import pilot_ref as pr
    N, mod, K_code, n = 1024, "QPSK", 256, 2
    cp, K = GEOM[N]
    step = (K // 2) // 8
    locs = [s * step * m for m in range(1, 8) for s in (-1, 1)]
    Kd = K - len(locs)
    nds = N_SYM // 4 * 3
    seg_bits = nds * Kd * 2
    nblk = om.tbcc_blocks(seg_bits, K_code)
    rng = np.random.default_rng(3)
    info = rng.integers(0, 2, (n, nblk, K_code)).astype(np.uint8)
    txe = om.TxEngine(N, cp, N - 2, Kd, (1, 3), mod)
    coded, _, _ = gpu_encode(om, txe, info, seg_bits, om.BITS_PACKED, om.BITS_UNPACKED, tail=0)
    assert np.array_equal(coded, tbcc_ref.encode_segments(info, seg_bits))
    iq = np.stack([pilot_frame(coded[f], N, cp, K, locs, mod, 0.01, 0.02, rng) for f in range(n)])
    fl = iq.shape[1]
    rxe = om.RxEngine(N_SYM, N, cp, N - 2, (1, 3), K, 100, 0.7, modulation=mod)
    rxe.set_max_trials(0)
    rxe.set_pilots(locs, 1.0)
    assert rxe.data_symbols_per_frame(fl) == nds
    d_iq = om.DeviceBuffer(iq.nbytes).upload(iq)
    d_eq, d_data = om.DeviceBuffer(n * nds * K * 8), om.DeviceBuffer(n * nds * Kd * 8)
    d_llr, d_cfo = om.DeviceBuffer(n * seg_bits * 4), om.DeviceBuffer(n * 8)
    assert rxe.demod_frames_pilots(d_iq, n, fl, fl, d_eq, mode=pr.CPE, d_data=d_data, d_cfo=d_cfo, d_llr=d_llr) == nds
    eq = d_eq.download(np.complex64, n * nds * K).reshape(n, nds, K)
    assert int((~eq.any(axis=2)).sum()) == 0
    cfo = d_cfo.download(np.float64, n)
    assert np.all(np.abs(cfo - 0.01) < 2e-3), cfo
    llr = d_llr.download(np.float32, n * seg_bits).reshape(n, seg_bits)
    bits, metric, ok, _ = gpu_decode(om, rxe, n, nblk, K_code, d_llr=d_llr, stride=seg_bits)
    rb, rm, rok = tbcc_ref.decode_segments(llr, nblk, K_code)
    assert np.array_equal(bits, rb) and np.array_equal(metric, rm) and np.array_equal(ok, rok)
    assert np.array_equal(bits, info), "%d blocks differ from the transmitted bits" % int(np.any(bits != info, axis=2).sum())


# ------------------------------------------------------------------------------------------ capture, errors
def test_decode_is_capturable_after_reserve(om, torch, rx0):
    K, n_seg, bps = 256, 6, 5
    rng = np.random.default_rng(9)
    c = rng.integers(0, 2, (n_seg * bps, K)).astype(np.uint8)
    llr = tbcc_ref.awgn_llrs(tbcc_ref.encode(c), 0.0, rng).reshape(n_seg, bps * 3 * K)
    rx0.reserve_tbcc(n_seg * bps, K)
    d_llr = torch.from_numpy(llr).cuda()
    outs = dict(bits=torch.zeros(n_seg * bps * K // 8, dtype=torch.uint8, device="cuda"),
                metric=torch.zeros(n_seg * bps, dtype=torch.float32, device="cuda"),
                ok=torch.zeros(n_seg * bps, dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()

    def call(stream):
        rx0.tbcc_decode_frames(d_llr, n_seg, bps * 3 * K, bps, K, d_bits=outs["bits"], bits_mode=om.BITS_PACKED, d_metric=outs["metric"],
                               d_tb_ok=outs["ok"], stream=stream)

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = {k: v.clone() for k, v in outs.items()}
    rb, rm, rok = tbcc_ref.decode(llr.reshape(n_seg * bps, 3 * K))
    assert np.array_equal(eager["bits"].cpu().numpy(), pack_msb(rb).ravel())
    assert np.array_equal(eager["metric"].cpu().numpy(), rm) and np.array_equal(eager["ok"].cpu().numpy(), rok)
    for v in outs.values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert not outs["metric"].any()                                         # capture enqueues nothing
    for _ in range(2):
        for v in outs.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], eager[k]), k


def test_argument_errors_leave_poisoned_outputs_untouched(om, rx0, tx0):
    K, bps, n_seg = 40, 2, 3
    llr = np.ones((n_seg, bps * 3 * K), np.float32)
    d_llr = om.DeviceBuffer(llr.nbytes).upload(llr)
    nb = n_seg * bps
    d_bits = om.DeviceBuffer(nb * K).upload(np.full(nb * K, POISON, np.uint8))
    d_m = om.DeviceBuffer(nb * 4).upload(np.full(nb, 12345.0, np.float32))
    d_ok = om.DeviceBuffer(nb * 4).upload(np.full(nb, -7, np.int32))

    def dec(n_seg_, stride, bps_, K_, mode=om.BITS_UNPACKED):
        rx0.tbcc_decode_frames(d_llr, n_seg_, stride, bps_, K_, d_bits=d_bits, bits_mode=mode, d_metric=d_m, d_tb_ok=d_ok)

    for args in ((n_seg, bps * 3 * K, bps, 44), (n_seg, bps * 3 * K, bps, 16), (n_seg, bps * 3 * K, bps, 2056),
                 (n_seg, bps * 3 * K - 1, bps, K), (-1, bps * 3 * K, bps, K), (n_seg, bps * 3 * K, -1, K),
                 (2 ** 31, bps * 3 * K, 2, K), (n_seg, 2 ** 41, bps, K), (n_seg, bps * 3 * K, bps, K, om.BITS_NONE)):
        with pytest.raises(ValueError):
            dec(*args)
    with pytest.raises(ValueError):
        rx0.reserve_tbcc(4, 20)
    with pytest.raises(ValueError):
        rx0.reserve_tbcc(-1, 40)
    dec(0, bps * 3 * K, bps, K)                                             # no-ops
    dec(n_seg, bps * 3 * K, 0, K)
    rx0.tbcc_decode_frames(d_llr, n_seg, bps * 3 * K, bps, K)
    assert np.all(d_bits.download(np.uint8, nb * K) == POISON)
    assert np.all(d_m.download(np.float32, nb) == 12345.0) and np.all(d_ok.download(np.int32, nb) == -7)

    info = np.zeros((n_seg, bps, K), np.uint8)
    d_info = om.DeviceBuffer(info.nbytes).upload(info)
    seg_bits = bps * 3 * K + 8
    d_coded = om.DeviceBuffer(n_seg * seg_bits).upload(np.full(n_seg * seg_bits, POISON, np.uint8))
    U, P = om.BITS_UNPACKED, om.BITS_PACKED
    for kw in (dict(K=44), dict(seg_bits=bps * 3 * K - 1), dict(n_seg=-1), dict(bps=-1), dict(info_mode=om.BITS_NONE),
               dict(coded_mode=7), dict(coded_mode=P, seg_bits=bps * 3 * K + 4), dict(n_seg=2 ** 31, bps=2)):
        a = dict(n_seg=n_seg, bps=bps, K=K, seg_bits=seg_bits, info_mode=U, coded_mode=U)
        a.update(kw)
        with pytest.raises(ValueError):
            tx0.tbcc_encode_frames(d_info, a["n_seg"], a["bps"], a["K"], d_coded, a["seg_bits"], info_mode=a["info_mode"],
                                   coded_mode=a["coded_mode"])
    tx0.tbcc_encode_frames(d_info, 0, bps, K, d_coded, seg_bits)            # no-op
    assert np.all(d_coded.download(np.uint8, n_seg * seg_bits) == POISON)
