"""channel_kernel (csrc/tx_kernels.hip, through ofdm_channel_apply / TxEngine.channel) against tests/channel_ref.py (-m gpu): the
convolution at every frame count, tap layout, length, stride and store path, and the noise stream sample by sample.

Every output lies in a buffer from conftest.poisoned (0xFF bytes) with 64 bytes in front of and behind the frames, and every
call is followed by a look at the WHOLE buffer: whatever lies outside [f * out_stride, f * out_stride + out_len) of a frame
must still be poison.  The input's gaps and surroundings are 0xFF bytes too (NaN): a sample read from there shows in the result.

Convolution: relerr < 1e-5 against np.convolve in complex128, the suite's bar.  The store path (16-byte pair stores where a
frame's output starts on a 16-byte boundary, 8-byte stores elsewhere and for the last sample of an odd length) does not enter
the arithmetic, so the same call at another alignment must give the same bits.

Noise: the input is zero, so the output IS the noise, and every sample is compared with channel_ref.noise.  The error is that of
the hardware's float32 log2 / sqrt / sin / cos (and of the float32 result) against float64.  Measured on an MI355X over all the
noise cases of this file (profiles/channel_noise_error.txt holds the figure of each case): max |device - reference| / sigma is
2.0e-7 .. 7.5e-7 in the three-frame cases and 7.75e-7 over the 2 097 667 samples of the long frame.  NOISE_BAR = 4e-6 is four
times the largest, rounded up to one digit (the ceiling set for it was 1e-3).  Each of the faults this file is there for (a word
used twice, radians for revolutions, a pair drawing the same words twice, the frame or the seed's upper half missing from the
counter) moves samples by O(sigma).

The grid-stride loop: a stride shorter than the grid repeats pairs with the same values, which no comparison can see.  The long
frame is therefore also timed on the device: 0.010 .. 0.014 ms as it is, 7.7 ms with `pr += blockDim.x`; ONE_PASS_MS = 0.5 is
16.8 MB of output at 34 GB/s, 1/200 of the memory's rate.

Not reached: the upper word of the pair counter (p >> 32) needs 2^33 samples in one frame, 64 GiB of output."""
import numpy as np
import pytest

import channel_ref as cr
from conftest import poisoned, relerr
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
NOISE_BAR = 4e-6                            # x sigma; see the module docstring
GUARD = 64                                  # bytes; a multiple of 16, so the guard does not change the alignment
LONG = 2 * 4096 * 256 + 515                 # launch_channel caps the grid at 4096 x 256 pairs: the first length that loops
ONE_PASS_MS = 0.5                           # device time of the long noisy frame; see the module docstring
NAN = np.complex64(complex(np.nan, np.nan))


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
def tx(om, torch):
    """any transmitter handle serves the channel (it reads buffers, not the handle's numerology)"""
    return om.TxEngine(64, 16, 62, 60)


def crandn(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def random_taps(rng, n_taps, rows=None):
    """complex taps of norm 1: [n_taps], or `rows` distinct rows of them"""
    t = crandn(rng, rows or 1, n_taps).astype(np.complex128)
    t = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.complex64)
    return t if rows else t[0]


class Out:
    """n_frames rows of out_stride samples, `lead` samples behind a 16-byte boundary, in a poisoned buffer with a guard on
    either side.  read() -> [n_frames][out_len] after asserting that every other byte of the buffer is still poison."""

    def __init__(self, om, n_frames, out_stride, out_len, lead=0):
        self.shape = (int(n_frames), int(out_stride), int(out_len))
        self.lo = GUARD + 8 * lead
        self.total = self.lo + 8 * n_frames * out_stride + GUARD
        self.buf = poisoned(om, self.total)
        assert self.buf.data_ptr() % 16 == 0
        self.addr = self.buf.data_ptr() + self.lo

    def read(self):
        n_frames, out_stride, out_len = self.shape
        raw = self.buf.download(np.uint8, self.total)
        body = raw[self.lo:self.lo + 8 * n_frames * out_stride].reshape(n_frames, 8 * out_stride)
        stray = [int((raw[:self.lo] != 0xFF).sum()), int((body[:, 8 * out_len:] != 0xFF).sum()),
                 int((raw[self.lo + 8 * n_frames * out_stride:] != 0xFF).sum())]
        assert stray == [0, 0, 0], "bytes written in front of / between / behind the frames: %s" % stray
        return np.ascontiguousarray(body[:, :8 * out_len]).view(np.complex64).reshape(n_frames, out_len)

    def untouched(self):
        return bool(np.all(self.buf.download(np.uint8, self.total) == 0xFF))


def upload_rows(om, rows, stride):
    """[n][len] complex64 -> device [n][stride], everything outside the rows NaN (0xFF bytes), 64 such bytes behind the last"""
    rows = np.atleast_2d(rows)
    n, length = rows.shape
    host = np.full((n * stride + GUARD // 8,), NAN, np.complex64)
    host[:n * stride].reshape(n, stride)[:, :length] = rows
    return om.DeviceBuffer(host.nbytes).upload(host)


def channel(om, tx, x, taps, out_len, in_gap=0, out_gap=0, lead=0, noise_var=0.0, seed=0, stream=None):
    """x [n_frames][in_len], taps [n_taps] or [n_frames][n_taps] -> the device's [n_frames][out_len], whole buffer checked"""
    x = np.atleast_2d(x)
    n_frames, in_len = x.shape
    taps = np.asarray(taps, np.complex64)
    d_x = upload_rows(om, x, in_len + in_gap)
    d_t = upload_rows(om, taps, taps.shape[-1])
    out = Out(om, n_frames, out_len + out_gap, out_len, lead)
    tx.channel(d_x, n_frames, in_len + in_gap, in_len, d_t, taps.shape[-1], out.addr, out_len + out_gap, out_len,
               noise_var=noise_var, seed=seed, per_frame_taps=taps.ndim == 2, stream=stream)
    return out.read()


def out_lens(in_len, n_taps):
    full = in_len + n_taps - 1
    return sorted({n for n in (1, 2, in_len - 3, in_len, full - 1, full) if 1 <= n <= full})


# ------------------------------------------------------------------------------------------ convolution, no noise
@pytest.mark.parametrize("out_gap", (0, 3), ids=("gap0", "gap3"))
@pytest.mark.parametrize("per_frame", (False, True), ids=("shared", "perframe"))
@pytest.mark.parametrize("n_frames", (1, 3, 5))
def test_convolution_equals_reference(om, tx, n_frames, per_frame, out_gap):
    """in_len 1, 2, 7 (shorter than 9 taps), 300, 301  x  1, 2, 9 taps  x  every out_len of out_lens (1, 2, shorter than the input,
    the input's, the full convolution and one less: odd and even)  x  in_stride = in_len, in_len + 5.  With out_gap = 3 an even
    out_len gives an odd stride: frames 1 and 3 then start 8 bytes off the 16-byte grid."""
    rng = np.random.default_rng(1000 + 10 * n_frames + per_frame)
    n_calls = 0
    for in_len in (1, 2, 7, 300, 301):
        x = crandn(rng, n_frames, in_len)
        for n_taps in (1, 2, 9):
            taps = random_taps(rng, n_taps, n_frames if per_frame else None)
            for out_len in out_lens(in_len, n_taps):
                ref = cr.conv(x, taps, out_len)
                for in_gap in (0, 5):
                    what = "in_len %d, %d taps, out_len %d, in_gap %d" % (in_len, n_taps, out_len, in_gap)
                    y = channel(om, tx, x, taps, out_len, in_gap=in_gap, out_gap=out_gap)
                    for f in range(n_frames):
                        assert relerr(y[f], ref[f]) < TOL, "%s, frame %d: %.3g" % (what, f, relerr(y[f], ref[f]))
                    if per_frame and n_frames > 1:
                        # a kernel that gave every frame the taps of frame 0 would be right in frame 0 only
                        ref0 = cr.conv(x, taps[0], out_len)
                        for f in range(1, n_frames):
                            assert relerr(ref[f], ref0[f]) > 1e-2 and relerr(y[f], ref0[f]) > 1e-2, what
                    n_calls += 1
    assert n_calls == 128


def test_convolution_with_the_reference_taps_equals_the_oracle(om, tx):
    """the five taps of the reference's channel, normalised, shared by three frames of odd length at an odd stride"""
    rng = np.random.default_rng(5)
    taps = (orc.REF_TAPS / np.linalg.norm(orc.REF_TAPS)).astype(np.complex64)
    x = crandn(rng, 3, 301)
    y = channel(om, tx, x, taps, 305, in_gap=5, out_gap=0)
    assert relerr(y, cr.conv(x, taps, 305)) < TOL
    for f in range(3):
        assert relerr(y[f], orc.channel_apply(x[f], orc.REF_TAPS, 64)[:305]) < TOL


@pytest.mark.parametrize("noise_var", (0.0, 0.25), ids=("clean", "noisy"))
def test_store_path_does_not_change_a_bit(om, tx, noise_var):
    """aligned rows (even stride on a 16-byte boundary), an odd stride (frames 1 and 3 misaligned), and the base one sample off
    the boundary with an even stride (every frame misaligned) and an odd one (frames 0, 2, 4): the same values element for element"""
    rng = np.random.default_rng(6)
    for in_len in (300, 301):
        x = crandn(rng, 5, in_len)
        taps = random_taps(rng, 9, 5)
        for out_len in (1, 2, in_len - 3, in_len, in_len + 7, in_len + 8):
            even, odd = 2 + out_len % 2, 1 + out_len % 2
            kw = dict(noise_var=noise_var, seed=77)
            aligned = channel(om, tx, x, taps, out_len, out_gap=even, **kw)
            assert relerr(aligned, cr.conv(x, taps, out_len) + (cr.noise(77, 5, out_len, noise_var) if noise_var else 0)) < TOL
            for gap, lead in ((odd, 0), (even, 1), (odd, 1)):
                y = channel(om, tx, x, taps, out_len, out_gap=gap, lead=lead, **kw)
                assert np.array_equal(y, aligned), "out_len %d, stride %d, lead %d" % (out_len, out_len + gap, lead)


def test_long_frame_where_the_grid_loops(om, tx):
    """one frame of 2 * 4096 * 256 + 515 samples, one tap: every thread of the capped grid takes a second pair or none, the last
    pair is half a pair.  Every sample compared; once on the boundary, once a sample off it."""
    rng = np.random.default_rng(7)
    x = crandn(rng, 1, LONG)
    taps = random_taps(rng, 1)
    ref = cr.conv(x, taps, LONG)
    y = channel(om, tx, x, taps, LONG, out_gap=1)
    assert relerr(y, ref) < TOL
    assert np.max(np.abs(y - ref) / np.abs(ref)) < TOL                     # one product per sample: each to float32 rounding
    assert np.array_equal(channel(om, tx, x, taps, LONG, out_gap=1, lead=1), y)


def test_long_frame_is_one_pass_over_the_pairs(om, tx, torch):
    """A loop whose stride is not the whole grid computes every pair again in every workgroup behind its owner: the same values,
    so no comparison sees it, only the clock (4096 workgroups: ~2000 times the work).  Device time between two events around the
    call, the best of three."""
    d_x = upload_rows(om, np.zeros((1, LONG), np.complex64), LONG)
    d_t = upload_rows(om, np.ones(1, np.complex64), 1)
    out = Out(om, 1, LONG + 1, LONG)
    s = torch.cuda.Stream()
    ms = []
    with torch.cuda.stream(s):
        for _ in range(4):                                                  # the first call is not timed
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            tx.channel(d_x, 1, LONG, LONG, d_t, 1, out.addr, LONG + 1, LONG, noise_var=0.25, seed=1, stream=s.cuda_stream)
            t1.record(s)
            s.synchronize()
            ms.append(t0.elapsed_time(t1))
    print("long noisy frame: %s ms" % ", ".join("%.3f" % t for t in ms))
    out.read()
    assert min(ms[1:]) < ONE_PASS_MS


def test_nothing_to_do_is_ok_and_writes_nothing(om, tx):
    rng = np.random.default_rng(8)
    d_x = upload_rows(om, crandn(rng, 3, 16), 16)
    d_t = upload_rows(om, random_taps(rng, 2), 2)
    out = Out(om, 3, 16, 16)
    for nv in (0.0, 0.25):
        tx.channel(d_x, 3, 16, 16, d_t, 2, out.addr, 16, 0, noise_var=nv, seed=1)                  # out_len = 0
        tx.channel(d_x, 0, 16, 16, d_t, 2, out.addr, 16, 16, noise_var=nv, seed=1)                 # n_frames = 0
        tx.channel(d_x, 3, 16, 0, d_t, 2, out.addr, 16, 0, noise_var=nv, seed=1)                   # in_len = out_len = 0
    assert out.untouched()


def test_65535_frames_are_accepted(om, tx):
    """the largest grid in y; two samples and one tap per frame"""
    rng = np.random.default_rng(9)
    x = crandn(rng, 65535, 2)
    taps = random_taps(rng, 1)
    y = channel(om, tx, x, taps, 2)
    assert relerr(y, cr.conv(x, taps, 2)) < TOL


def test_argument_errors_leave_the_output_untouched(om, tx):
    from ofdm_mi355x._lib import OFDM_ERR_INVALID, check, ptr
    rng = np.random.default_rng(10)
    n_frames, in_len, n_taps = 3, 16, 4
    d_x = upload_rows(om, crandn(rng, 1, 1 << 17), 1 << 17)                # each large enough for every call below, were it to run
    d_t = upload_rows(om, random_taps(rng, 1 << 17), 1 << 17)
    out = Out(om, 1, 1 << 17, 1 << 17)
    ok = dict(n_frames=n_frames, in_stride=in_len, in_len=in_len, n_taps=n_taps, noise_var=0.0, out_stride=in_len, out_len=in_len)
    bad = (dict(n_taps=0), dict(noise_var=-1e-3), dict(out_len=in_len + n_taps, out_stride=in_len + n_taps), dict(in_stride=in_len - 1),
           dict(out_stride=in_len - 1), dict(n_frames=65536, in_len=2, in_stride=2, out_len=2, out_stride=2, n_taps=1))
    for change in bad:
        a = dict(ok, **change)
        for per_frame in (0, 1):
            rc = tx.lib.ofdm_channel_apply(tx._h, ptr(d_x), a["n_frames"], a["in_stride"], a["in_len"], ptr(d_t), a["n_taps"], per_frame,
                                           a["noise_var"], 1, ptr(out.addr), a["out_stride"], a["out_len"], None)
            assert rc == OFDM_ERR_INVALID, (change, rc)
            with pytest.raises(ValueError):
                check(rc)
    with pytest.raises(ValueError):
        tx.channel(d_x, n_frames, in_len, in_len, d_t, 0, out.addr, in_len, in_len)
    assert out.untouched()


# ------------------------------------------------------------------------------------------ noise
def noise_layouts(out_len):
    """(name, out_gap, lead): rows on the 16-byte grid; an odd stride (frame 1 off it); the base one sample off it (frames 0, 2)"""
    even, odd = 2 - out_len % 2, 1 + out_len % 2
    return (("aligned", even, 0), ("odd stride", odd, 0), ("base + 8", even, 1))


@pytest.mark.parametrize("noise_var", (0.25, 1e-6))
@pytest.mark.parametrize("seed", (0, 1234, (7 << 32) | 5), ids=("seed0", "seed1234", "seed7:5"))
@pytest.mark.parametrize("out_len", (1, 2, 1001, 4096))
def test_noise_equals_reference_sample_by_sample(om, tx, out_len, seed, noise_var):
    ref = cr.noise(seed, 3, out_len, noise_var)
    sig = float(cr.sigma(noise_var))
    x = np.zeros((3, out_len), np.complex64)
    got = {}
    for name, gap, lead in noise_layouts(out_len):
        got[name] = channel(om, tx, x, np.ones(1, np.complex64), out_len, out_gap=gap, lead=lead, noise_var=noise_var, seed=seed)
    err = float(np.max(np.abs(got["aligned"] - ref)) / sig)
    print("noise error: out_len %4d seed %#11x noise_var %-6g frames 3: max |device - reference| / sigma = %.3g" % (out_len, seed, noise_var, err))
    assert err < NOISE_BAR
    for name in ("odd stride", "base + 8"):
        assert np.array_equal(got[name], got["aligned"]), name


def test_long_noise_frame_equals_reference_and_has_its_statistics(om, tx):
    """the pair index beyond the capped grid (a second trip of the loop must go on counting pairs, not restart), and the bounds of
    tests/test_channel_ref_host.py on the device's own samples"""
    nv, seed = 0.25, 1234
    ref = cr.noise(seed, 1, LONG, nv)
    y = channel(om, tx, np.zeros((1, LONG), np.complex64), np.ones(1, np.complex64), LONG, out_gap=1, noise_var=nv, seed=seed)
    err = float(np.max(np.abs(y - ref)) / float(cr.sigma(nv)))
    print("noise error: out_len %d seed %#11x noise_var %-6g frames 1: max |device - reference| / sigma = %.3g" % (LONG, seed, nv, err))
    st = cr.statistics(y[0], nv)
    print("statistics of the device's frame: %s" % ", ".join("%s %.3g" % kv for kv in st.items()))
    assert err < NOISE_BAR
    assert not cr.within_bounds(st), cr.within_bounds(st)


def test_signal_plus_noise_equals_the_sum_of_the_references(om, tx):
    rng = np.random.default_rng(12)
    x = crandn(rng, 3, 301)
    taps = random_taps(rng, 9, 3)
    seed = (7 << 32) | 5
    ref = cr.conv(x, taps, 305) + cr.noise(seed, 3, 305, 0.25)
    for lead in (0, 1):
        y = channel(om, tx, x, taps, 305, in_gap=5, lead=lead, noise_var=0.25, seed=seed)
        assert relerr(y, ref) < TOL
    assert relerr(channel(om, tx, x, taps, 305, in_gap=5), ref) > 0.1       # (the noise is most of it)


def test_graph_capture_equals_eager(om, tx, torch):
    """one noisy three-frame call with per-frame taps: captured, replayed twice, byte for byte the eager result"""
    rng = np.random.default_rng(13)
    n_frames, in_len, n_taps, out_len, out_stride = 3, 301, 9, 305, 308
    d_x = upload_rows(om, crandn(rng, n_frames, in_len), in_len)
    d_t = upload_rows(om, random_taps(rng, n_taps, n_frames), n_taps)
    out = Out(om, n_frames, out_stride, out_len, lead=1)
    poison = np.full(out.total, 0xFF, np.uint8)
    s = torch.cuda.Stream()

    def call(stream):
        tx.channel(d_x, n_frames, in_len, in_len, d_t, n_taps, out.addr, out_stride, out_len, noise_var=0.25, seed=1234,
                   per_frame_taps=True, stream=stream)

    with torch.cuda.stream(s):
        call(s.cuda_stream)
    s.synchronize()
    eager = out.read().copy()
    assert np.all(np.isfinite(eager.view(np.float32)))
    out.buf.upload(poison)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    assert out.untouched()                                                  # capture enqueues nothing
    for _ in range(2):
        out.buf.upload(poison)
        g.replay()
        torch.cuda.synchronize()
        assert out.read().tobytes() == eager.tobytes()
