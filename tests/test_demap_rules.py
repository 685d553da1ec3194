"""Every hard-decision path of the de-mappers, input by input, at its decision edges.

The fused de-mapper decides with hand-written v_cmp / v_addc chains (pack4 / pack2 in csrc/demap_hard.hpp) next to the plain
C++ rule hard_bits<MOD>; the standalone de-mapper (ofdm_demap) with hard_bits through word stores.  Random or noisy symbols
almost never land on a threshold, so the inputs here are planted (tests/demap_corpus.py): thresholds and their neighbours
at 1 and 2 ulps, +-0, denormals, FLT_MIN / FLT_MAX, values whose four-way product overflows, inf and NaN.

Expected bits: a symbol with both coordinates finite decides exactly like orc.demap_hard (QPSK ties through its literal
restatement of BitRecovery).  The reference defines no bits for a non-finite coordinate, so no oracle assertion is made
there: every variant must then agree with the device's own hard_bits<MOD>, which the standalone de-mapper also uses.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import demap_corpus as dc
from conftest import PKG, ROOT, poisoned, relerr
from oracle import ofdm_oracle as orc

SRC = os.path.join(ROOT, "tests", "device", "demap_rules.hip")
CSRC = os.path.join(PKG, "csrc")
# csrc/Makefile's flags: the inline assembly must run as it does in the library
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]
TOL = 1e-5


def _compile(out):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.run(["hipcc"] + FLAGS + ["-I", CSRC, "-o", out, SRC], check=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("demap_rules") / "demap_rules"))


def test_demap_rules_harness_compiles_for_gfx950(tmp_path):
    """pack4 / pack2 / hard_bits / store_bits of every modulation instantiated and assembled for gfx950: broken inline asm or
    templates fail here, without a GPU."""
    exe = _compile(str(tmp_path / "demap_rules"))
    assert os.path.getsize(exe) > 0


def run_harness(exe, z, bits, workdir):
    """-> {variant: uint8[n, bits]} from one device run of the harness on the symbols z"""
    z = np.ascontiguousarray(z, np.complex64)
    assert z.size % 4 == 0
    fin = os.path.join(workdir, "sym_%d.bin" % bits)
    outdir = os.path.join(workdir, "out_%d" % bits)
    os.makedirs(outdir, exist_ok=True)
    z.tofile(fin)
    r = subprocess.run([exe, str(bits), fin, outdir], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names = r.stdout.split()
    want = {"hard", "pack4_asm", "pack4_c", "pack2_asm", "pack2_c", "store_u", "store_pair_u"}
    if bits % 2 == 0:
        want |= {"store_p_asm", "store_p_c"}
    assert set(names) == want
    return {nm: np.fromfile(os.path.join(outdir, nm + ".bin"), np.uint8).reshape(z.size, bits) for nm in names}


def _mismatch(z, got, want, rows):
    bad = np.nonzero(rows & (got != want).any(axis=1))[0]
    return "%d symbols, first: %s" % (bad.size, ", ".join("%r -> %s want %s" % (complex(z[i]), got[i].tolist(), want[i].tolist())
                                                        for i in bad[:6]))


@pytest.fixture(scope="module")
def device_rules(harness, tmp_path_factory):
    """the harness run once per modulation on its corpus: {bits: (z, {variant: bits})}"""
    wd = str(tmp_path_factory.mktemp("demap_rules_run"))
    out = {}
    for bits in dc.MODS:
        z = dc.corpus(bits)
        out[bits] = (z, run_harness(harness, z, bits, wd))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [1, 2, 4, 6])
def test_fused_decision_variants_match_oracle_at_edges(device_rules, bits):
    z, res = device_rules[bits]
    want = dc.expected_bits(z, bits)
    fin = dc.finite(z)
    hard = res["hard"]
    bad = []
    for name, got in res.items():
        if not np.array_equal(got[fin], want[fin]):
            bad.append("%s<%d> vs orc.demap_hard: %s" % (name, bits, _mismatch(z, got, want, fin)))
        # non-finite coordinates: no reference bits exist; every variant decides like hard_bits
        if not np.array_equal(got[~fin], hard[~fin]):
            bad.append("%s<%d> vs hard_bits on non-finite symbols: %s" % (name, bits, _mismatch(z, got, hard, ~fin)))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_qpsk_tie_next_to_overflowing_or_nan_symbol(device_rules):
    """The QPSK tie pre-check multiplies the coordinates of a group: (1e20, 1e20) next to 0+0j gives inf * 0 = NaN, and NaN next
    to an exact zero gives NaN.  The zero must still take the literal tie path: BitRecovery's (1, 0)."""
    z, res = device_rules[2]
    groups = np.stack([z.real, z.imag], -1).reshape(-1, 8)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.prod(groups, axis=1, dtype=np.float32)
    zero = z == 0
    hit = np.repeat(np.isnan(prod), 4) & zero
    assert hit.sum() > 100                                   # the corpus plants such groups
    want = dc.expected_bits(z, 2)
    assert (want[hit] == [1, 0]).all()
    bad = ["%s: %s" % (name, _mismatch(z, got, want, hit)) for name, got in res.items() if not np.array_equal(got[hit], want[hit])]
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------ ofdm_demap through the C ABI
@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


@pytest.fixture(scope="module")
def rx(om):
    return om.RxEngine(1, 64, 16, 62, (1, 3), 60, 100)


def _download_at(om, buf, byte_off, dtype, count):
    """count elements of dtype starting byte_off bytes into a DeviceBuffer"""
    out = np.empty(count, dtype=dtype)
    assert byte_off + out.nbytes <= buf.nbytes
    lib = om._lib.load()
    om._lib.check(lib.ofdm_device_synchronize(buf.device))
    om._lib.check(lib.ofdm_memcpy_d2h(buf.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(buf.data_ptr() + byte_off),
                                      out.nbytes))
    return out


def _oracle_soft(z, bits):
    if bits == 2:
        return orc.bit_recovery(z)[1:]
    return orc.soft_demap_qam(z, dc.MODS[bits])[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [1, 2, 4, 6])
def test_ofdm_demap_hard_bits_on_planted_corpus(om, rx, device_rules, bits):
    """Standalone de-mapper on the planted corpus, hard only and hard + soft: finite symbols decide like orc.demap_hard,
    non-finite ones like the fused path's hard_bits (the reference defines no bits there)."""
    z, res = device_rules[bits]
    n = z.size
    want = dc.expected_bits(z, bits)
    fin = dc.finite(z)
    want[~fin] = res["hard"][~fin]
    d_z = om.DeviceBuffer(z.nbytes).upload(z)
    softs = [None] if bits == 1 else [None, "both"]
    for soft in softs:
        d_h = poisoned(om, n * bits)
        d_0 = om.DeviceBuffer(n * bits * 4) if soft else None
        d_1 = om.DeviceBuffer(n * bits * 4) if soft else None
        rx.demap(d_z, n, dc.MODS[bits], d_h, d_0, d_1)
        got = d_h.download(np.uint8, n * bits).reshape(n, bits)
        assert np.array_equal(got, want), "soft=%s: %s" % (soft, _mismatch(z, got, want, np.ones(n, bool)))


def _soft_corpus(bits, seed=1, n_noisy=4000):
    """finite planted symbols with coordinates below 1e18, plus n_noisy noisy constellation points, shuffled"""
    z = dc.corpus(bits, seed=seed, shuffles=1)
    z = z[dc.finite(z) & (np.maximum(np.abs(z.real), np.abs(z.imag)) < 1e18)]
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, n_noisy * bits)
    noisy = (orc.map_bits(b, dc.MODS[bits]) + 0.1 * (rng.standard_normal(n_noisy) + 1j * rng.standard_normal(n_noisy)))
    z = np.concatenate([z, noisy.astype(np.complex64)])
    return z[rng.permutation(z.size)]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [2, 4, 6])
def test_ofdm_demap_soft_metrics_on_planted_corpus(om, rx, bits):
    """Soft metrics on finite planted symbols vs orc.bit_recovery (QPSK) / orc.soft_demap_qam, 1e-5 norm-relative.
    Limit: coordinates stay below 1e18.  The device forms the nearest-point distance in float32 (ex*ex in demap_dmin), which
    overflows above ~1.8e19 where the fp64 oracle does not; sigma -- and every metric -- then differs."""
    z = _soft_corpus(bits)
    n = z.size
    s0, s1 = _oracle_soft(z, bits)
    d_z = om.DeviceBuffer(z.nbytes).upload(z)
    d_h, d_0, d_1 = om.DeviceBuffer(n * bits), om.DeviceBuffer(n * bits * 4), om.DeviceBuffer(n * bits * 4)
    rx.demap(d_z, n, dc.MODS[bits], d_h, d_0, d_1)
    g0, g1 = d_0.download(np.float32, n * bits), d_1.download(np.float32, n * bits)
    assert relerr(g0, s0) < TOL and relerr(g1, s1) < TOL
    # the same at the scale of the ordinary symbols (|coordinates| < 10), which the huge ones dwarf in the line above
    small = np.repeat(np.maximum(np.abs(z.real), np.abs(z.imag)) < 10, bits)
    assert relerr(g0[small], s0[small]) < TOL and relerr(g1[small], s1[small]) < TOL
    assert np.array_equal(d_h.download(np.uint8, n * bits), orc.demap_hard(z, dc.MODS[bits]))


LENGTHS = [1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 40001, 40002, 40003]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [1, 2, 4, 6])
def test_ofdm_demap_lengths_alignments_and_output_subsets(om, rx, bits):
    """launch_demap picks its paths by length and alignment: 4-symbol words of pass 1 and their scalar tail, the 2-symbol QPSK
    pass 2, the 128-symbol tiles of the 64-QAM soft kernel; a symbol pointer 8 bytes past a 16-byte boundary or an odd hard
    pointer forces the scalar paths.  Every combination must give the oracle's bits (and metrics), write nothing past n, and a
    single soft array must equal the matching array of the two-array call bit for bit; hard bits must not depend on whether
    soft outputs were requested."""
    mod = dc.MODS[bits]
    zall = _soft_corpus(bits, seed=bits, n_noisy=30000)
    assert zall.size >= max(LENGTHS)
    slack = 64
    nmax = max(LENGTHS)
    d_z = om.DeviceBuffer(nmax * 8 + slack)
    d_h = om.DeviceBuffer(nmax * bits + slack)
    d_s = [om.DeviceBuffer(nmax * bits * 4 + slack) for _ in range(2)]
    soft_sets = [(False, False)] if bits == 1 else [(False, False), (True, False), (False, True), (True, True)]
    for n in LENGTHS:
        z = zall[:n]
        want_h = orc.demap_hard(z, mod)
        want_s = _oracle_soft(z, bits) if bits != 1 else None
        for zoff, hoff in ((0, 0), (8, 0), (0, 1), (8, 1)):
            soff = zoff                                         # soft arrays follow the symbol pointer's alignment
            d_z.upload(np.concatenate([np.zeros(zoff // 8, np.complex64), z]))
            soft = {}
            for s0, s1 in soft_sets:
                d_h.upload(np.full(d_h.nbytes, 0xFF, np.uint8))
                for d in d_s:
                    d.upload(np.full(d.nbytes, 0xFF, np.uint8))
                rx.demap(d_z.data_ptr() + zoff, n, mod, d_h.data_ptr() + hoff, d_s[0].data_ptr() + soff if s0 else None,
                         d_s[1].data_ptr() + soff if s1 else None)
                hb = d_h.download(np.uint8, d_h.nbytes)
                tag = "n=%d zoff=%d hoff=%d soft=%s" % (n, zoff, hoff, (s0, s1))
                assert np.array_equal(hb[hoff:hoff + n * bits], want_h), tag
                assert (hb[:hoff] == 0xFF).all() and (hb[hoff + n * bits:] == 0xFF).all(), tag + ": hard write outside [0, n)"
                for k, on in enumerate((s0, s1)):
                    raw = d_s[k].download(np.uint8, d_s[k].nbytes)
                    lo, hi = soff, soff + n * bits * 4
                    if not on:
                        assert (raw == 0xFF).all(), tag + ": soft%d written though not requested" % k
                        continue
                    assert (raw[:lo] == 0xFF).all() and (raw[hi:] == 0xFF).all(), tag + ": soft%d write outside [0, n)" % k
                    soft[(s0, s1, k)] = raw[lo:hi].copy()
                    assert relerr(soft[(s0, s1, k)].view(np.float32), want_s[k]) < TOL, tag
            if bits != 1:
                assert np.array_equal(soft[(True, False, 0)], soft[(True, True, 0)]), "n=%d zoff=%d: soft0 alone" % (n, zoff)
                assert np.array_equal(soft[(False, True, 1)], soft[(True, True, 1)]), "n=%d zoff=%d: soft1 alone" % (n, zoff)


@pytest.mark.gpu
def test_ofdm_demap_argument_errors_and_empty_call(om, rx):
    d_z = om.DeviceBuffer(64).upload(np.ones(8, np.complex64))
    d_h = poisoned(om, 64)
    d_s = om.DeviceBuffer(256)
    with pytest.raises(ValueError):
        rx.demap(d_z, 8, "BPSK", d_h, d_s, None)
    with pytest.raises(ValueError):
        rx.demap(d_z, 8, "BPSK", d_h, None, d_s)
    with pytest.raises(ValueError):
        rx.demap(d_z, -1, "QPSK", d_h)
    for bad in (0, 3, 5, 8):
        with pytest.raises(ValueError):
            rx.demap(d_z, 8, bad, d_h)
    d_0, d_1 = poisoned(om, 256), poisoned(om, 256)
    for mod in ("QPSK", "16QAM", "64QAM"):
        rx.demap(d_z, 0, mod, d_h, d_0, d_1)
    rx.demap(d_z, 0, "BPSK", d_h)
    for d in (d_h, d_0, d_1):
        assert (d.download(np.uint8, d.nbytes) == 0xFF).all()


def _qam_dmin64(z, lv):
    """nearest-point distance per symbol in fp64 (the oracle's definition, soft_demap_qam)"""
    zz = z.astype(np.complex128)
    ex = np.min(np.abs(zz.real[:, None] - lv[None, :]), axis=1)
    ey = np.min(np.abs(zz.imag[:, None] - lv[None, :]), axis=1)
    return np.hypot(ex, ey)


@pytest.mark.gpu
def test_ofdm_demap_past_the_pass2_grid_cap(om, rx):
    """16-QAM, n = 2^26 + 5, hard + soft.  Pass 2 runs at most 262 144 workgroups x 256 lanes = 2^26 symbols per trip of its
    grid-stride loop: the last 5 symbols are the only ones of a second trip.  sigma is computed on the host in fp64 from the
    whole buffer, in chunks; hard bits are compared everywhere, metrics around index 2^26 and on a sample of the rest."""
    bits, mod = 4, "16QAM"
    n = (1 << 26) + 5
    lv, _ = orc.qam_levels(mod)
    rng = np.random.default_rng(26)
    z = np.empty(n, np.complex64)
    CH = 1 << 22
    for s in range(0, n, CH):
        m = min(CH, n - s)
        q = rng.integers(0, 4, (2, m))
        z.real[s:s + m] = lv[q[0]] + rng.standard_normal(m, dtype=np.float32) * np.float32(0.08)
        z.imag[s:s + m] = lv[q[1]] + rng.standard_normal(m, dtype=np.float32) * np.float32(0.08)
    dsum = 0.0
    for s in range(0, n, CH):
        dsum += float(np.sum(_qam_dmin64(z[s:s + CH], lv)))
    sigma = 0.7071067811865476 * dsum / n
    d_z = om.DeviceBuffer(z.nbytes).upload(z)
    d_h = om.DeviceBuffer(n * bits)
    d_0, d_1 = om.DeviceBuffer(n * bits * 4), om.DeviceBuffer(n * bits * 4)
    rx.demap(d_z, n, mod, d_h, d_0, d_1)
    hb = d_h.download(np.uint8, n * bits)
    for s in range(0, n, CH):
        assert np.array_equal(hb[s * bits:(s + CH) * bits], orc.demap_hard(z[s:s + CH], mod)), "hard bits at %d" % s
    del hb
    starts = sorted(set([(1 << 26) - 4096, 0] + [int(x) for x in rng.integers(0, n - 4096, 24)]))
    for s in starts:
        m = min(4096 + 5, n - s)
        w = z[s:s + m]
        _, r0, r1 = orc.soft_demap_qam(w, mod)
        sig_w = 0.7071067811865476 * np.mean(_qam_dmin64(w, lv))
        r0, r1 = r0 * (sig_w / sigma) ** 2, r1 * (sig_w / sigma) ** 2          # the window's metrics at the buffer's sigma
        g0 = _download_at(om, d_0, s * bits * 4, np.float32, m * bits)
        g1 = _download_at(om, d_1, s * bits * 4, np.float32, m * bits)
        assert relerr(g0, r0) < TOL and relerr(g1, r1) < TOL, "metrics at %d" % s
    tail = _download_at(om, d_0, (n - 5) * bits * 4, np.float32, 5 * bits)
    assert np.isfinite(tail).all() and (tail <= 0).all()
