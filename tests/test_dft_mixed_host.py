"""csrc/dft_mixed.hpp executed lane by lane on the CPU (host compilation by hipcc, no GPU): every one of the 137 plans
M = 2^a 3^b 5^c <= 4096, both directions, against numpy.fft in fp64."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr

SRC = os.path.join(ROOT, "tests", "host", "dft_mixed_host_test.cpp")
SIZES = sorted(2 ** a * 3 ** b * 5 ** c for a in range(13) for b in range(8) for c in range(6) if 2 ** a * 3 ** b * 5 ** c <= 4096)
SAN_SIZES = [1, 5, 12, 75, 1200, 2187, 3125, 4096]


def _build(tmp_path_factory, name, extra):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp(name) / "dft_mixed_host_test")
    subprocess.run(["hipcc", "-O2", "-std=c++17", "-fno-slp-vectorize"] + extra + ["-o", out, SRC], check=True)
    return out


def _run(exe, tmp_path, sizes, x_of):
    """-> {M: (forward, inverse, plan line as ints)}"""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([x_of[m] for m in sizes]).astype(np.complex64).tofile(fin)
    r = subprocess.run([exe, fin, fout] + [str(m) for m in sizes], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(fout, dtype=np.complex64)
    lines = [[int(t) for t in ln.split()] for ln in r.stdout.strip().splitlines()]
    res, at = {}, 0
    for m, ln in zip(sizes, lines):
        res[m] = (out[at:at + m], out[at + m:at + 2 * m], ln)
        at += 2 * m
    assert at == out.size
    return res


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(2187)
    return {m: (rng.standard_normal(m) + 1j * rng.standard_normal(m)).astype(np.complex64) for m in SIZES}


@pytest.fixture(scope="module")
def results(tmp_path_factory, inputs):
    exe = _build(tmp_path_factory, "dftmixed", [])
    return _run(exe, tmp_path_factory.mktemp("dftmixed_io"), SIZES, inputs)


def test_there_are_137_sizes():
    assert len(SIZES) == 137 and SIZES[0] == 1 and SIZES[-1] == 4096


def test_every_plan_matches_numpy_in_both_directions(results, inputs):
    worst = (0.0, 0, "")
    for m in SIZES:
        x = inputs[m].astype(np.complex128)
        fwd, inv, _ = results[m]
        for what, got, ref in (("forward", fwd, np.fft.fft(x) / np.sqrt(m)), ("inverse", inv, np.fft.ifft(x) * np.sqrt(m))):
            e = relerr(got, ref)
            worst = max(worst, (e, m, what))
            assert e < 1e-6, (m, what, e)
    print("worst error %.3g at M = %d (%s)" % worst)


def test_plan_radices_multiply_to_m(results):
    for m in SIZES:
        M, n_pass, lanes, rpg, pad, row_elems = results[m][2][:6]
        radix = results[m][2][6:]
        assert M == m and len(radix) == n_pass and set(radix) <= {2, 3, 4, 5}
        assert int(np.prod(radix, dtype=np.int64)) == m
        assert lanes * rpg == 256 and lanes & (lanes - 1) == 0
        assert row_elems >= m and rpg * row_elems <= 4096 + 6 * 128
        # a lane's butterflies fit the registers of the size's class (M <= 2048, or any M): ceil((M / R) / lanes) <=
        # ceil(ceil(cap / R) / 256)
        cap = 2048 if m <= 2048 else 4096
        for r in radix:
            assert -(-(m // r) // lanes) <= -(-(-(-cap // r)) // 256), (m, r)
    assert 3 in results[1200][2][6:] and 5 in results[1200][2][6:]


def test_impulse_at_index_one(tmp_path_factory, tmp_path):
    exe = _build(tmp_path_factory, "dftmixed_imp", [])
    sizes = [m for m in SIZES if m > 1]
    imp = {}
    for m in sizes:
        e = np.zeros(m, np.complex64)
        e[1] = 1
        imp[m] = e
    res = _run(exe, tmp_path, sizes, imp)
    for m in sizes:
        k = np.arange(m)
        assert relerr(res[m][0], np.exp(-2j * np.pi * k / m) / np.sqrt(m)) < 5e-7, m
        assert relerr(res[m][1], np.exp(+2j * np.pi * k / m) / np.sqrt(m)) < 5e-7, m


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path_factory, tmp_path, inputs):
    """The same stand-alone program, instrumented: a stray LDS index or register slot of a plan is an error here."""
    exe = _build(tmp_path_factory, "dftmixed_san", ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    res = _run(exe, tmp_path, SAN_SIZES, inputs)
    for m in SAN_SIZES:
        assert relerr(res[m][0], np.fft.fft(inputs[m].astype(np.complex128)) / np.sqrt(m)) < 1e-6, m
