"""The C ABI of receive diversity for DFT-spread OFDM without a GPU: the library exports the calls, the ctypes table and the
engine carry them, ofdm_mrc_despread_out has the layout a C compiler gives it, and every argument error of
ofdm_combine_despread_frames returns OFDM_ERR_INVALID with its reason before the handle is read -- so that it can be reached
here with a handle that is only an address: a block of zeroed host memory."""
import ctypes as C
import os

import pytest

NEW = ("ofdm_rx_reserve_mrc_despread", "ofdm_combine_despread_frames", "ofdm_rx_demod_frames_mrc_despread")
FIELDS = ["sym", "llr", "bits", "beta", "weight", "comb"]
ERR_INVALID = -1
GIVEN, SEG, EST = 0, 1, 2
NONE, PACKED, UNPACKED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_library_and_package_export_the_calls(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    for name in ("reserve_mrc_despread", "combine_despread_frames", "demod_frames_mrc_despread"):
        assert callable(getattr(om.RxEngine, name))
    assert [f[0] for f in _lib.MrcDespreadOut._fields_] == FIELDS
    assert (om.BITS_NONE, om.BITS_PACKED, om.BITS_UNPACKED) == (NONE, PACKED, UNPACKED)
    assert lib.ofdm_abi_version() == 1


def test_header_declares_the_block_as_c(lib, tmp_path):
    """the struct layout and the three prototypes as a C compiler sees them"""
    import shutil
    import subprocess
    from conftest import ROOT
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ofdm_mi355x.h"\n'
                   'int (*const p_reserve)(ofdm_rx*, int32_t, int32_t, int64_t) = ofdm_rx_reserve_mrc_despread;\n'
                   'int (*const p_stage)(ofdm_rx*, const float*, int32_t, int64_t, int64_t, int32_t, int64_t, const float*, int64_t, float,\n'
                   '    int32_t, int32_t, const double*, const double*, int32_t, const ofdm_mrc_despread_out*, void*) = ofdm_combine_despread_frames;\n'
                   'int64_t (*const p_frames)(ofdm_rx*, const float*, int32_t, int64_t, int64_t, int64_t, float*, int32_t*, int32_t,\n'
                   '    const double*, const double*, int32_t, const ofdm_mrc_despread_out*, void*) = ofdm_rx_demod_frames_mrc_despread;\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", ' +
                   ", ".join("offsetof(ofdm_mrc_despread_out, %s)" % f for f in FIELDS) +
                   ', sizeof(ofdm_mrc_despread_out)); return OFDM_ABI_VERSION; }\n')
    obj = tmp_path / "t.o"
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    # the layout alone, linked without the library
    lay = tmp_path / "l.c"
    lay.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ofdm_mi355x.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", ' +
                   ", ".join("offsetof(ofdm_mrc_despread_out, %s)" % f for f in FIELDS) +
                   ', sizeof(ofdm_mrc_despread_out)); return OFDM_ABI_VERSION; }\n')
    exe = tmp_path / "l"
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(lay), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    from ofdm_mi355x import _lib
    assert r.returncode == 1
    assert r.stdout.split() == ["0", "8", "16", "24", "32", "40", str(C.sizeof(_lib.MrcDespreadOut))]


def test_argument_errors_are_invalid_before_the_handle_is_used(lib):
    from ofdm_mi355x import _lib
    fake = C.create_string_buffer(1 << 16)                   # never read: every call below is refused on its arguments
    h = C.addressof(fake)
    sink = C.create_string_buffer(64)
    p = C.addressof(sink)
    nan, inf = float("nan"), float("inf")

    def nv(*v):
        return (C.c_double * len(v))(*v)

    def call(handle=h, sym=p, csi=p, n_branch=2, n_seg=2, rows=3, M=60, seg_stride=None, csi_stride=None, rho=0.03, mod=4, mode=GIVEN,
             var=nv(0.1, 0.2), sigma2=None, bits_mode=UNPACKED, out="llr"):
        o = None if out is None else _lib.MrcDespreadOut(**{k: p for k in out.split()})
        return lib.ofdm_combine_despread_frames(handle, sym, n_branch, n_seg, rows, M, rows * M if seg_stride is None else seg_stride,
                                                csi, M if csi_stride is None else csi_stride, rho, mod, mode, var, sigma2, bits_mode,
                                                None if o is None else C.byref(o), None)

    assert call(handle=None) == ERR_INVALID and b"null handle" in lib.ofdm_last_error()
    for kw, text in ((dict(M=7), b"2^a 3^b 5^c"), (dict(M=0), b"2^a 3^b 5^c"), (dict(M=-4), b"2^a 3^b 5^c"), (dict(M=4100), b"2^a 3^b 5^c"),
                     (dict(n_seg=-1), b"negative count"), (dict(rows=-1), b"negative count"),
                     (dict(n_branch=0), b"n_branch"), (dict(n_branch=-1), b"n_branch"), (dict(n_branch=9, var=nv(*[0.1] * 9)), b"n_branch"),
                     (dict(seg_stride=3 * 60 - 1), b"seg_stride < rows"), (dict(csi_stride=59), b"csi_stride <"),
                     (dict(mod=1), b"modulation"), (dict(mod=3), b"modulation"), (dict(mode=EST), b"OFDM_MRC_NOISE_EST"), (dict(mode=3), b"noise_mode"),
                     (dict(mode=-1), b"noise_mode"), (dict(var=None), b"h_noise_var"), (dict(mode=SEG, sigma2=None), b"d_sigma2"),
                     (dict(var=nv(0.1, 0.0)), b"noise_var"), (dict(var=nv(-1.0, 0.1)), b"noise_var"), (dict(var=nv(0.1, nan)), b"noise_var"),
                     (dict(var=nv(inf, 0.1)), b"noise_var"), (dict(rho=-0.5), b"rho"), (dict(rho=nan), b"rho"), (dict(rho=inf), b"rho"),
                     (dict(out=None), b"no pointer"), (dict(out=""), b"no pointer"),
                     (dict(out="bits", bits_mode=NONE), b"bits_mode"), (dict(out="bits", bits_mode=7), b"bits_mode"),
                     (dict(out="llr bits", M=75, mod=2, bits_mode=PACKED), b"packed bits"),
                     (dict(n_seg=(1 << 30) + 1), b"index range"), (dict(n_branch=1, n_seg=(1 << 31) + 1, var=nv(0.1)), b"index range"),
                     (dict(rows=1 << 40, M=2, seg_stride=1 << 62), b"index range"),
                     (dict(n_seg=1 << 19, seg_stride=1 << 30), b"index range"), (dict(n_seg=1 << 19, csi_stride=1 << 30), b"index range"),
                     (dict(n_branch=1, var=nv(0.1), n_seg=1 << 31, rows=2, M=4096, seg_stride=8192, csi_stride=4096), b"index range"),
                     # more than 2^31 - 1 workgroups: small rows pass every other limit (2^31 units, 2^31 * 12 < 2^40 symbols)
                     (dict(n_branch=1, var=nv(0.1), n_seg=1 << 31, rows=1, M=12), b"workgroups"),
                     (dict(n_branch=1, var=nv(0.1), n_seg=1 << 30, rows=65, M=12), b"workgroups")):      # two groups of 64 rows each
        assert call(**kw) == ERR_INVALID, kw
        err = lib.ofdm_last_error()
        assert b"ofdm_combine_despread_frames" in err and text in err, (kw, err)
    # the buffers are looked at after the arguments
    assert call(sym=None) == ERR_INVALID and b"null d_sym or d_csi" in lib.ofdm_last_error()
    assert call(csi=None) == ERR_INVALID and b"null d_sym or d_csi" in lib.ofdm_last_error()
    # only the first n_branch variances are read
    assert call(n_branch=1, var=nv(0.1, nan), n_seg=0) == 0
    # no-ops: the handle is not touched
    assert call(n_seg=0) == 0 and call(rows=0) == 0
    assert call(mode=SEG, sigma2=p, n_seg=0) == 0 and call(rho=0.0, rows=0) == 0 and call(n_branch=8, var=nv(*[0.1] * 8), n_seg=0) == 0
    assert call(out="llr bits", M=60, mod=2, bits_mode=PACKED, rows=0) == 0 and call(out="comb beta", rows=0) == 0
    # the most workgroups a launch takes, 2^31 - 1, passes the checks (rows = 0 makes it a no-op after them)
    assert call(n_branch=1, var=nv(0.1), n_seg=(1 << 31) - 1, rows=0, M=12) == 0

    assert lib.ofdm_rx_reserve_mrc_despread(None, 60, 2, 1) == ERR_INVALID and b"ofdm_rx_reserve_mrc_despread" in lib.ofdm_last_error()
    for args in ((7, 2, 1), (0, 2, 1), (4100, 2, 1), (60, 0, 1), (60, 9, 1), (60, 2, -1), (60, 2, (1 << 30) + 1)):
        assert lib.ofdm_rx_reserve_mrc_despread(h, *args) == ERR_INVALID, args
        assert b"ofdm_rx_reserve_mrc_despread" in lib.ofdm_last_error()

    out = _lib.MrcDespreadOut(llr=p)
    two = nv(0.1, 0.2)
    f = lib.ofdm_rx_demod_frames_mrc_despread
    assert f(None, p, 2, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_rx_demod_frames_mrc_despread" in lib.ofdm_last_error() and b"null handle" in lib.ofdm_last_error()
    assert f(h, p, 2, 1, 32, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert f(h, None, 2, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert f(h, p, 0, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert b"n_branch" in lib.ofdm_last_error()
    assert f(h, p, 9, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert f(h, p, 2, 1, 64, 64, None, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert b"needs d_eq" in lib.ofdm_last_error()


def test_engine_checks_the_noise_arguments():
    """exactly one of noise_var / d_sigma2, and n_branch numbers: refused in Python, before the library is called"""
    import ofdm_mi355x as om
    e = object.__new__(om.RxEngine)                          # no handle: the checks come first
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.combine_despread_frames(e, 1, 2, 1, 1, 12, 12, 1, 12, 0.03, "QPSK", d_llr=1)
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.combine_despread_frames(e, 1, 2, 1, 1, 12, 12, 1, 12, 0.03, "QPSK", noise_var=[0.1, 0.1], d_sigma2=1, d_llr=1)
    with pytest.raises(ValueError, match="n_branch"):
        om.RxEngine.combine_despread_frames(e, 1, 2, 1, 1, 12, 12, 1, 12, 0.03, "QPSK", noise_var=[0.1], d_llr=1)
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.demod_frames_mrc_despread(e, 1, 2, 1, 64, 64, 1)
    with pytest.raises(ValueError, match="n_branch"):
        om.RxEngine.demod_frames_mrc_despread(e, 1, 2, 1, 64, 64, 1, noise_var=[0.1, 0.2, 0.3])
