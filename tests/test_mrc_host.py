"""The receive-diversity combining calls' C ABI without a GPU: the library exports them, the ctypes table and the engine carry
them, ofdm_mrc_out has the layout a C compiler gives it, and every argument error of ofdm_combine_csi_frames returns
OFDM_ERR_INVALID with its reason before the handle is read -- so that it can be reached here with a handle that is only an
address: a block of zeroed host memory."""
import ctypes as C
import os

import pytest

NEW = ("ofdm_rx_reserve_mrc", "ofdm_combine_csi_frames", "ofdm_rx_demod_frames_mrc")
ERR_INVALID = -1
GIVEN, SEG, EST = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_library_and_package_export_the_mrc_calls(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    for name in ("reserve_mrc", "combine_csi_frames", "demod_frames_mrc"):
        assert callable(getattr(om.RxEngine, name))
    assert [f[0] for f in _lib.MrcOut._fields_] == ["llr", "sym", "weight"]
    assert (om.MRC_NOISE_GIVEN, om.MRC_NOISE_SEG, om.MRC_NOISE_EST) == (GIVEN, SEG, EST)
    assert lib.ofdm_abi_version() == 1


def test_header_declares_the_block_as_c(lib, tmp_path):
    """the enum values, the branch limit and the struct layout as a C compiler sees them"""
    import shutil
    import subprocess
    from conftest import ROOT
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ofdm_mi355x.h"\n'
                   'int main(void) { printf("%d %d %d %d %zu %zu %zu %zu\\n", OFDM_MRC_NOISE_GIVEN, OFDM_MRC_NOISE_SEG, '
                   'OFDM_MRC_NOISE_EST, OFDM_MRC_MAX_BRANCHES, offsetof(ofdm_mrc_out, llr), offsetof(ofdm_mrc_out, sym), '
                   'offsetof(ofdm_mrc_out, weight), sizeof(ofdm_mrc_out)); return OFDM_ABI_VERSION; }\n')
    exe = tmp_path / "t"
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    from ofdm_mi355x import _lib
    assert r.returncode == 1
    assert r.stdout.split() == ["0", "1", "2", "8", "0", "8", "16", str(C.sizeof(_lib.MrcOut))]
    assert _lib.MRC_MAX_BRANCHES == 8


def test_argument_errors_are_invalid_before_the_handle_is_used(lib):
    from ofdm_mi355x import _lib
    fake = C.create_string_buffer(1 << 16)                   # never read: every call below is refused on its arguments
    h = C.addressof(fake)
    sink = C.create_string_buffer(64)
    p = C.addressof(sink)
    nan, inf = float("nan"), float("inf")

    def nv(*v):
        return (C.c_double * len(v))(*v)

    def call(handle=h, n_branch=2, n_seg=2, rows=3, row_len=57, seg_stride=None, csi_stride=None, rho=0.03, mod=4, mode=GIVEN,
             var=nv(0.1, 0.2), sigma2=None, llr=p):
        out = _lib.MrcOut(llr, None, None)
        return lib.ofdm_combine_csi_frames(handle, p, n_branch, n_seg, rows, row_len, rows * row_len if seg_stride is None else seg_stride,
                                           p, row_len if csi_stride is None else csi_stride, rho, mod, mode, var, sigma2, C.byref(out),
                                           None)

    assert call(handle=None) == ERR_INVALID and b"null handle" in lib.ofdm_last_error()
    for kw, text in ((dict(n_seg=-1), b"negative count"), (dict(rows=-1), b"negative count"), (dict(row_len=-1, seg_stride=0), b"negative count"),
                     (dict(n_branch=0), b"n_branch"), (dict(n_branch=-1), b"n_branch"), (dict(n_branch=9, var=nv(*[0.1] * 9)), b"n_branch"),
                     (dict(seg_stride=3 * 57 - 1), b"seg_stride < rows * row_len"), (dict(csi_stride=56), b"csi_stride < row_len"),
                     (dict(mod=1), b"modulation"), (dict(mod=3), b"modulation"), (dict(mode=EST), b"noise_mode"), (dict(mode=3), b"noise_mode"),
                     (dict(mode=-1), b"noise_mode"), (dict(var=None), b"h_noise_var"), (dict(mode=SEG, sigma2=None), b"d_sigma2"),
                     (dict(var=nv(0.1, 0.0)), b"noise_var"), (dict(var=nv(-1.0, 0.1)), b"noise_var"), (dict(var=nv(0.1, nan)), b"noise_var"),
                     (dict(var=nv(inf, 0.1)), b"noise_var"), (dict(rho=-0.5), b"rho"), (dict(rho=nan), b"rho"), (dict(rho=inf), b"rho"),
                     (dict(n_seg=(1 << 30) + 1), b"index range"), (dict(n_branch=1, n_seg=(1 << 31) + 1, var=nv(0.1)), b"index range"),
                     (dict(row_len=(1 << 30) + 1, rows=1), b"index range"), (dict(rows=1 << 40, row_len=2, seg_stride=1 << 62), b"index range"),
                     (dict(n_seg=1 << 19, seg_stride=1 << 30), b"index range"), (dict(n_seg=1 << 19, csi_stride=1 << 30), b"index range")):
        assert call(**kw) == ERR_INVALID, kw
        err = lib.ofdm_last_error()
        assert b"ofdm_combine_csi_frames" in err and text in err, (kw, err)
    # only the first n_branch variances are read
    assert call(n_branch=1, var=nv(0.1, nan), n_seg=0) == 0
    # no-ops: the handle is not touched
    assert call(n_seg=0) == 0 and call(rows=0) == 0 and call(llr=None) == 0 and call(row_len=0) == 0
    assert call(mode=SEG, sigma2=p, n_seg=0) == 0 and call(rho=0.0, rows=0) == 0 and call(n_branch=8, var=nv(*[0.1] * 8), n_seg=0) == 0
    # units at the limit are accepted: 2 * 2^30 = 2^31
    assert call(n_seg=1 << 30, rows=0) == 0

    assert lib.ofdm_rx_reserve_mrc(None, 1, 1, 1, 1) == ERR_INVALID and b"ofdm_rx_reserve_mrc" in lib.ofdm_last_error()
    for args in ((1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1), (0, 1, 1, 1), (9, 1, 1, 1), (2, (1 << 30) + 1, 1, 1), (1, 1, 1 << 40, 2),
                 (1, 1, 1, (1 << 30) + 1)):
        assert lib.ofdm_rx_reserve_mrc(h, *args) == ERR_INVALID, args
        assert b"ofdm_rx_reserve_mrc" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_mrc(h, 2, 0, 0, 0) == 0

    out = _lib.MrcOut(p, None, None)
    two = nv(0.1, 0.2)
    assert lib.ofdm_rx_demod_frames_mrc(None, p, 2, 1, 64, 64, p, None, GIVEN, two, C.byref(out), None, None) == ERR_INVALID
    assert b"ofdm_rx_demod_frames_mrc" in lib.ofdm_last_error()
    assert lib.ofdm_rx_demod_frames_mrc(h, p, 2, 1, 32, 64, p, None, GIVEN, two, C.byref(out), None, None) == ERR_INVALID
    assert lib.ofdm_rx_demod_frames_mrc(h, p, 0, 1, 64, 64, p, None, GIVEN, two, C.byref(out), None, None) == ERR_INVALID
    assert b"n_branch" in lib.ofdm_last_error()
    assert lib.ofdm_rx_demod_frames_mrc(h, p, 2, 1, 64, 64, None, None, GIVEN, two, C.byref(out), None, None) == ERR_INVALID
    assert b"needs d_eq" in lib.ofdm_last_error()


def test_engine_checks_the_noise_arguments():
    """exactly one of noise_var / d_sigma2, and n_branch numbers: refused in Python, before the library is called"""
    import ofdm_mi355x as om
    e = object.__new__(om.RxEngine)                          # no handle: the checks come first
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.combine_csi_frames(e, 1, 2, 1, 1, 2, 2, 1, 2, 0.03, "QPSK", d_llr=1)
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.combine_csi_frames(e, 1, 2, 1, 1, 2, 2, 1, 2, 0.03, "QPSK", noise_var=[0.1, 0.1], d_sigma2=1, d_llr=1)
    with pytest.raises(ValueError, match="n_branch"):
        om.RxEngine.combine_csi_frames(e, 1, 2, 1, 1, 2, 2, 1, 2, 0.03, "QPSK", noise_var=[0.1], d_llr=1)
    with pytest.raises(ValueError, match="n_branch"):
        om.RxEngine.demod_frames_mrc(e, 1, 2, 1, 64, 64, 1, noise_var=[0.1, 0.2, 0.3])
