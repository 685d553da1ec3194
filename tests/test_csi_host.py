"""The channel-state-weighted LLR calls' C ABI without a GPU: the library exports them, the ctypes table and the engine carry
them, and every argument error of ofdm_demap_csi_frames returns OFDM_ERR_INVALID with its reason before the handle is read --
so that it can be reached here with a handle that is only an address: a block of zeroed host memory."""
import ctypes as C
import os

import pytest

NEW = ("ofdm_rx_reserve_csi", "ofdm_rx_csi_frames", "ofdm_demap_csi_frames", "ofdm_rx_demod_frames_csi")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_library_and_package_export_the_csi_calls(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    for name in ("reserve_csi", "csi_frames", "demap_csi_frames", "demod_frames_csi"):
        assert callable(getattr(om.RxEngine, name))
    assert [f[0] for f in _lib.CsiOut._fields_] == ["llr", "sigma2", "n_used"]
    assert (om.CSI_NOISE_EST, om.CSI_NOISE_GIVEN, om.CSI_ROWS_ALL, om.CSI_ROWS_DATA) == (0, 1, 0, 1)
    assert lib.ofdm_abi_version() == 1


def test_header_declares_the_block_as_c(lib, tmp_path):
    """the enum values and the struct layout as a C compiler sees them"""
    import shutil
    import subprocess
    from conftest import ROOT
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ofdm_mi355x.h"\n'
                   'int main(void) { printf("%d %d %d %d %zu %zu %zu %zu\\n", OFDM_CSI_NOISE_EST, OFDM_CSI_NOISE_GIVEN, '
                   'OFDM_CSI_ROWS_ALL, OFDM_CSI_ROWS_DATA, offsetof(ofdm_csi_out, llr), offsetof(ofdm_csi_out, sigma2), '
                   'offsetof(ofdm_csi_out, n_used), sizeof(ofdm_csi_out)); return OFDM_ABI_VERSION; }\n')
    exe = tmp_path / "t"
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    from ofdm_mi355x import _lib
    assert r.returncode == 1
    assert r.stdout.split() == ["0", "1", "0", "1", "0", "8", "16", str(C.sizeof(_lib.CsiOut))]


def test_argument_errors_are_invalid_before_the_handle_is_used(lib):
    from ofdm_mi355x import _lib
    fake = C.create_string_buffer(1 << 16)                   # never read: every call below is refused on its arguments
    h = C.addressof(fake)
    sink = C.create_string_buffer(64)
    p = C.addressof(sink)
    nan, inf = float("nan"), float("inf")

    def call(handle=h, n_seg=2, rows=3, row_len=57, seg_stride=None, csi_stride=None, rho=0.03, mod=4, mode=0, var=0.0, llr=p):
        out = _lib.CsiOut(llr, None, None)
        return lib.ofdm_demap_csi_frames(handle, p, n_seg, rows, row_len, rows * row_len if seg_stride is None else seg_stride, p,
                                         row_len if csi_stride is None else csi_stride, rho, mod, mode, var, C.byref(out), None)

    assert call(handle=None) == ERR_INVALID and b"null handle" in lib.ofdm_last_error()
    for kw, text in ((dict(n_seg=-1), b"negative count"), (dict(rows=-1), b"negative count"), (dict(row_len=-1, seg_stride=0), b"negative count"),
                     (dict(seg_stride=3 * 57 - 1), b"seg_stride < rows * row_len"), (dict(csi_stride=56), b"csi_stride < row_len"),
                     (dict(mod=1), b"modulation"), (dict(mod=3), b"modulation"), (dict(mode=2), b"noise_mode"), (dict(mode=-1), b"noise_mode"),
                     (dict(mode=1, var=0.0), b"noise_var"), (dict(mode=1, var=-1.0), b"noise_var"), (dict(mode=1, var=nan), b"noise_var"),
                     (dict(mode=1, var=inf), b"noise_var"), (dict(rho=-0.5), b"rho"), (dict(rho=nan), b"rho"), (dict(rho=inf), b"rho"),
                     (dict(n_seg=(1 << 31) + 1), b"index range"), (dict(row_len=(1 << 30) + 1, rows=1), b"index range"),
                     (dict(rows=1 << 40, row_len=2, seg_stride=1 << 62), b"index range"),
                     (dict(n_seg=1 << 20, seg_stride=1 << 30), b"index range"), (dict(n_seg=1 << 20, csi_stride=1 << 30), b"index range")):
        assert call(**kw) == ERR_INVALID, kw
        err = lib.ofdm_last_error()
        assert b"ofdm_demap_csi_frames" in err and text in err, (kw, err)
    # no-ops: the handle is not touched
    assert call(n_seg=0) == 0 and call(rows=0) == 0 and call(llr=None) == 0 and call(row_len=0) == 0
    assert call(mode=1, var=0.5, n_seg=0) == 0 and call(rho=0.0, rows=0) == 0

    assert lib.ofdm_rx_reserve_csi(None, 1, 1, 1) == ERR_INVALID and b"ofdm_rx_reserve_csi" in lib.ofdm_last_error()
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), ((1 << 31) + 1, 1, 1), (1, 1 << 40, 2), (1, 1, (1 << 30) + 1)):
        assert lib.ofdm_rx_reserve_csi(h, *args) == ERR_INVALID, args
    assert lib.ofdm_rx_reserve_csi(h, 0, 0, 0) == 0

    assert lib.ofdm_rx_csi_frames(None, 1, 0, p, 60, None) == ERR_INVALID and b"null handle" in lib.ofdm_last_error()
    assert lib.ofdm_rx_csi_frames(h, -1, 0, p, 60, None) == ERR_INVALID and b"negative" in lib.ofdm_last_error()
    assert lib.ofdm_rx_csi_frames(h, 1, 2, p, 60, None) == ERR_INVALID and b"layout" in lib.ofdm_last_error()
    # a zeroed handle has no pilots and has demodulated no frames
    assert lib.ofdm_rx_csi_frames(h, 1, 1, p, 60, None) == ERR_INVALID and b"pilots" in lib.ofdm_last_error()
    assert lib.ofdm_rx_csi_frames(h, 1, 0, p, 60, None) == ERR_INVALID and b"last ofdm_rx_demod_frames call" in lib.ofdm_last_error()

    out = _lib.CsiOut(p, None, None)
    assert lib.ofdm_rx_demod_frames_csi(None, p, 1, 64, 64, p, None, 0, None, 0, 0.0, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_rx_demod_frames_csi" in lib.ofdm_last_error()
    assert lib.ofdm_rx_demod_frames_csi(h, p, 1, 32, 64, p, None, 0, None, 0, 0.0, C.byref(out), None) == ERR_INVALID
    assert lib.ofdm_rx_demod_frames_csi(h, p, 1, 64, 64, None, None, 0, None, 0, 0.0, C.byref(out), None) == ERR_INVALID
    assert b"needs d_eq" in lib.ofdm_last_error()
