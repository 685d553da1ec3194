"""The segmented soft de-mapper's C ABI without a GPU: the three new symbols are exported and bound, the ctypes struct mirrors the
header's, the header still compiles as C11, and argument errors are reported before any device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ("ofdm_rx_reserve_soft", "ofdm_demap_frames", "ofdm_rx_demod_frames_soft")


def _lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load(), L


def test_soft_symbols_are_exported_and_bound():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.PROTOTYPES
    assert lib.ofdm_abi_version() == 1


def test_soft_out_struct_matches_the_header():
    _, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    body = re.search(r"typedef struct ofdm_soft_out \{(.*?)\} ofdm_soft_out;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in L.SoftOut._fields_] == ["soft0", "soft1", "llr", "sigma"]
    assert C.sizeof(L.SoftOut) == 4 * C.sizeof(C.c_void_p)


def test_null_handle_is_rejected_by_name():
    lib, L = _lib()
    buf = (C.c_float * 64)()
    out = L.SoftOut()
    out.llr = C.addressof(buf)
    assert lib.ofdm_demap_frames(None, buf, 1, 4, 4, 2, C.byref(out), None) == L.OFDM_ERR_INVALID
    assert "ofdm_demap_frames" in lib.ofdm_last_error().decode()
    assert lib.ofdm_rx_demod_frames_soft(None, buf, 1, 32, 32, buf, None, 0, None, C.byref(out), None) == L.OFDM_ERR_INVALID
    assert "ofdm_rx_demod_frames_soft" in lib.ofdm_last_error().decode()
    assert lib.ofdm_rx_reserve_soft(None, 4, 100) == L.OFDM_ERR_INVALID
    assert "ofdm_rx_reserve_soft" in lib.ofdm_last_error().decode()


def test_argument_errors_need_no_device():
    """Checked before the handle is used: a stand-in handle that is never dereferenced is enough."""
    lib, L = _lib()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    buf = (C.c_float * 64)()
    out = L.SoftOut()
    out.llr = C.addressof(buf)
    for n_seg, seg_len, stride, mod in ((-1, 4, 4, 2), (1, -4, 4, 2), (2, 4, 3, 2), (1, 4, 4, 1), (1, 4, 4, 3),
                                        (1 << 32, 4, 4, 2), (4, 1 << 41, 1 << 41, 2), (1 << 20, 8, 1 << 30, 4)):
        assert lib.ofdm_demap_frames(dummy, buf, n_seg, seg_len, stride, mod, C.byref(out), None) == L.OFDM_ERR_INVALID
        assert "ofdm_demap_frames" in lib.ofdm_last_error().decode()
    # empty batches and an output set without pointers are no-ops
    none = L.SoftOut()
    assert lib.ofdm_demap_frames(dummy, buf, 0, 4, 4, 2, C.byref(out), None) == L.OFDM_OK
    assert lib.ofdm_demap_frames(dummy, buf, 3, 0, 0, 4, C.byref(out), None) == L.OFDM_OK
    assert lib.ofdm_demap_frames(dummy, buf, 3, 4, 4, 6, C.byref(none), None) == L.OFDM_OK
    assert lib.ofdm_demap_frames(dummy, buf, 3, 4, 4, 6, None, None) == L.OFDM_OK
    # the receiver: soft outputs without d_eq, bad layout
    assert lib.ofdm_rx_demod_frames_soft(dummy, buf, 1, 32, 32, None, None, 0, None, C.byref(out), None) == L.OFDM_ERR_INVALID
    assert "d_eq" in lib.ofdm_last_error().decode()
    assert lib.ofdm_rx_demod_frames_soft(dummy, buf, 1, 16, 32, buf, None, 0, None, C.byref(out), None) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_demod_frames_soft(dummy, None, 1, 32, 32, buf, None, 0, None, C.byref(out), None) == L.OFDM_ERR_INVALID
    assert lib.ofdm_rx_demod_frames_soft(dummy, buf, -1, 32, 32, buf, None, 0, None, C.byref(out), None) == L.OFDM_ERR_INVALID


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_header_compiles_as_c11(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    src = tmp_path / "h.c"
    src.write_text('#include "ofdm_mi355x.h"\n'
                   "int use(ofdm_rx* h, const float* d, ofdm_soft_out* o) {\n"
                   "    return ofdm_demap_frames(h, d, 1, 2, 2, OFDM_MOD_QPSK, o, 0) + ofdm_rx_reserve_soft(h, 1, 2) +\n"
                   "           (int)ofdm_rx_demod_frames_soft(h, d, 1, 2, 2, (float*)d, 0, 0, 0, o, 0);\n"
                   "}\n")
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
