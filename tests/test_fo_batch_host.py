"""The frame-batched CFO-search receiver's C ABI without a GPU: the new symbols are exported and bound, the ctypes struct
mirrors the header's, and argument errors are reported before any device is touched."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("ofdm_fo_reserve", "ofdm_fo_demod_frames")


def _lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load(), L


def test_batch_symbols_are_exported_and_bound():
    lib, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in L.PROTOTYPES
    assert lib.ofdm_abi_version() == 1


def test_batch_out_struct_matches_the_header():
    _, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read()
    body = re.search(r"typedef struct ofdm_fo_batch_out \{(.*?)\} ofdm_fo_batch_out;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f[0] for f in L.FoBatchOut._fields_]
    assert C.sizeof(L.FoBatchOut) == 9 * C.sizeof(C.c_void_p) + 8          # nine pointers, one int32 padded to 8 bytes


def test_batch_argument_errors_need_no_device():
    lib, L = _lib()
    status = (C.c_int32 * 4)()
    out = L.FoBatchOut()
    out.status = C.addressof(status)
    iq = (C.c_float * 64)()
    # NULL handle
    assert lib.ofdm_fo_demod_frames(None, iq, 1, 32, 32, C.byref(out), None) == L.OFDM_ERR_INVALID
    assert lib.ofdm_fo_reserve(None, 4, 1000) == L.OFDM_ERR_INVALID
    # status == NULL (and no output set at all) is rejected before the handle is looked at
    dummy = C.create_string_buffer(64)
    none = L.FoBatchOut()
    assert lib.ofdm_fo_demod_frames(C.cast(dummy, C.c_void_p), iq, 1, 32, 32, C.byref(none), None) == L.OFDM_ERR_INVALID
    assert lib.ofdm_fo_demod_frames(C.cast(dummy, C.c_void_p), iq, 1, 32, 32, None, None) == L.OFDM_ERR_INVALID
    assert "status" in lib.ofdm_last_error().decode()
