"""The channel-tracking calls' C ABI without a GPU: the library exports them, the ctypes table and the engine carry them, the
header's block compiles as plain C with the constants the package states, and a null handle is refused by name."""
import os

import pytest

NEW = ("ofdm_chan_track_frames", "ofdm_rx_demod_frames_track", "ofdm_rx_reserve_chan_track")
ERR_INVALID = -1


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
    for name in ("chan_track_frames", "demod_frames_track", "reserve_chan_track"):
        assert callable(getattr(om.RxEngine, name))
    assert (om.TRACK_HOLD, om.TRACK_LINEAR) == (0, 1) == (om.RxEngine.TRACK_HOLD, om.RxEngine.TRACK_LINEAR)
    assert len(_lib.PROTOTYPES["ofdm_chan_track_frames"][1]) == 12 and len(_lib.PROTOTYPES["ofdm_rx_demod_frames_track"][1]) == 10
    assert [f[0] for f in _lib.TrackOut._fields_] == ["eq", "bits", "csi", "H_pat", "takes"]
    assert lib.ofdm_abi_version() == 1


def test_prototypes_cover_the_header(lib):
    import re
    from conftest import ROOT
    from ofdm_mi355x import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofdm_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofdm_[a-z0-9_]+)\s*\(", txt))
    assert set(NEW) <= declared and set(_lib.PROTOTYPES) == declared


def test_header_declares_the_block_as_c(lib, tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "ofdm_mi355x.h"\n'
                   '_Static_assert(OFDM_TRACK_HOLD == 0 && OFDM_TRACK_LINEAR == 1, "the package states the header\'s modes");\n'
                   '_Static_assert(OFDM_ABI_VERSION == 1, "the ABI version stays");\n'
                   '_Static_assert(offsetof(ofdm_track_out, takes) == 4 * sizeof(void*), "five pointers");\n'
                   'int64_t (*a)(ofdm_rx*, const float*, int64_t, int64_t, int64_t, const int32_t*, int32_t, int32_t, int32_t, int32_t,\n'
                   '             const ofdm_track_out*, void*) = ofdm_chan_track_frames;\n'
                   'int64_t (*b)(ofdm_rx*, const float*, int64_t, int64_t, int64_t, int32_t, int32_t, int32_t*, const ofdm_track_out*,\n'
                   '             void*) = ofdm_rx_demod_frames_track;\n'
                   'int (*c)(ofdm_rx*, int64_t, int64_t) = ofdm_rx_reserve_chan_track;\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_null_handle_is_refused_by_name(lib):
    import ctypes as C
    from ofdm_mi355x import _lib
    out = _lib.TrackOut(1, None, None, None, None)
    assert lib.ofdm_chan_track_frames(None, None, 1, 64, 64, None, 1, 0, 0, 0, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_chan_track_frames: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_rx_demod_frames_track(None, None, 1, 64, 64, 1, 0, None, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_rx_demod_frames_track: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_chan_track(None, 1, 64) == ERR_INVALID and b"ofdm_rx_reserve_chan_track: null handle" in lib.ofdm_last_error()
