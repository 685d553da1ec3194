"""The channel-estimate averaging calls' C ABI without a GPU: the library exports them, the ctypes table and the engine carry them,
the header's block compiles as plain C with the chunk length the package states, and a null handle is refused by name."""
import os

import pytest

NEW = ("ofdm_chan_average_frames", "ofdm_rx_set_chan_average", "ofdm_rx_reserve_chan_average", "ofdm_rx_chan_spread_frames")
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
    for name in ("set_chan_average", "reserve_chan_average", "chan_average_frames", "chan_spread_frames"):
        assert callable(getattr(om.RxEngine, name))
    assert om.RxEngine.CHANAVG_CHUNK == 16
    assert len(_lib.PROTOTYPES["ofdm_chan_average_frames"][1]) == 13
    assert lib.ofdm_abi_version() == 1


def test_header_declares_the_block_as_c(lib, tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT
    import ofdm_mi355x as om
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "t.c"
    src.write_text('#include "ofdm_mi355x.h"\n'
                   '_Static_assert(OFDM_CHANAVG_CHUNK == %d, "the package states the header\'s chunk length");\n'
                   '_Static_assert(OFDM_ABI_VERSION == 1, "the ABI version stays");\n'
                   'int (*a)(ofdm_rx*, const float*, int64_t, int64_t, int64_t, const int32_t*, int32_t, float*, float*, float*, int32_t*,\n'
                   '         float*, void*) = ofdm_chan_average_frames;\n'
                   'int (*b)(ofdm_rx*, int32_t) = ofdm_rx_set_chan_average;\n'
                   'int (*c)(ofdm_rx*, int64_t, int64_t) = ofdm_rx_reserve_chan_average;\n'
                   'int (*d)(ofdm_rx*, int64_t, double*, void*) = ofdm_rx_chan_spread_frames;\n' % om.RxEngine.CHANAVG_CHUNK)
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_null_handle_is_refused_by_name(lib):
    assert lib.ofdm_chan_average_frames(None, None, 1, 64, 64, None, -1, None, None, None, None, None, None) == ERR_INVALID
    assert b"ofdm_chan_average_frames: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_rx_set_chan_average(None, 1) == ERR_INVALID and b"ofdm_rx_set_chan_average" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_chan_average(None, 1, 64) == ERR_INVALID and b"ofdm_rx_reserve_chan_average" in lib.ofdm_last_error()
    assert lib.ofdm_rx_chan_spread_frames(None, 1, None, None) == ERR_INVALID and b"ofdm_rx_chan_spread_frames" in lib.ofdm_last_error()
