"""The DFT-spread OFDM calls' C ABI without a GPU: the library exports them, the ctypes table and the engines carry them, the
header's block compiles as plain C with the constants the package states, a null handle is refused by name, and the two host
calls (ofdm_dft_size_ok, ofdm_dft_plan_info) answer without a device."""
import os

import pytest

NEW = ("ofdm_dft_size_ok", "ofdm_dft_plan_info", "ofdm_tx_dft_spread", "ofdm_tx_reserve_spread", "ofdm_tx_modulate_frames_spread",
       "ofdm_dft_despread_frames", "ofdm_rx_reserve_despread", "ofdm_rx_demod_frames_despread")
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
    for name in ("dft_spread", "reserve_spread", "modulate_frames_spread"):
        assert callable(getattr(om.TxEngine, name))
    for name in ("dft_despread_frames", "reserve_despread", "demod_frames_despread"):
        assert callable(getattr(om.RxEngine, name))
    assert (om.DESPREAD_NOISE_RHO, om.DESPREAD_NOISE_GIVEN, om.DESPREAD_NOISE_SEG) == (0, 1, 2)
    assert len(_lib.PROTOTYPES["ofdm_dft_despread_frames"][1]) == 16 and len(_lib.PROTOTYPES["ofdm_rx_demod_frames_despread"][1]) == 13
    assert len(_lib.PROTOTYPES["ofdm_tx_modulate_frames_spread"][1]) == 8
    assert [f[0] for f in _lib.DespreadOut._fields_] == ["sym", "llr", "bits", "beta", "weight"]
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
                   '_Static_assert(OFDM_DESPREAD_NOISE_RHO == 0 && OFDM_DESPREAD_NOISE_GIVEN == 1 && OFDM_DESPREAD_NOISE_SEG == 2,\n'
                   '               "the package states the header\'s modes");\n'
                   '_Static_assert(OFDM_ABI_VERSION == 1, "the ABI version stays");\n'
                   '_Static_assert(offsetof(ofdm_despread_out, weight) == 4 * sizeof(void*), "five pointers");\n'
                   '_Static_assert(sizeof(ofdm_despread_out) == 5 * sizeof(void*), "five pointers");\n'
                   'int (*a)(int32_t) = ofdm_dft_size_ok;\n'
                   'int (*b)(int32_t, int32_t*, int32_t*, int32_t*) = ofdm_dft_plan_info;\n'
                   'int (*c)(ofdm_tx*, const float*, int64_t, int32_t, float*, void*) = ofdm_tx_dft_spread;\n'
                   'int (*d)(ofdm_tx*, int32_t, int64_t) = ofdm_tx_reserve_spread;\n'
                   'int64_t (*e)(ofdm_tx*, const uint8_t*, int32_t, int64_t, int32_t, float*, int64_t, void*) = ofdm_tx_modulate_frames_spread;\n'
                   'int (*f)(ofdm_rx*, const float*, int64_t, int64_t, int32_t, int64_t, const float*, int64_t, float, int32_t, int32_t,\n'
                   '         double, const double*, int32_t, const ofdm_despread_out*, void*) = ofdm_dft_despread_frames;\n'
                   'int (*g)(ofdm_rx*, int32_t, int64_t) = ofdm_rx_reserve_despread;\n'
                   'int64_t (*h)(ofdm_rx*, const float*, int64_t, int64_t, int64_t, float*, int32_t*, int32_t, double, const double*,\n'
                   '             int32_t, const ofdm_despread_out*, void*) = ofdm_rx_demod_frames_despread;\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_null_handle_is_refused_by_name(lib):
    import ctypes as C
    from ofdm_mi355x import _lib
    out = _lib.DespreadOut(1, None, None, None, None)
    assert lib.ofdm_tx_dft_spread(None, None, 1, 12, None, None) == ERR_INVALID
    assert b"ofdm_tx_dft_spread: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_tx_reserve_spread(None, 12, 1) == ERR_INVALID and b"ofdm_tx_reserve_spread: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_tx_modulate_frames_spread(None, None, 2, 1, 4, None, 320, None) == ERR_INVALID
    assert b"ofdm_tx_modulate_frames_spread: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_dft_despread_frames(None, None, 1, 1, 12, 12, None, 12, 0.0, 2, 0, 0.0, None, 0, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_dft_despread_frames: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_despread(None, 12, 1) == ERR_INVALID and b"ofdm_rx_reserve_despread: null handle" in lib.ofdm_last_error()
    assert lib.ofdm_rx_demod_frames_despread(None, None, 1, 64, 64, None, None, 0, 0.0, None, 0, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_rx_demod_frames_despread: null handle" in lib.ofdm_last_error()


def _smooth(m):
    for p in (2, 3, 5):
        while m % p == 0:
            m //= p
    return m == 1


def test_size_ok_against_a_factorisation(lib):
    import ofdm_mi355x as om
    ok = [m for m in range(-3, 4201) if lib.ofdm_dft_size_ok(m) == 1]
    assert ok == [m for m in range(1, 4097) if _smooth(m)] and len(ok) == 137
    assert om.dft_size_ok(1200) and not om.dft_size_ok(1201) and not om.dft_size_ok(0) and not om.dft_size_ok(2 ** 40)
    for m in (60, 75, 150, 300, 600, 1200, 2400):
        assert om.dft_size_ok(m)
    for n_rb in range(1, 111):
        assert om.dft_size_ok(12 * n_rb) == _smooth(n_rb)
    assert sum(_smooth(n) for n in range(1, 111)) == 35


def test_plan_info(lib):
    import ctypes as C
    import ofdm_mi355x as om
    assert om.dft_plan_info(1) == (0, 0, 256)
    assert om.dft_plan_info(12) == (2, 0, 64)                # 3 x 4, four lanes per row
    assert om.dft_plan_info(60) == (3, 0, 16)                # 3 x 5 x 4
    assert om.dft_plan_info(1200) == (5, 0, 1)               # 3 x 5 x 5 x 4 x 4
    assert om.dft_plan_info(2187) == (7, 0, 1)
    assert om.dft_plan_info(4096) == (6, 0, 1)
    with pytest.raises(ValueError, match="ofdm_dft_plan_info"):
        om.dft_plan_info(7)
    assert lib.ofdm_dft_plan_info(12, None, None, None) == 0
    n = C.c_int32(-1)
    assert lib.ofdm_dft_plan_info(4100, C.byref(n), None, None) == ERR_INVALID and n.value == -1
