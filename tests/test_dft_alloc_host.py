"""The multi-user allocation calls' C ABI without a GPU: the library exports them, the ctypes table and the engines carry them,
the header's block compiles as plain C, a null handle is refused by name, every refusal of the set and of the stage that the
arguments alone decide is made before the handle's device is touched, and ofdm_alloc_layout answers with the contract's formula."""
import ctypes as C
import os

import numpy as np
import pytest

import dft_alloc_ref as aref

NEW = ("ofdm_alloc_layout", "ofdm_rx_set_allocations", "ofdm_tx_set_allocations", "ofdm_rx_reserve_despread_alloc",
       "ofdm_dft_despread_alloc_frames", "ofdm_rx_demod_frames_despread_alloc", "ofdm_tx_dft_spread_alloc",
       "ofdm_tx_reserve_spread_alloc", "ofdm_tx_modulate_frames_alloc")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def i32(*v):
    return np.array(v, np.int32)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_library_and_package_export_the_calls(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    for name in ("set_allocations", "reserve_despread_alloc", "dft_despread_alloc_frames", "demod_frames_despread_alloc"):
        assert callable(getattr(om.RxEngine, name))
    for name in ("set_allocations", "reserve_spread_alloc", "dft_spread_alloc", "modulate_frames_alloc"):
        assert callable(getattr(om.TxEngine, name))
    assert callable(om.alloc_layout)
    assert len(_lib.PROTOTYPES["ofdm_dft_despread_alloc_frames"][1]) == 15
    assert len(_lib.PROTOTYPES["ofdm_rx_demod_frames_despread_alloc"][1]) == 13


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
                   '_Static_assert(OFDM_MAX_ALLOCS == 32, "the cap of a set");\n'
                   '_Static_assert(OFDM_ABI_VERSION == 1, "the ABI version stays");\n'
                   '_Static_assert(sizeof(ofdm_despread_out) == 5 * sizeof(void*), "ofdm_despread_out is reused unchanged");\n'
                   'int (*a)(int32_t, const int32_t*, const int32_t*, int64_t, int64_t, int32_t, int64_t*, int64_t*, int64_t*, int64_t*)\n'
                   '    = ofdm_alloc_layout;\n'
                   'int (*b)(ofdm_rx*, int32_t, const int32_t*, const int32_t*, const int32_t*) = ofdm_rx_set_allocations;\n'
                   'int (*c)(ofdm_tx*, int32_t, const int32_t*, const int32_t*) = ofdm_tx_set_allocations;\n'
                   'int (*d)(ofdm_rx*, int64_t) = ofdm_rx_reserve_despread_alloc;\n'
                   'int (*e)(ofdm_rx*, const float*, int64_t, int64_t, int64_t, int64_t, const float*, int64_t, float, int32_t, double,\n'
                   '         const double*, int32_t, const ofdm_despread_out*, void*) = ofdm_dft_despread_alloc_frames;\n'
                   'int64_t (*f)(ofdm_rx*, const float*, int64_t, int64_t, int64_t, float*, int32_t*, int32_t, double, const double*,\n'
                   '             int32_t, const ofdm_despread_out*, void*) = ofdm_rx_demod_frames_despread_alloc;\n'
                   'int (*g)(ofdm_tx*, const float*, int64_t, int64_t, float*, void*) = ofdm_tx_dft_spread_alloc;\n'
                   'int (*h)(ofdm_tx*, int64_t) = ofdm_tx_reserve_spread_alloc;\n'
                   'int64_t (*i)(ofdm_tx*, const uint8_t*, int32_t, int64_t, int32_t, float*, int64_t, void*) = ofdm_tx_modulate_frames_alloc;\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_null_handle_is_refused_by_name(lib):
    from ofdm_mi355x import _lib
    out = _lib.DespreadOut(1, None, None, None, None)
    s, m, q = i32(0), i32(12), i32(2)
    calls = (("ofdm_rx_set_allocations", lambda: lib.ofdm_rx_set_allocations(None, 1, p(s), p(m), p(q))),
             ("ofdm_tx_set_allocations", lambda: lib.ofdm_tx_set_allocations(None, 1, p(s), p(m))),
             ("ofdm_rx_reserve_despread_alloc", lambda: lib.ofdm_rx_reserve_despread_alloc(None, 1)),
             ("ofdm_dft_despread_alloc_frames",
              lambda: lib.ofdm_dft_despread_alloc_frames(None, None, 1, 1, 12, 12, None, 12, 0.0, 0, 0.0, None, 0, C.byref(out), None)),
             ("ofdm_rx_demod_frames_despread_alloc",
              lambda: lib.ofdm_rx_demod_frames_despread_alloc(None, None, 1, 64, 64, None, None, 0, 0.0, None, 0, C.byref(out), None)),
             ("ofdm_tx_dft_spread_alloc", lambda: lib.ofdm_tx_dft_spread_alloc(None, None, 1, 12, None, None)),
             ("ofdm_tx_reserve_spread_alloc", lambda: lib.ofdm_tx_reserve_spread_alloc(None, 1)),
             ("ofdm_tx_modulate_frames_alloc", lambda: lib.ofdm_tx_modulate_frames_alloc(None, None, 2, 1, 4, None, 320, None)))
    for name, call in calls:
        assert call() == ERR_INVALID, name
        assert (name + ": null handle").encode() in lib.ofdm_last_error(), name


def test_the_set_is_refused_before_the_device_is_touched(lib):
    """a zeroed block stands in for a handle: every refusal below is decided by the lists alone"""
    block = C.create_string_buffer(1 << 16)
    dummy = C.cast(block, C.c_void_p)
    bad = {"overlap": ((0, 12, 2), (11, 12, 4)),
           "overlap, unsorted": ((36, 24, 2), (0, 60, 4)),
           "start + M > 4096": ((4085, 12, 2),),
           "M must be": ((0, 7, 2),),
           "M must be ": ((0, 0, 2),),
           "start < 0": ((-1, 12, 2),),
           "modulation must be": ((0, 12, 1),),
           "modulation must be ": ((0, 12, 3),),
           "OFDM_MAX_ALLOCS": tuple((12 * k, 12, 2) for k in range(33))}
    for why, allocs in bad.items():
        assert aref.check_set(list(allocs)) is not None, why
        s, m, q = (i32(*[a[k] for a in allocs]) for k in range(3))
        assert lib.ofdm_rx_set_allocations(dummy, len(allocs), p(s), p(m), p(q)) == ERR_INVALID, why
        msg = lib.ofdm_last_error()
        assert b"ofdm_rx_set_allocations" in msg and why.split(",")[0].strip().encode() in msg, (why, msg)
        if not why.startswith("modulation"):
            assert lib.ofdm_tx_set_allocations(dummy, len(allocs), p(s), p(m)) == ERR_INVALID, why
            assert b"ofdm_tx_set_allocations" in lib.ofdm_last_error()
    s, m, q = i32(0), i32(12), i32(2)
    assert lib.ofdm_rx_set_allocations(dummy, -1, p(s), p(m), p(q)) == ERR_INVALID
    assert lib.ofdm_rx_set_allocations(dummy, 1, None, p(m), p(q)) == ERR_INVALID and b"null array" in lib.ofdm_last_error()
    assert lib.ofdm_rx_set_allocations(dummy, 1, p(s), p(m), None) == ERR_INVALID
    assert lib.ofdm_tx_set_allocations(dummy, 1, p(s), None) == ERR_INVALID
    assert not any(block.raw)                                # nothing was stored


def test_without_a_set_the_calls_refuse(lib):
    from ofdm_mi355x import _lib
    block = C.create_string_buffer(1 << 16)
    dummy = C.cast(block, C.c_void_p)
    buf = C.cast(C.create_string_buffer(64), C.c_void_p)
    out = _lib.DespreadOut(buf.value, None, None, None, None)
    assert lib.ofdm_dft_despread_alloc_frames(dummy, buf, 1, 1, 12, 12, None, 12, 0.0, 0, 0.0, None, 0, C.byref(out), None) == ERR_INVALID
    assert b"ofdm_dft_despread_alloc_frames: no allocation set" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_despread_alloc(dummy, 4) == ERR_INVALID and b"no allocation set" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_despread_alloc(dummy, -1) == ERR_INVALID
    assert lib.ofdm_tx_dft_spread_alloc(dummy, buf, 1, 12, buf, None) == ERR_INVALID
    assert b"ofdm_tx_dft_spread_alloc: no allocation set" in lib.ofdm_last_error()
    assert lib.ofdm_tx_reserve_spread_alloc(dummy, -1) == ERR_INVALID


def test_alloc_layout_against_the_formula(lib):
    import ofdm_mi355x as om
    sets = ([(0, 12, 2), (12, 24, 4), (36, 24, 6)], [(1, 25, 4), (27, 1, 2), (31, 45, 6)], [(0, 1200, 6)],
            [(12 * k, 12, 2 + 2 * (k % 3)) for k in range(32)])
    for allocs in sets:
        M, mod = [a[1] for a in allocs], [a[2] for a in allocs]
        for n_seg, rows in ((1, 1), (3, 17), (0, 5), (2, 0)):
            for mode, packed in ((om.BITS_UNPACKED, False), (om.BITS_PACKED, True), (om.BITS_NONE, False)):
                if packed and any(m * b % 8 for m, b in zip(M, mod)):
                    with pytest.raises(ValueError, match="ofdm_alloc_layout: packed"):
                        om.alloc_layout(M, mod, n_seg, rows, mode)
                    continue
                got = om.alloc_layout(M, mod, n_seg, rows, mode)
                so, lo, bo, tot = aref.layout(allocs, n_seg, rows, packed)
                assert list(got["sym_off"]) == so and list(got["llr_off"]) == lo and (got["sym"], got["llr"]) == tot[:2]
                if mode == om.BITS_NONE:
                    assert not got["bits_off"].any() and got["bits"] == 0
                else:
                    assert list(got["bits_off"]) == bo and got["bits"] == tot[2]
    assert lib.ofdm_alloc_layout(1, p(i32(12)), p(i32(2)), 1, 1, 0, None, None, None, None) == 0       # outputs may be NULL
    for M, mod, kw in (([7], [2], {}), ([12], [1], {}), ([12] * 33, [2] * 33, {}), ([], [], {}), ([12], [2], dict(n_seg=-1)),
                       ([12], [2], dict(rows=-1)), ([12], [2], dict(bits_mode=9))):
        with pytest.raises(ValueError, match="ofdm_alloc_layout"):
            om.alloc_layout(M, mod, kw.get("n_seg", 1), kw.get("rows", 1), kw.get("bits_mode", 0))
