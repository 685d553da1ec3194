"""The C ABI of receive diversity for multi-user allocations of DFT-spread OFDM without a GPU: the library exports the three
calls, the ctypes table and the engine carry them, the header's block compiles as plain C, a null handle is refused by name, and
every refusal that the arguments alone decide returns OFDM_ERR_INVALID with its reason before the handle's device is touched --
so that it can be reached here with a handle that is only a block of zeroed host memory (which has no allocation set: that
refusal comes last).  The refusals that need a set in force (row_len < max(start + M), packed bits that do not fill bytes, the
workgroup count of a given set) are in test_gpu_mrc_despread_alloc.py: a set can only be installed on a device."""
import ctypes as C
import os

import pytest

NEW = ("ofdm_rx_reserve_mrc_despread_alloc", "ofdm_combine_despread_alloc_frames", "ofdm_rx_demod_frames_mrc_despread_alloc")
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
    for name in ("reserve_mrc_despread_alloc", "combine_despread_alloc_frames", "demod_frames_mrc_despread_alloc"):
        assert callable(getattr(om.RxEngine, name))
    assert len(_lib.PROTOTYPES["ofdm_rx_reserve_mrc_despread_alloc"][1]) == 4
    assert len(_lib.PROTOTYPES["ofdm_combine_despread_alloc_frames"][1]) == 16
    assert len(_lib.PROTOTYPES["ofdm_rx_demod_frames_mrc_despread_alloc"][1]) == 14
    assert lib.ofdm_abi_version() == 1


def test_engine_keywords_are_those_of_the_parent_calls():
    import inspect
    import ofdm_mi355x as om
    stage = list(inspect.signature(om.RxEngine.combine_despread_alloc_frames).parameters)
    single = list(inspect.signature(om.RxEngine.combine_despread_frames).parameters)
    alloc = list(inspect.signature(om.RxEngine.dft_despread_alloc_frames).parameters)
    assert stage == [("row_len" if k == "M" else k) for k in single if k != "modulation"]         # the set holds the sizes
    assert "row_len" in alloc and set(stage) <= set(single) | set(alloc)
    comp = list(inspect.signature(om.RxEngine.demod_frames_mrc_despread_alloc).parameters)
    assert comp == list(inspect.signature(om.RxEngine.demod_frames_mrc_despread).parameters)


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
                   '_Static_assert(OFDM_ABI_VERSION == 1, "the ABI version stays");\n'
                   '_Static_assert(sizeof(ofdm_mrc_despread_out) == 6 * sizeof(void*), "ofdm_mrc_despread_out is reused unchanged");\n'
                   'int (*a)(ofdm_rx*, int32_t, int64_t, int64_t) = ofdm_rx_reserve_mrc_despread_alloc;\n'
                   'int (*b)(ofdm_rx*, const float*, int32_t, int64_t, int64_t, int64_t, int64_t, const float*, int64_t, float, int32_t,\n'
                   '         const double*, const double*, int32_t, const ofdm_mrc_despread_out*, void*) = ofdm_combine_despread_alloc_frames;\n'
                   'int64_t (*c)(ofdm_rx*, const float*, int32_t, int64_t, int64_t, int64_t, float*, int32_t*, int32_t, const double*,\n'
                   '             const double*, int32_t, const ofdm_mrc_despread_out*, void*) = ofdm_rx_demod_frames_mrc_despread_alloc;\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_argument_errors_are_invalid_before_the_device_is_touched(lib):
    from ofdm_mi355x import _lib
    fake = C.create_string_buffer(1 << 16)                   # a zeroed stand-in: no set, and its device is never touched
    h = C.addressof(fake)
    sink = C.create_string_buffer(64)
    other = C.create_string_buffer(64)
    p, q = C.addressof(sink), C.addressof(other)
    nan, inf = float("nan"), float("inf")

    def nv(*v):
        return (C.c_double * len(v))(*v)

    def call(handle=h, sym=p, csi=p, n_branch=2, n_seg=2, rows=3, row_len=60, seg_stride=None, csi_stride=None, rho=0.03, mode=GIVEN,
             var=nv(0.1, 0.2), sigma2=None, bits_mode=UNPACKED, out="llr"):
        # "sym!": that output at the input's own address
        o = None if out is None else _lib.MrcDespreadOut(**{k.rstrip("!"): (p if k.endswith("!") else q) for k in out.split()})
        return lib.ofdm_combine_despread_alloc_frames(handle, sym, n_branch, n_seg, rows, row_len,
                                                      rows * row_len if seg_stride is None else seg_stride, csi,
                                                      row_len if csi_stride is None else csi_stride, rho, mode, var, sigma2, bits_mode,
                                                      None if o is None else C.byref(o), None)

    name = b"ofdm_combine_despread_alloc_frames"
    assert call(handle=None) == ERR_INVALID and name + b": null handle" in lib.ofdm_last_error()
    for kw, text in ((dict(csi=None), b"d_csi is required"),
                     (dict(n_seg=-1), b"negative count"), (dict(rows=-1), b"negative count"), (dict(row_len=-1), b"negative count"),
                     (dict(n_branch=0), b"n_branch"), (dict(n_branch=-1), b"n_branch"), (dict(n_branch=9, var=nv(*[0.1] * 9)), b"n_branch"),
                     (dict(seg_stride=3 * 60 - 1), b"seg_stride < rows"), (dict(csi_stride=59), b"csi_stride <"),
                     (dict(mode=EST), b"OFDM_MRC_NOISE_EST"), (dict(mode=3), b"noise_mode"), (dict(mode=-1), b"noise_mode"),
                     (dict(var=None), b"h_noise_var"), (dict(mode=SEG, sigma2=None), b"d_sigma2"),
                     (dict(var=nv(0.1, 0.0)), b"noise_var"), (dict(var=nv(-1.0, 0.1)), b"noise_var"), (dict(var=nv(0.1, nan)), b"noise_var"),
                     (dict(var=nv(inf, 0.1)), b"noise_var"), (dict(rho=-0.5), b"rho"), (dict(rho=nan), b"rho"), (dict(rho=inf), b"rho"),
                     (dict(out=None), b"no pointer"), (dict(out=""), b"no pointer"),
                     (dict(out="bits", bits_mode=NONE), b"bits_mode"), (dict(out="bits", bits_mode=7), b"bits_mode"),
                     (dict(out="sym!"), b"== d_sym"), (dict(out="llr comb!"), b"== d_sym"),
                     (dict(row_len=(1 << 30) + 1), b"index range"), (dict(rows=1 << 40, row_len=2, seg_stride=1 << 62), b"index range"),
                     (dict(n_seg=(1 << 30) + 1), b"index range"), (dict(n_branch=1, n_seg=(1 << 31) + 1, var=nv(0.1)), b"index range"),
                     (dict(n_seg=1 << 19, seg_stride=1 << 30), b"index range"), (dict(n_seg=1 << 19, csi_stride=1 << 30), b"index range"),
                     # n_branch*n_seg = 2^31 units pass; 2^31 segments are more than 2^31 - 1 workgroups for every set there is
                     (dict(n_branch=1, var=nv(0.1), n_seg=1 << 31, rows=1, row_len=12), b"workgroups"),
                     # every argument is fine: the stand-in has no set
                     (dict(), b"no allocation set"), (dict(mode=SEG, sigma2=p), b"no allocation set"),
                     (dict(out="sym llr bits beta weight comb"), b"no allocation set"),
                     (dict(n_branch=1, var=nv(0.1), n_seg=(1 << 31) - 1, rows=1, row_len=12), b"no allocation set")):
        assert call(**kw) == ERR_INVALID, kw
        err = lib.ofdm_last_error()
        assert name in err and text in err, (kw, err)
    assert not any(fake.raw)                                 # nothing was stored

    r = lib.ofdm_rx_reserve_mrc_despread_alloc
    assert r(None, 2, 1, 60) == ERR_INVALID and b"ofdm_rx_reserve_mrc_despread_alloc: null handle" in lib.ofdm_last_error()
    for args in ((0, 1, 60), (9, 1, 60), (-1, 1, 60), (2, -1, 60), (2, 1, -1), (2, (1 << 30) + 1, 60), (2, 1, (1 << 30) + 1),
                 (8, 1 << 28, 1 << 20)):
        assert r(h, *args) == ERR_INVALID, args
        assert b"ofdm_rx_reserve_mrc_despread_alloc" in lib.ofdm_last_error()

    out = _lib.MrcDespreadOut(llr=q)
    two = nv(0.1, 0.2)
    f = lib.ofdm_rx_demod_frames_mrc_despread_alloc
    who = b"ofdm_rx_demod_frames_mrc_despread_alloc"
    assert f(None, p, 2, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert who + b": null handle" in lib.ofdm_last_error()
    assert f(h, p, 2, 1, 32, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID and who in lib.ofdm_last_error()
    assert f(h, None, 2, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert f(h, p, 0, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert b"n_branch" in lib.ofdm_last_error()
    assert f(h, p, 9, 1, 64, 64, p, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert f(h, p, 2, 1, 64, 64, None, None, GIVEN, two, None, NONE, C.byref(out), None) == ERR_INVALID
    assert b"needs d_eq" in lib.ofdm_last_error()
    assert not any(fake.raw)


def test_engine_checks_the_noise_arguments():
    """exactly one of noise_var / d_sigma2, and n_branch numbers: refused in Python, before the library is called"""
    import ofdm_mi355x as om
    e = object.__new__(om.RxEngine)                          # no handle: the checks come first
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.combine_despread_alloc_frames(e, 1, 2, 1, 1, 12, 12, 1, 12, 0.03, d_llr=1)
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.combine_despread_alloc_frames(e, 1, 2, 1, 1, 12, 12, 1, 12, 0.03, noise_var=[0.1, 0.1], d_sigma2=1, d_llr=1)
    with pytest.raises(ValueError, match="n_branch"):
        om.RxEngine.combine_despread_alloc_frames(e, 1, 2, 1, 1, 12, 12, 1, 12, 0.03, noise_var=[0.1], d_llr=1)
    with pytest.raises(ValueError, match="exactly one"):
        om.RxEngine.demod_frames_mrc_despread_alloc(e, 1, 2, 1, 64, 64, 1)
    with pytest.raises(ValueError, match="n_branch"):
        om.RxEngine.demod_frames_mrc_despread_alloc(e, 1, 2, 1, 64, 64, 1, noise_var=[0.1, 0.2, 0.3])
