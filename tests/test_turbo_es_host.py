"""The early-termination calls' C ABI without a GPU: the library exports them, the ctypes table and the engine carry them, and the
argument checks return OFDM_ERR_INVALID before the handle is looked at -- so that they can be reached here with a handle that
is only an address: a block of zeroed host memory that a correct call never reads."""
import ctypes as C
import os

import pytest

import turbo_cases as tc

NEW = ("ofdm_rx_reserve_turbo_es", "ofdm_turbo_decode_es_frames", "ofdm_rx_reserve_tb_es", "ofdm_tb_decode_es_frames")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import ofdm_mi355x
    from ofdm_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return ofdm_mi355x.load()


def test_library_and_package_export_the_early_termination_calls(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    for name in ("reserve_turbo_es", "turbo_decode_es_frames", "reserve_tb_es", "tb_decode_es_frames"):
        assert callable(getattr(om.RxEngine, name))
    assert [f[0] for f in _lib.TurboEsOut._fields_] == ["bits", "bits_mode", "llr", "iters", "crc_ok", "stat_stride"]
    assert [f[0] for f in _lib.TbEsOut._fields_] == ["payload", "payload_mode", "tb_ok", "cb_ok", "syndrome", "cb_iters"]
    assert lib.ofdm_abi_version() == 1


def test_argument_errors_are_invalid_before_the_handle_is_used(lib):
    import ofdm_mi355x as om
    from ofdm_mi355x import _lib
    K, bps = 40, 4
    f1, f2 = tc.QPP[K]
    per = 3 * K + 12
    fake = C.create_string_buffer(1 << 16)                   # never read: every call below is refused on its arguments
    h = C.addressof(fake)

    def call(handle=h, n_seg=2, stride=bps * per, bps_=bps, K_=K, f1_=f1, f2_=f2, kind=om.CRC24B, lo=1, hi=6, stat_stride=0):
        out = _lib.TurboEsOut(None, om.BITS_UNPACKED, None, None, None, stat_stride)
        return lib.ofdm_turbo_decode_es_frames(handle, None, n_seg, stride, bps_, K_, f1_, f2_, kind, lo, hi, C.byref(out), None)

    assert call(handle=None) == ERR_INVALID and b"null handle" in lib.ofdm_last_error()
    for kw, text in ((dict(lo=0), b"min_iter"), (dict(lo=4, hi=3), b"min_iter"), (dict(hi=17), b"max_iter"), (dict(kind=4), b"crc_kind"),
                     (dict(kind=-1), b"crc_kind"), (dict(f1_=2), b"permutation"), (dict(stat_stride=1), b"stat_stride"),
                     (dict(stat_stride=bps - 1), b"stat_stride"), (dict(stat_stride=-1), b"stat_stride"), (dict(K_=44), b"K must"),
                     (dict(stride=bps * per - 1), b"seg_stride")):
        assert call(**kw) == ERR_INVALID, kw
        err = lib.ofdm_last_error()
        assert b"ofdm_turbo_decode_es_frames" in err and text in err, (kw, err)
    assert call() == 0                                       # an `out` without any pointer: a no-op, the handle is not touched
    assert call(stat_stride=bps) == 0 and call(stat_stride=bps + 3) == 0 and call(lo=16, hi=16) == 0 and call(n_seg=0) == 0

    assert lib.ofdm_rx_reserve_turbo_es(None, 8, K) == ERR_INVALID and b"ofdm_rx_reserve_turbo_es" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_turbo_es(h, 8, 44) == ERR_INVALID and lib.ofdm_rx_reserve_turbo_es(h, -1, K) == ERR_INVALID
    assert lib.ofdm_rx_reserve_tb_es(None, 1, 80, 64) == ERR_INVALID and b"ofdm_rx_reserve_tb_es" in lib.ofdm_last_error()
    assert lib.ofdm_rx_reserve_tb_es(h, 1, 81, 64) == ERR_INVALID

    A, Z = 80, 64
    G = 3 * (3 * 64 + 12)
    tb_out = _lib.TbEsOut(None, om.BITS_UNPACKED, None, None, None, None)

    def tb(handle=h, lo=1, hi=6, out=tb_out, A_=A):
        return lib.ofdm_tb_decode_es_frames(handle, None, 1, G, A_, Z, G, 1, 0, *tc.QPP[56], *tc.QPP[64], 0, None, lo, hi, 0, None, 1000,
                                            C.byref(out) if out is not None else None, None)

    assert tb(handle=None) == ERR_INVALID and b"null handle" in lib.ofdm_last_error()
    for kw in (dict(lo=0), dict(lo=3, hi=2), dict(hi=17), dict(out=None), dict(A_=81)):
        assert tb(**kw) == ERR_INVALID, kw
        assert b"ofdm_tb_decode_es_frames" in lib.ofdm_last_error()
