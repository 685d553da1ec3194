"""The refused and no-op calls of the codec side of the C ABI -- every public call of csrc/capi_tbcc.hip, capi_bitproc.hip,
capi_turbo.hip and capi_tb.hip -- as one table, shared by tests/test_gpu_codec_refusals.py and the recorder
tests/golden/gen_codec_refusals.py.  A case is (id, call, keyword arguments); run() makes the call and returns
[status, ofdm_last_error() text], the text "" where the call did not fail.

No case launches a kernel or grows a workspace: a call whose arguments are all fine is given null buffers (its last refusal),
nothing to do (n_seg == 0, nothing wanted) or, for a reserve call, a batch of 0.  Each refusal text of a call appears at the first
argument value that triggers it and -- in the case behind it -- at the last value that does not.  Where that last value would
allocate (the upper limit of a reserve call's count) only the refused side is listed."""
import ctypes as C

P, U = 1, 2                                  # OFDM_BITS_PACKED, OFDM_BITS_UNPACKED
MAXB = (1 << 31) - 1                         # blocks of one launch
ITEMS = 1 << 40                              # n_seg * stride
GOLD_MAX = (1 << 31) - 1600
TB_ITEMS = 1 << 38

# call -> parameter names in the header's order; "h" takes "TX" / "RX" / None, "BUF" stands for a device address
CALLS = {
    "ofdm_tbcc_blocks": ["seg_bits", "K"],
    "ofdm_tbcc_rm_blocks": ["seg_bits", "K", "E"],
    "ofdm_tx_tbcc_encode_frames": ["h", "d_info", "info_mode", "n_seg", "blocks_per_seg", "K", "d_coded", "coded_mode", "seg_bits", "stream"],
    "ofdm_tx_tbcc_encode_rm_frames": ["h", "d_info", "info_mode", "n_seg", "blocks_per_seg", "K", "E", "d_coded", "coded_mode", "seg_bits",
                                      "stream"],
    "ofdm_rx_reserve_tbcc": ["h", "n_blocks", "K"],
    "ofdm_tbcc_decode_frames": ["h", "d_llr", "n_seg", "seg_stride", "blocks_per_seg", "K", "out", "stream"],
    "ofdm_tbcc_rate_dematch_frames": ["h", "d_llr", "n_seg", "seg_stride", "blocks_per_seg", "K", "E", "d_out", "out_stride", "stream"],
    "ofdm_tbcc_decode_rm_frames": ["h", "d_llr", "n_seg", "seg_stride", "blocks_per_seg", "K", "E", "out", "stream"],
    "ofdm_crc_bits": ["kind"],
    "ofdm_crc_compute": ["kind", "host_bits", "A", "crc"],
    "ofdm_crc_compute_long": ["kind", "host_bits", "n_bits", "crc"],
    "ofdm_gold_bits": ["c_init", "first", "n", "host_out"],
    "ofdm_tx_reserve_bitproc": ["h"],
    "ofdm_rx_reserve_bitproc": ["h"],
    "ofdm_tx_crc_attach_frames": ["h", "d_payload", "payload_mode", "n_blocks", "A", "kind", "mask", "d_mask", "d_info", "info_mode", "stream"],
    "ofdm_crc_check_frames": ["h", "d_info", "info_mode", "n_blocks", "A", "kind", "mask", "d_mask", "out", "stream"],
    "ofdm_tx_scramble_frames": ["h", "d_in", "mode", "n_seg", "seg_bits", "d_cinit", "d_out", "stream"],
    "ofdm_descramble_llr_frames": ["h", "d_llr", "n_seg", "seg_stride", "seg_bits", "d_cinit", "d_out", "out_stride", "stream"],
    "ofdm_turbo_blocks": ["seg_bits", "K"],
    "ofdm_turbo_qpp_check": ["K", "f1", "f2"],
    "ofdm_tx_turbo_encode_frames": ["h", "d_info", "info_mode", "n_seg", "blocks_per_seg", "K", "f1", "f2", "d_coded", "coded_mode", "seg_bits",
                                    "stream"],
    "ofdm_rx_reserve_turbo": ["h", "n_blocks", "K"],
    "ofdm_turbo_decode_frames": ["h", "d_llr", "n_seg", "seg_stride", "blocks_per_seg", "K", "f1", "f2", "n_iter", "out", "stream"],
    "ofdm_rx_reserve_turbo_es": ["h", "n_blocks", "K"],
    "ofdm_turbo_decode_es_frames": ["h", "d_llr", "n_seg", "seg_stride", "blocks_per_seg", "K", "f1", "f2", "crc_kind", "min_iter", "max_iter",
                                    "out", "stream"],
    "ofdm_turbo_rm_blocks": ["seg_bits", "K", "E"],
    "ofdm_turbo_rm_info": ["K", "Ncb", "rv", "k0", "n_avail"],
    "ofdm_tx_reserve_turbo_rm": ["h"],
    "ofdm_rx_reserve_turbo_rm": ["h"],
    "ofdm_tx_turbo_encode_rm_frames": ["h", "d_info", "info_mode", "n_seg", "blocks_per_seg", "K", "f1", "f2", "E", "Ncb", "rv", "d_rv",
                                       "d_coded", "coded_mode", "seg_bits", "stream"],
    "ofdm_turbo_rate_dematch_frames": ["h", "d_llr", "n_seg", "seg_stride", "blocks_per_seg", "K", "E", "Ncb", "rv", "d_rv", "accumulate",
                                       "d_out", "out_stride", "stream"],
    "ofdm_turbo_k_next": ["bits"],
    "ofdm_tb_geometry": ["A", "Z", "G", "q", "N_IR", "geom"],
    "ofdm_tx_reserve_tb": ["h", "n_tb", "A", "Z", "G", "q"],
    "ofdm_rx_reserve_tb": ["h", "n_tb", "A", "Z"],
    "ofdm_rx_reserve_tb_es": ["h", "n_tb", "A", "Z"],
    "ofdm_tx_tb_encode_frames": ["h", "d_payload", "payload_mode", "n_tb", "A", "Z", "G", "q", "N_IR", "f1_minus", "f2_minus", "f1_plus",
                                 "f2_plus", "rv", "d_rv", "d_cw", "cw_mode", "cw_bits", "stream"],
    "ofdm_tb_decode_frames": ["h", "d_llr", "n_tb", "llr_stride", "A", "Z", "G", "q", "N_IR", "f1_minus", "f2_minus", "f1_plus", "f2_plus",
                              "rv", "d_rv", "n_iter", "accumulate", "d_soft", "soft_stride", "out", "stream"],
    "ofdm_tb_decode_es_frames": ["h", "d_llr", "n_tb", "llr_stride", "A", "Z", "G", "q", "N_IR", "f1_minus", "f2_minus", "f1_plus", "f2_plus",
                                 "rv", "d_rv", "min_iter", "max_iter", "accumulate", "d_soft", "soft_stride", "out", "stream"],
}
OUT_TYPES = {"ofdm_tbcc_decode_frames": "TbccOut", "ofdm_tbcc_decode_rm_frames": "TbccOut", "ofdm_crc_check_frames": "CrcOut",
             "ofdm_turbo_decode_frames": "TurboOut", "ofdm_turbo_decode_es_frames": "TurboEsOut", "ofdm_tb_decode_frames": "TbOut",
             "ofdm_tb_decode_es_frames": "TbEsOut"}

WANT_BITS = {"bits": "BUF", "bits_mode": U}
TB = dict(A=40, Z=0, G=200, q=2, N_IR=0, f1_minus=0, f2_minus=0, f1_plus=7, f2_plus=16)       # one block of K = 64: 204 soft floats
# a call every check of which passes, up to its last refusal (null buffers) -- or, for the calls without one, a plain success
BASE = {
    "ofdm_tbcc_blocks": dict(seg_bits=72, K=24),
    "ofdm_tbcc_rm_blocks": dict(seg_bits=10, K=24, E=10),
    "ofdm_tx_tbcc_encode_frames": dict(h="TX", d_info=None, info_mode=U, n_seg=1, blocks_per_seg=1, K=24, d_coded=None, coded_mode=U,
                                       seg_bits=72, stream=None),
    "ofdm_tx_tbcc_encode_rm_frames": dict(h="TX", d_info=None, info_mode=U, n_seg=1, blocks_per_seg=1, K=24, E=40, d_coded=None,
                                          coded_mode=U, seg_bits=40, stream=None),
    "ofdm_rx_reserve_tbcc": dict(h="RX", n_blocks=0, K=24),
    "ofdm_tbcc_decode_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=72, blocks_per_seg=1, K=24, out=WANT_BITS, stream=None),
    "ofdm_tbcc_rate_dematch_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=40, blocks_per_seg=1, K=24, E=40, d_out=None,
                                          out_stride=72, stream=None),
    "ofdm_tbcc_decode_rm_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=40, blocks_per_seg=1, K=24, E=40, out=WANT_BITS,
                                       stream=None),
    "ofdm_crc_bits": dict(kind=0),
    "ofdm_crc_compute": dict(kind=0, host_bits=None, A=8, crc=None),
    "ofdm_crc_compute_long": dict(kind=0, host_bits=None, n_bits=8, crc=None),
    "ofdm_gold_bits": dict(c_init=1, first=0, n=8, host_out=None),
    "ofdm_tx_reserve_bitproc": dict(h="TX"),
    "ofdm_rx_reserve_bitproc": dict(h="RX"),
    "ofdm_tx_crc_attach_frames": dict(h="TX", d_payload=None, payload_mode=U, n_blocks=1, A=8, kind=0, mask=0, d_mask=None, d_info=None,
                                      info_mode=U, stream=None),
    "ofdm_crc_check_frames": dict(h="RX", d_info=None, info_mode=U, n_blocks=1, A=8, kind=0, mask=0, d_mask=None, out={"ok": "BUF"},
                                  stream=None),
    "ofdm_tx_scramble_frames": dict(h="TX", d_in=None, mode=U, n_seg=1, seg_bits=16, d_cinit=None, d_out=None, stream=None),
    "ofdm_descramble_llr_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=16, seg_bits=16, d_cinit=None, d_out=None, out_stride=16,
                                       stream=None),
    "ofdm_turbo_blocks": dict(seg_bits=132, K=40),
    "ofdm_turbo_qpp_check": dict(K=40, f1=3, f2=10),
    "ofdm_tx_turbo_encode_frames": dict(h="TX", d_info=None, info_mode=U, n_seg=1, blocks_per_seg=1, K=40, f1=3, f2=10, d_coded=None,
                                        coded_mode=U, seg_bits=132, stream=None),
    "ofdm_rx_reserve_turbo": dict(h="RX", n_blocks=0, K=40),
    "ofdm_turbo_decode_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=132, blocks_per_seg=1, K=40, f1=3, f2=10, n_iter=1,
                                     out=WANT_BITS, stream=None),
    "ofdm_rx_reserve_turbo_es": dict(h="RX", n_blocks=0, K=40),
    "ofdm_turbo_decode_es_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=132, blocks_per_seg=1, K=40, f1=3, f2=10, crc_kind=0,
                                        min_iter=1, max_iter=1, out=WANT_BITS, stream=None),
    "ofdm_turbo_rm_blocks": dict(seg_bits=10, K=40, E=10),
    "ofdm_turbo_rm_info": dict(K=40, Ncb=0, rv=0, k0=None, n_avail=None),
    "ofdm_tx_reserve_turbo_rm": dict(h="TX"),
    "ofdm_rx_reserve_turbo_rm": dict(h="RX"),
    "ofdm_tx_turbo_encode_rm_frames": dict(h="TX", d_info=None, info_mode=U, n_seg=1, blocks_per_seg=1, K=40, f1=3, f2=10, E=100, Ncb=0,
                                           rv=0, d_rv=None, d_coded=None, coded_mode=U, seg_bits=100, stream=None),
    "ofdm_turbo_rate_dematch_frames": dict(h="RX", d_llr=None, n_seg=1, seg_stride=100, blocks_per_seg=1, K=40, E=100, Ncb=0, rv=0,
                                           d_rv=None, accumulate=0, d_out=None, out_stride=132, stream=None),
    "ofdm_turbo_k_next": dict(bits=40),
    "ofdm_tb_geometry": dict(A=40, Z=0, G=200, q=2, N_IR=0, geom="GEOM"),
    "ofdm_tx_reserve_tb": dict(h="TX", n_tb=0, A=40, Z=0, G=200, q=2),
    "ofdm_rx_reserve_tb": dict(h="RX", n_tb=0, A=40, Z=0),
    "ofdm_rx_reserve_tb_es": dict(h="RX", n_tb=0, A=40, Z=0),
    "ofdm_tx_tb_encode_frames": dict(h="TX", d_payload=None, payload_mode=U, n_tb=1, rv=0, d_rv=None, d_cw=None, cw_mode=U, cw_bits=200,
                                     stream=None, **TB),
    "ofdm_tb_decode_frames": dict(h="RX", d_llr=None, n_tb=1, llr_stride=200, rv=0, d_rv=None, n_iter=1, accumulate=0, d_soft=None,
                                  soft_stride=204, out={"tb_ok": "BUF"}, stream=None, **TB),
    "ofdm_tb_decode_es_frames": dict(h="RX", d_llr=None, n_tb=1, llr_stride=200, rv=0, d_rv=None, min_iter=1, max_iter=1, accumulate=0,
                                     d_soft=None, soft_stride=204, out={"tb_ok": "BUF"}, stream=None, **TB),
}

CASES = []


def case(call, name, **over):
    unknown = set(over) - set(CALLS[call])
    assert not unknown, (call, unknown)
    CASES.append(("%s/%s" % (call[5:], name), call, dict(BASE[call], **over)))


def edge(call, name, bad, good=None):
    """the first value(s) a refusal triggers at, and the last that it does not"""
    case(call, name + "-refused", **bad)
    if good is not None:
        case(call, name + "-passes", **good)


def tbcc_geometry(call, rm=False):
    kmax = {"seg_bits": 6144, "seg_stride": 6144, "out_stride": 6144}
    roomy = {k: v for k, v in kmax.items() if k in CALLS[call] and not (rm and k != "out_stride")}
    edge(call, "K-low", dict(K=16), dict(K=24))
    edge(call, "K-high", dict(K=2056), dict(K=2048, **roomy))
    edge(call, "K-multiple", dict(K=28), dict(K=32, **{k: 96 for k in roomy}))
    if rm:
        edge(call, "E-low", dict(E=0), dict(E=1))
        edge(call, "E-high", dict(E=48 * 24 + 1), dict(E=48 * 24, **{k: 48 * 24 for k in ("seg_bits", "seg_stride") if k in CALLS[call]}))


def turbo_geometry(call):
    big = {k: 3 * 6144 + 12 for k in ("seg_bits", "seg_stride", "out_stride") if k in CALLS[call]}
    rm = "E" in CALLS[call]
    if rm:
        big = {k: v for k, v in big.items() if k == "out_stride"}
    edge(call, "K-low", dict(K=32), dict(K=40))
    edge(call, "K-high", dict(K=6152), dict(K=6144, **big, **({"f1": 263, "f2": 480} if "f1" in CALLS[call] else {})))
    edge(call, "K-multiple", dict(K=44), dict(K=48, **({"f1": 7, "f2": 12} if "f1" in CALLS[call] else {}),
                                               **{k: 156 for k in big}))


def qpp_edges(call):
    edge(call, "f1-negative", dict(f1=-1), dict(f1=0))
    edge(call, "f1-high", dict(f1=40), dict(f1=39))
    edge(call, "f2-negative", dict(f2=-1), dict(f2=0))
    edge(call, "f2-high", dict(f2=40), dict(f2=39))
    edge(call, "no-permutation", dict(f1=2, f2=10), dict(f1=3, f2=10))


def enc_edges(call, need):
    """the checks every encoder shares behind its geometry: need = the base call's coded bits per segment"""
    case(call, "null-handle", h=None)
    edge(call, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
    edge(call, "blocks-negative", dict(blocks_per_seg=-1), dict(blocks_per_seg=0))
    edge(call, "blocks-range", dict(n_seg=MAXB + 1), dict(n_seg=MAXB))
    edge(call, "info_mode-low", dict(info_mode=0), dict(info_mode=P))
    edge(call, "info_mode-high", dict(info_mode=3), dict(info_mode=U))
    edge(call, "coded_mode-low", dict(coded_mode=0), dict(coded_mode=P, seg_bits=(need + 7) // 8 * 8))
    edge(call, "coded_mode-high", dict(coded_mode=3), dict(coded_mode=U))
    edge(call, "seg_bits-short", dict(seg_bits=need - 1), dict(seg_bits=need))
    case(call, "seg_bits-negative-refused", seg_bits=-1, blocks_per_seg=0)
    edge(call, "packed-whole-bytes", dict(coded_mode=P, seg_bits=(need + 7) // 8 * 8 + 4), dict(coded_mode=P, seg_bits=(need + 7) // 8 * 8 + 8))
    edge(call, "items-one-segment", dict(seg_bits=ITEMS + 1), dict(seg_bits=ITEMS))
    edge(call, "items-product", dict(n_seg=2, seg_bits=ITEMS // 2 + 1), dict(n_seg=2, seg_bits=ITEMS // 2))
    case(call, "noop-no-segments", n_seg=0, d_info="BUF", d_coded="BUF")
    case(call, "noop-no-bits", blocks_per_seg=0, seg_bits=0, d_coded="BUF")
    case(call, "null-d_coded", d_info="BUF")
    case(call, "null-d_info", d_coded="BUF")


def dec_edges(call, need):
    """the checks every decoder shares behind its geometry: need = the base call's LLRs per segment"""
    case(call, "null-handle", h=None)
    edge(call, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
    edge(call, "blocks-negative", dict(blocks_per_seg=-1), dict(blocks_per_seg=0))
    edge(call, "blocks-range", dict(n_seg=MAXB + 1), dict(n_seg=MAXB))
    edge(call, "seg_stride-short", dict(seg_stride=need - 1), dict(seg_stride=need))
    edge(call, "items-one-segment", dict(seg_stride=ITEMS + 1), dict(seg_stride=ITEMS))
    edge(call, "items-product", dict(n_seg=2, seg_stride=ITEMS // 2 + 1), dict(n_seg=2, seg_stride=ITEMS // 2))
    edge(call, "bits_mode-low", dict(out={"bits": "BUF", "bits_mode": 0}), dict(out={"bits": "BUF", "bits_mode": P}))
    edge(call, "bits_mode-high", dict(out={"bits": "BUF", "bits_mode": 3}), dict(out={"bits": "BUF", "bits_mode": U}))
    case(call, "bits_mode-unread-without-bits", out={"bits_mode": 3})
    case(call, "noop-no-segments", n_seg=0, d_llr="BUF")
    case(call, "noop-no-blocks", blocks_per_seg=0, d_llr="BUF")
    case(call, "noop-null-out", out=None, d_llr="BUF")
    case(call, "noop-nothing-wanted", out={}, d_llr="BUF")
    case(call, "null-d_llr")


# ------------------------------------------------------------------------------------------ capi_tbcc
c = "ofdm_tbcc_blocks"
case(c, "fine")
edge(c, "K-low", dict(K=16), dict(K=24))
edge(c, "K-high", dict(K=2056), dict(K=2048))
edge(c, "K-multiple", dict(K=28), dict(K=32))
edge(c, "seg_bits-negative", dict(seg_bits=-1), dict(seg_bits=0))
c = "ofdm_tbcc_rm_blocks"
case(c, "fine")
tbcc_geometry(c, rm=True)
edge(c, "seg_bits-negative", dict(seg_bits=-1), dict(seg_bits=0))
c = "ofdm_tx_tbcc_encode_frames"
tbcc_geometry(c)
enc_edges(c, 72)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_bits=0)
c = "ofdm_tx_tbcc_encode_rm_frames"
tbcc_geometry(c, rm=True)
enc_edges(c, 40)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_bits=0)
c = "ofdm_rx_reserve_tbcc"
case(c, "fine")
case(c, "null-handle", h=None)
tbcc_geometry(c)
edge(c, "n_blocks-negative", dict(n_blocks=-1), dict(n_blocks=0))
edge(c, "n_blocks-range", dict(n_blocks=MAXB + 1), dict(n_blocks=MAXB))
c = "ofdm_tbcc_decode_frames"
tbcc_geometry(c)
dec_edges(c, 72)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_stride=0)
case(c, "null-d_llr-metric-alone-wanted", out={"metric": "BUF"})
c = "ofdm_tbcc_decode_rm_frames"
tbcc_geometry(c, rm=True)
dec_edges(c, 40)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_stride=0)
c = "ofdm_tbcc_rate_dematch_frames"
tbcc_geometry(c, rm=True)
case(c, "null-handle", h=None)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "blocks-negative", dict(blocks_per_seg=-1), dict(blocks_per_seg=0))
edge(c, "blocks-range", dict(n_seg=MAXB + 1), dict(n_seg=MAXB))
edge(c, "seg_stride-short", dict(seg_stride=39), dict(seg_stride=40))
edge(c, "out_stride-short", dict(out_stride=71), dict(out_stride=72))
edge(c, "items-seg_stride", dict(n_seg=2, seg_stride=ITEMS // 2 + 1), dict(n_seg=2, seg_stride=ITEMS // 2))
edge(c, "items-out_stride", dict(n_seg=2, out_stride=ITEMS // 2 + 1), dict(n_seg=2, out_stride=ITEMS // 2))
_lim = MAXB * 256 // (3 * 2048)
edge(c, "grid-range", dict(n_seg=_lim + 1, K=2048, out_stride=6144), dict(n_seg=_lim, K=2048, out_stride=6144))
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_stride=0, out_stride=0)
case(c, "noop-no-segments", n_seg=0, d_llr="BUF", d_out="BUF")
case(c, "noop-no-blocks", blocks_per_seg=0, d_llr="BUF", d_out="BUF")
case(c, "null-d_llr", d_out="BUF")
case(c, "null-d_out", d_llr="BUF")

# ------------------------------------------------------------------------------------------ capi_bitproc
c = "ofdm_crc_bits"
edge(c, "kind-low", dict(kind=-1), dict(kind=0))
edge(c, "kind-high", dict(kind=4), dict(kind=3))
for c, size in (("ofdm_crc_compute", "A"), ("ofdm_crc_compute_long", "n_bits")):
    edge(c, "kind-low", dict(kind=-1), dict(kind=0))
    edge(c, "kind-high", dict(kind=4), dict(kind=3))
    edge(c, size + "-low", {size: 0}, {size: 8})
    edge(c, size + "-multiple", {size: 12}, {size: 16})
    case(c, "null-bits", crc="U32")
    case(c, "null-crc", host_bits="HOST")
    case(c, "fine", host_bits="HOST", crc="U32")
edge("ofdm_crc_compute", "A-high", dict(A=2048, kind=3), dict(A=2040, kind=3))
edge("ofdm_crc_compute", "A-plus-L", dict(A=2032), dict(A=2024))
edge("ofdm_crc_compute_long", "n_bits-high", dict(n_bits=(1 << 30) + 8), dict(n_bits=1 << 30))
c = "ofdm_gold_bits"
edge(c, "first-negative", dict(first=-1), dict(first=0))
edge(c, "n-negative", dict(n=-1), dict(n=0))
edge(c, "first-high", dict(first=GOLD_MAX + 1, n=0), dict(first=GOLD_MAX, n=0))
edge(c, "sum-high", dict(first=1, n=GOLD_MAX), dict(first=0, n=GOLD_MAX))
case(c, "null-host_out")
case(c, "fine", host_out="HOST")
for c in ("ofdm_tx_reserve_bitproc", "ofdm_rx_reserve_bitproc", "ofdm_tx_reserve_turbo_rm", "ofdm_rx_reserve_turbo_rm"):
    case(c, "fine")
    case(c, "null-handle", h=None)
for c, mode_a, mode_b in (("ofdm_tx_crc_attach_frames", "payload_mode", "info_mode"), ("ofdm_crc_check_frames", "info_mode", None)):
    edge(c, "kind-low", dict(kind=-1), dict(kind=0))
    edge(c, "kind-high", dict(kind=4), dict(kind=3))
    edge(c, "A-low", dict(A=0), dict(A=8))
    edge(c, "A-multiple", dict(A=12), dict(A=16))
    edge(c, "A-high", dict(A=2048, kind=3), dict(A=2040, kind=3))
    edge(c, "A-plus-L", dict(A=2032), dict(A=2024))
    edge(c, "n_blocks-negative", dict(n_blocks=-1), dict(n_blocks=0))
    edge(c, "n_blocks-range", dict(n_blocks=MAXB + 1), dict(n_blocks=MAXB))
    edge(c, mode_a + "-low", {mode_a: 0}, {mode_a: P})
    edge(c, mode_a + "-high", {mode_a: 3}, {mode_a: U})
    if mode_b:
        edge(c, mode_b + "-low", {mode_b: 0}, {mode_b: P})
        edge(c, mode_b + "-high", {mode_b: 3}, {mode_b: U})
    edge(c, "mask-above-L", dict(kind=3, mask=0x100), dict(kind=3, mask=0xFF))
    case(c, "mask-unread-with-d_mask", kind=3, mask=0x100, d_mask="BUF")
    case(c, "null-handle", h=None)
    case(c, "null-handle-behind-the-argument-checks", h=None, kind=4)
case("ofdm_tx_crc_attach_frames", "noop-no-blocks", n_blocks=0, d_payload="BUF", d_info="BUF")
case("ofdm_tx_crc_attach_frames", "null-d_payload", d_info="BUF")
case("ofdm_tx_crc_attach_frames", "null-d_info", d_payload="BUF")
c = "ofdm_crc_check_frames"
edge(c, "payload_mode-low", dict(out={"payload": "BUF", "payload_mode": 0}), dict(out={"payload": "BUF", "payload_mode": P}))
edge(c, "payload_mode-high", dict(out={"payload": "BUF", "payload_mode": 3}), dict(out={"payload": "BUF", "payload_mode": U}))
case(c, "payload_mode-unread-without-payload", out={"ok": "BUF", "payload_mode": 3})
case(c, "noop-no-blocks", n_blocks=0, d_info="BUF")
case(c, "noop-null-out", out=None, d_info="BUF")
case(c, "noop-nothing-wanted", out={}, d_info="BUF")
case(c, "null-d_info")
c = "ofdm_tx_scramble_frames"
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "seg_bits-negative", dict(seg_bits=-1), dict(seg_bits=0))
edge(c, "seg_bits-high", dict(seg_bits=GOLD_MAX), dict(seg_bits=GOLD_MAX - 1))
edge(c, "items-product", dict(n_seg=1024, seg_bits=ITEMS // 1024 + 1), dict(n_seg=1024, seg_bits=ITEMS // 1024))
edge(c, "mode-low", dict(mode=0), dict(mode=P))
edge(c, "mode-high", dict(mode=3), dict(mode=U))
edge(c, "packed-whole-bytes", dict(mode=P, seg_bits=12), dict(mode=P, seg_bits=16))
case(c, "null-handle", h=None)
case(c, "null-handle-behind-the-argument-checks", h=None, mode=0)
case(c, "noop-no-segments", n_seg=0, d_in="BUF", d_out="BUF", d_cinit="BUF")
case(c, "noop-no-bits", seg_bits=0, d_in="BUF", d_out="BUF", d_cinit="BUF")
case(c, "null-d_in", d_out="BUF", d_cinit="BUF")
case(c, "null-d_out", d_in="BUF", d_cinit="BUF")
case(c, "null-d_cinit", d_in="BUF", d_out="BUF")
c = "ofdm_descramble_llr_frames"
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "seg_bits-negative", dict(seg_bits=-1), dict(seg_bits=0))
edge(c, "seg_bits-high", dict(seg_bits=GOLD_MAX, seg_stride=GOLD_MAX, out_stride=GOLD_MAX),
     dict(seg_bits=GOLD_MAX - 1, seg_stride=GOLD_MAX, out_stride=GOLD_MAX))
edge(c, "seg_stride-short", dict(seg_stride=15), dict(seg_stride=16))
edge(c, "out_stride-short", dict(out_stride=15), dict(out_stride=16))
edge(c, "items-seg_stride", dict(n_seg=2, seg_stride=ITEMS // 2 + 1), dict(n_seg=2, seg_stride=ITEMS // 2))
edge(c, "items-out_stride", dict(n_seg=2, out_stride=ITEMS // 2 + 1), dict(n_seg=2, out_stride=ITEMS // 2))
edge(c, "in-place-strides", dict(d_llr="BUF", d_out="BUF", out_stride=17), dict(d_llr="BUF", d_out="BUF", out_stride=16))
case(c, "null-handle", h=None)
case(c, "null-handle-behind-the-argument-checks", h=None, n_seg=-1)
case(c, "noop-no-segments", n_seg=0, d_llr="BUF", d_out="BUF", d_cinit="BUF")
case(c, "noop-no-bits", seg_bits=0, d_llr="BUF", d_out="BUF", d_cinit="BUF")
case(c, "null-d_llr", d_out="BUF", d_cinit="BUF")
case(c, "null-d_out", d_llr="BUF", d_cinit="BUF")

# ------------------------------------------------------------------------------------------ capi_turbo
c = "ofdm_turbo_blocks"
case(c, "fine")
turbo_geometry(c)
edge(c, "seg_bits-negative", dict(seg_bits=-1), dict(seg_bits=0))
c = "ofdm_turbo_qpp_check"
case(c, "fine")
turbo_geometry(c)
qpp_edges(c)
c = "ofdm_tx_turbo_encode_frames"
turbo_geometry(c)
qpp_edges(c)
enc_edges(c, 132)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_bits=0)
for c in ("ofdm_rx_reserve_turbo", "ofdm_rx_reserve_turbo_es"):
    case(c, "fine")
    case(c, "null-handle", h=None)
    turbo_geometry(c)
    edge(c, "n_blocks-negative", dict(n_blocks=-1), dict(n_blocks=0))
    case(c, "n_blocks-range-refused", n_blocks=MAXB + 1)
c = "ofdm_turbo_decode_frames"
turbo_geometry(c)
qpp_edges(c)
edge(c, "n_iter-low", dict(n_iter=0), dict(n_iter=1))
edge(c, "n_iter-high", dict(n_iter=17), dict(n_iter=16))
dec_edges(c, 132)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_stride=0)
case(c, "n_iter-in-front-of-seg_stride", n_iter=0, seg_stride=0)
c = "ofdm_turbo_decode_es_frames"
turbo_geometry(c)
qpp_edges(c)
edge(c, "crc_kind-low", dict(crc_kind=-1), dict(crc_kind=0))
edge(c, "crc_kind-high", dict(crc_kind=4), dict(crc_kind=3))
edge(c, "min_iter-low", dict(min_iter=0), dict(min_iter=1))
edge(c, "max_iter-high", dict(max_iter=17), dict(max_iter=16))
edge(c, "min-above-max", dict(min_iter=3, max_iter=2), dict(min_iter=2, max_iter=2))
dec_edges(c, 132)
edge(c, "stat_stride-short", dict(blocks_per_seg=2, seg_stride=264, out=dict(WANT_BITS, stat_stride=1)),
     dict(blocks_per_seg=2, seg_stride=264, out=dict(WANT_BITS, stat_stride=2)))
edge(c, "stat_stride-items", dict(n_seg=2, out=dict(WANT_BITS, stat_stride=ITEMS // 2 + 1)), dict(n_seg=2, out=dict(WANT_BITS, stat_stride=ITEMS // 2)))
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_stride=0)
case(c, "null-d_llr-iters-alone-wanted", out={"iters": "BUF"})
case(c, "bits_mode-in-front-of-stat_stride", blocks_per_seg=2, seg_stride=264, out={"bits": "BUF", "bits_mode": 0, "stat_stride": 1})
c = "ofdm_turbo_rm_blocks"
case(c, "fine")
turbo_geometry(c)
edge(c, "E-low", dict(E=0), dict(E=1))
edge(c, "E-high", dict(E=16 * 132 + 1), dict(E=16 * 132))
edge(c, "seg_bits-negative", dict(seg_bits=-1), dict(seg_bits=0))


def rm_edges(call, sized):
    """Ncb, E and rv of the rate-matching calls at K = 40: Kpi = 64, Navail = 132 at Ncb = 0 (3 Kpi) and 44 at Ncb = Kpi"""
    roomy = {k: 16 * 132 for k in sized}
    edge(call, "Ncb-low", dict(Ncb=63), dict(Ncb=64))
    edge(call, "Ncb-high", dict(Ncb=193), dict(Ncb=192))
    edge(call, "rv-low", dict(rv=-1), dict(rv=0))
    edge(call, "rv-high", dict(rv=4), dict(rv=3))
    if "d_rv" in CALLS[call]:
        case(call, "rv-unread-with-d_rv", rv=7, d_rv="BUF")
    if "E" in CALLS[call]:
        edge(call, "E-low", dict(E=0), dict(E=1))
        edge(call, "E-high", dict(E=16 * 132 + 1, **roomy), dict(E=16 * 132, **roomy))
        edge(call, "E-high-at-Ncb-Kpi", dict(E=16 * 44 + 1, Ncb=64, **roomy), dict(E=16 * 44, Ncb=64, **roomy))


c = "ofdm_turbo_rm_info"
case(c, "fine-no-outputs")
case(c, "fine", k0="I32", n_avail="I32")
turbo_geometry(c)
rm_edges(c, ())
c = "ofdm_tx_turbo_encode_rm_frames"
turbo_geometry(c)
qpp_edges(c)
rm_edges(c, ("seg_bits",))
enc_edges(c, 100)
case(c, "asymmetric-n_seg-2^31-no-blocks", n_seg=1 << 31, blocks_per_seg=0, seg_bits=0)
c = "ofdm_turbo_rate_dematch_frames"
turbo_geometry(c)
rm_edges(c, ("seg_stride",))
case(c, "null-handle", h=None)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "blocks-negative", dict(blocks_per_seg=-1), dict(blocks_per_seg=0))
edge(c, "seg_stride-short", dict(seg_stride=99), dict(seg_stride=100))
edge(c, "out_stride-short", dict(out_stride=131), dict(out_stride=132))
edge(c, "items-seg_stride", dict(n_seg=2, seg_stride=ITEMS // 2 + 1), dict(n_seg=2, seg_stride=ITEMS // 2))
edge(c, "items-out_stride", dict(n_seg=2, out_stride=ITEMS // 2 + 1), dict(n_seg=2, out_stride=ITEMS // 2))
_per = 3 * 6144 + 12
_lim = MAXB * 256 // _per
edge(c, "grid-range", dict(n_seg=_lim + 1, K=6144, out_stride=_per), dict(n_seg=_lim, K=6144, out_stride=_per))
_lim2 = MAXB * 256 // _per // 2
edge(c, "grid-range-two-blocks", dict(n_seg=_lim2 + 1, K=6144, blocks_per_seg=2, seg_stride=200, out_stride=2 * _per),
     dict(n_seg=_lim2, K=6144, blocks_per_seg=2, seg_stride=200, out_stride=2 * _per))
edge(c, "asymmetric-n_seg-2^31-no-blocks", dict(n_seg=1 << 31, blocks_per_seg=0, seg_stride=0, out_stride=0),
     dict(n_seg=MAXB, blocks_per_seg=0, seg_stride=0, out_stride=0))
case(c, "noop-no-segments", n_seg=0, d_llr="BUF", d_out="BUF")
case(c, "noop-no-blocks", blocks_per_seg=0, d_llr="BUF", d_out="BUF")
case(c, "null-d_llr", d_out="BUF")
case(c, "null-d_out", d_llr="BUF")

# ------------------------------------------------------------------------------------------ capi_tb
c = "ofdm_turbo_k_next"
edge(c, "bits-high", dict(bits=6145), dict(bits=6144))
case(c, "bits-zero", bits=0)
case(c, "bits-41", bits=41)


def plan_edges(call, with_g=True):
    """the segmentation and rate-matching arithmetic (tb_plan), through a call that reports it"""
    edge(call, "Z-not-a-block-size", dict(Z=44), dict(Z=48))
    edge(call, "A-low", dict(A=0), dict(A=8))
    edge(call, "A-multiple", dict(A=12), dict(A=16))
    edge(call, "A-high", dict(A=(1 << 20) - 16), dict(A=(1 << 20) - 24))
    edge(call, "block-below-40", dict(A=32, Z=40), dict(A=24, Z=40))
    if with_g:
        edge(call, "G-negative", dict(G=-2, q=1), dict(G=1, q=1))
        edge(call, "G-high", dict(G=1 << 31, q=1), dict(G=MAXB, q=1))
        edge(call, "q-low", dict(q=0), dict(q=1))
        edge(call, "q-divides-G", dict(G=201), dict(G=202))
        edge(call, "E-high", dict(G=16 * 204 + 2), dict(G=16 * 204))


c = "ofdm_tb_geometry"
case(c, "fine")
case(c, "fine-segmentation-only", G=0, q=0)
case(c, "null-out", geom=None)
plan_edges(c)
edge(c, "N_IR-negative", dict(N_IR=-1), dict(N_IR=0))
edge(c, "N_IR-below-Kpi", dict(N_IR=95), dict(N_IR=96))
c = "ofdm_tx_reserve_tb"
case(c, "fine")
case(c, "null-handle", h=None)
case(c, "G-zero-refused", G=0)
plan_edges(c)
edge(c, "n_tb-negative", dict(n_tb=-1), dict(n_tb=0))
case(c, "n_tb-range-refused", n_tb=MAXB + 1)
case(c, "n_tb-items-refused", n_tb=TB_ITEMS // 204 + 1)
for c in ("ofdm_rx_reserve_tb", "ofdm_rx_reserve_tb_es"):
    case(c, "fine")
    case(c, "null-handle", h=None)
    plan_edges(c, with_g=False)
    edge(c, "n_tb-negative", dict(n_tb=-1), dict(n_tb=0))
    case(c, "n_tb-range-refused", n_tb=MAXB + 1)
    case(c, "n_tb-items-refused", n_tb=TB_ITEMS // 204 + 1)


def tb_call_edges(call, row):
    """what ofdm_tx_tb_encode_frames and the two decodes check in common (tb_bad_call); row = the call's own row length"""
    case(call, "null-handle", h=None)
    case(call, "G-zero-refused", G=0)
    plan_edges(call)
    edge(call, "N_IR-negative", dict(N_IR=-1), dict(N_IR=0))
    edge(call, "N_IR-below-Kpi", dict(N_IR=95), dict(N_IR=96))
    edge(call, "n_tb-negative", dict(n_tb=-1), dict(n_tb=0))
    two = dict(A=48, Z=64, G=400)                            # K- = 56 and K+ = 64, one block each
    edge(call, "minus-no-permutation", dict(two, f1_minus=2, f2_minus=42, **{row: 400}), dict(two, f1_minus=19, f2_minus=42, **{row: 400}))
    case(call, "minus-unread-without-minus-blocks", f1_minus=-5, f2_minus=-5)
    edge(call, "plus-no-permutation", dict(f1_plus=2), dict(f1_plus=7))
    edge(call, "rv-low", dict(rv=-1), dict(rv=0))
    edge(call, "rv-high", dict(rv=4), dict(rv=3))
    case(call, "rv-unread-with-d_rv", rv=7, d_rv="BUF")
    case(call, "n_tb-range-refused", n_tb=MAXB + 1)         # the last count in range fails the row bound with the same text
    edge(call, "row-items", dict(**{row: TB_ITEMS + 1}), dict(**{row: TB_ITEMS}))
    edge(call, "row-items-product", dict(n_tb=2, **{row: TB_ITEMS // 2 + 1}), dict(n_tb=2, **{row: TB_ITEMS // 2}))


c = "ofdm_tx_tb_encode_frames"
tb_call_edges(c, "cw_bits")
edge(c, "payload_mode-low", dict(payload_mode=0), dict(payload_mode=P))
edge(c, "payload_mode-high", dict(payload_mode=3), dict(payload_mode=U))
edge(c, "cw_mode-low", dict(cw_mode=0), dict(cw_mode=P))
edge(c, "cw_mode-high", dict(cw_mode=3), dict(cw_mode=U))
edge(c, "cw_bits-short", dict(cw_bits=199), dict(cw_bits=200))
edge(c, "packed-whole-bytes", dict(cw_mode=P, cw_bits=204), dict(cw_mode=P, cw_bits=208))
case(c, "noop-no-blocks", n_tb=0, d_payload="BUF", d_cw="BUF")
case(c, "null-d_payload", d_cw="BUF")
case(c, "null-d_cw", d_payload="BUF")
for c in ("ofdm_tb_decode_frames", "ofdm_tb_decode_es_frames"):
    tb_call_edges(c, "llr_stride")
    if c == "ofdm_tb_decode_frames":
        edge(c, "n_iter-low", dict(n_iter=0), dict(n_iter=1))
        edge(c, "n_iter-high", dict(n_iter=17), dict(n_iter=16))
    else:
        edge(c, "min_iter-low", dict(min_iter=0), dict(min_iter=1))
        edge(c, "max_iter-high", dict(max_iter=17), dict(max_iter=16))
        edge(c, "min-above-max", dict(min_iter=3, max_iter=2), dict(min_iter=2, max_iter=2))
    edge(c, "llr_stride-short", dict(llr_stride=199), dict(llr_stride=200))
    edge(c, "soft_stride-short", dict(soft_stride=203), dict(soft_stride=204))
    edge(c, "soft_stride-items", dict(soft_stride=TB_ITEMS + 1), dict(soft_stride=TB_ITEMS))
    case(c, "null-out", out=None)
    edge(c, "payload_mode-low", dict(out={"payload": "BUF", "payload_mode": 0}), dict(out={"payload": "BUF", "payload_mode": P}))
    edge(c, "payload_mode-high", dict(out={"payload": "BUF", "payload_mode": 3}), dict(out={"payload": "BUF", "payload_mode": U}))
    case(c, "payload_mode-unread-without-payload", out={"payload_mode": 3})
    case(c, "noop-no-blocks", n_tb=0, d_llr="BUF", d_soft="BUF")
    case(c, "null-d_llr", d_soft="BUF")
    case(c, "null-d_soft", d_llr="BUF")

IDS = [i for i, _, _ in CASES]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)


class Runner:
    """makes the table's calls on one transmitter and one receiver handle of library `om` (ofdm_mi355x, loaded)"""
    calls, out_types = CALLS, OUT_TYPES                      # the table: tests/despread_refusal_cases.py runs its own

    def __init__(self, om):
        from ofdm_mi355x import _lib
        self.lib, self._lib = om.load(), _lib
        self.tx = om.TxEngine(64, 16, 62, 60)
        self.rx = om.RxEngine(8, 64, 16, 62, (1, 3), 60, 100)
        self.buf = om.DeviceBuffer(256)
        self.host = (C.c_uint8 * 16)()
        self.keep = []

    def value(self, call, name, v):
        if name == "h":
            return {"TX": self.tx._h, "RX": self.rx._h, None: None}[v]
        if name == "out":
            if v is None:
                return None
            s = getattr(self._lib, self.out_types[call])()
            for k, x in v.items():
                setattr(s, k, self.buf.data_ptr() if x == "BUF" else x)
            self.keep.append(s)
            return C.byref(s)
        if v == "BUF":
            return self.buf.data_ptr()
        if v == "HOST":
            return C.cast(self.host, C.c_void_p)
        if v in ("U32", "I32", "GEOM"):
            s = {"U32": C.c_uint32, "I32": C.c_int32, "GEOM": self._lib.TbGeom}[v]()
            self.keep.append(s)
            return C.byref(s)
        return v

    def run(self, call, kwargs):
        args = [self.value(call, n, kwargs[n]) for n in self.calls[call]]
        status = int(getattr(self.lib, call)(*args))
        self.keep.clear()
        return [status, self.lib.ofdm_last_error().decode() if status < 0 else ""]
