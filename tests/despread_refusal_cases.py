"""The refused and no-op calls of the DFT-spread side of the C ABI -- every public call of csrc/capi_dft.hip, capi_dft_tx.hip and
capi_despread.hip, and the three of capi_mrc.hip whose argument checks they share -- as one table, shared by
tests/test_gpu_despread_refusals.py and the recorder tests/golden/gen_despread_refusals.py.  The rules are those of
tests/codec_refusal_cases.py, and so is the Runner: no case launches a kernel or grows a workspace; a call whose arguments are all
fine is given null buffers (its last refusal), nothing to do (no segments, no frames) or, for a reserve call, a batch of 0 (which
may build the plan of its M); each refusal text appears at the first argument value that triggers it and -- in the case behind
it -- at the last value that does not.  Where that last value would allocate, launch or replace the allocation set, only the
refused side is listed.

The order in which a call refuses depends on the allocation set of its handle, so every case of a call that takes a handle runs
in three STATES of both handles: no set, a set with a gap, two sizes and two modulations, and a set with an allocation whose
M * bits per symbol is no whole number of bytes.  The two ofdm_*_set_allocations calls, which make the states, run in the first.
A name says what a case does in the state it is written for; the other states record what they give.  Where a call refuses a
missing set in front of everything a block of cases is about, WITH_A_SET keeps that block out of the first state: the cases in
front of the block show where the refusal stands."""
import ctypes as C

import codec_refusal_cases as codec

P, U = 1, 2                                  # OFDM_BITS_PACKED, OFDM_BITS_UNPACKED
RHO, GIVEN, SEG = 0, 1, 2                    # OFDM_DESPREAD_NOISE_*
M_GIVEN, M_SEG, M_EST = 0, 1, 2              # OFDM_MRC_NOISE_*
N31, LEN, ROW = 1 << 31, 1 << 40, 1 << 30    # segments (units), symbols per segment and n_seg * stride, entries per row
GROUPS = (1 << 31) - 1                       # workgroups of one launch
DEMOD_MAX = ((1 << 31) - 1) // 8             # frames and data symbols of ofdm_rx_demod_frames
NAN, INF = float("nan"), float("inf")
# the handles of the Runner: nfft 64, cp 16, 60 data bins (rows_per_group 16), QPSK, [1, 3]: a frame of 4 symbols is 320 samples
KD, FRAME = 60, 320

# state -> [(start, M, bits per symbol)]; the transmitter's set is the same without the modulations
STATES = {"none": [], "set": [(0, 4, 2), (6, 6, 4)], "odd": [(0, 6, 2)]}

_STAGE = ["d_csi", "csi_stride", "rho"]
_DS_TAIL = ["noise_mode", "noise_var", "d_sigma2", "bits_mode", "out", "stream"]
_MRC_TAIL = ["noise_mode", "h_noise_var", "d_sigma2", "bits_mode", "out", "stream"]
_FRAMES = ["n_frames", "frame_stride", "frame_len", "d_eq", "d_tsr"]
CALLS = {
    "ofdm_dft_size_ok": ["M"],
    "ofdm_dft_plan_info": ["M", "n_pass", "radix8", "rows_per_group"],
    "ofdm_alloc_layout": ["n_alloc", "M", "mod", "n_seg", "rows", "bits_mode", "sym_off", "llr_off", "bits_off", "totals"],
    "ofdm_rx_set_allocations": ["h", "n_alloc", "h_start", "h_M", "h_mod"],
    "ofdm_tx_set_allocations": ["h", "n_alloc", "h_start", "h_M"],
    "ofdm_tx_reserve_spread": ["h", "M", "n_rows"],
    "ofdm_tx_dft_spread": ["h", "d_sym", "n_rows", "M", "d_out", "stream"],
    "ofdm_tx_modulate_frames_spread": ["h", "d_bits", "bits_mode", "n_frames", "n_sym", "d_iq", "frame_stride", "stream"],
    "ofdm_tx_reserve_spread_alloc": ["h", "n_rows"],
    "ofdm_tx_dft_spread_alloc": ["h", "d_sym", "n_rows", "row_len", "d_out", "stream"],
    "ofdm_tx_modulate_frames_alloc": ["h", "d_bits", "bits_mode", "n_frames", "n_sym", "d_iq", "frame_stride", "stream"],
    "ofdm_rx_reserve_despread": ["h", "M", "n_seg"],
    "ofdm_dft_despread_frames": ["h", "d_sym", "n_seg", "rows", "M", "seg_stride"] + _STAGE + ["modulation"] + _DS_TAIL,
    "ofdm_rx_demod_frames_despread": ["h", "d_iq"] + _FRAMES + _DS_TAIL,
    "ofdm_rx_reserve_mrc_despread": ["h", "M", "n_branch", "n_seg"],
    "ofdm_combine_despread_frames": ["h", "d_sym", "n_branch", "n_seg", "rows", "M", "seg_stride"] + _STAGE + ["modulation"] + _MRC_TAIL,
    "ofdm_rx_demod_frames_mrc_despread": ["h", "d_iq", "n_branch"] + _FRAMES + _MRC_TAIL,
    "ofdm_rx_reserve_despread_alloc": ["h", "n_seg"],
    "ofdm_dft_despread_alloc_frames": ["h", "d_sym", "n_seg", "rows", "row_len", "seg_stride"] + _STAGE + _DS_TAIL,
    "ofdm_rx_demod_frames_despread_alloc": ["h", "d_iq"] + _FRAMES + _DS_TAIL,
    "ofdm_rx_reserve_mrc_despread_alloc": ["h", "n_branch", "n_seg", "row_len"],
    "ofdm_combine_despread_alloc_frames": ["h", "d_sym", "n_branch", "n_seg", "rows", "row_len", "seg_stride"] + _STAGE + _MRC_TAIL,
    "ofdm_rx_demod_frames_mrc_despread_alloc": ["h", "d_iq", "n_branch"] + _FRAMES + _MRC_TAIL,
    "ofdm_rx_reserve_mrc": ["h", "n_branch", "n_seg", "rows", "row_len"],
    "ofdm_combine_csi_frames": ["h", "d_sym", "n_branch", "n_seg", "rows", "row_len", "seg_stride"] + _STAGE +
                               ["modulation", "noise_mode", "h_noise_var", "d_sigma2", "out", "stream"],
    "ofdm_rx_demod_frames_mrc": ["h", "d_iq", "n_branch"] + _FRAMES + ["noise_mode", "h_noise_var", "out", "d_sigma2_out", "stream"],
}
SETTERS = ("ofdm_rx_set_allocations", "ofdm_tx_set_allocations")
OUT_TYPES = {c: "MrcDespreadOut" if "h_noise_var" in a else "DespreadOut" for c, a in CALLS.items() if "out" in a}
OUT_TYPES.update(ofdm_combine_csi_frames="MrcOut", ofdm_rx_demod_frames_mrc="MrcOut")

LLR = {"llr": "BUF"}
_SEGS = dict(h="RX", d_sym=None, n_seg=1, rows=1, seg_stride=12, rho=0.0, d_sigma2=None, stream=None)
_DS = dict(_SEGS, d_csi=None, csi_stride=0, noise_mode=RHO, noise_var=0.0, bits_mode=0, out=LLR)
_MRC = dict(_SEGS, n_branch=2, d_csi=None, csi_stride=12, noise_mode=M_GIVEN, h_noise_var=[1.0, 1.0], bits_mode=0, out=LLR)
_COMP = dict(h="RX", d_iq="BUF", n_frames=0, frame_stride=FRAME, frame_len=FRAME, d_eq="BUF", d_tsr=None, stream=None)
_DS_COMP = dict(_COMP, noise_mode=RHO, noise_var=0.0, d_sigma2=None, bits_mode=0, out=LLR)
_MRC_COMP = dict(_COMP, n_branch=2, noise_mode=M_GIVEN, h_noise_var=[1.0, 1.0], d_sigma2=None, bits_mode=0, out=LLR)
_TX_COMP = dict(h="TX", d_bits=None, bits_mode=U, n_frames=1, n_sym=4, d_iq=None, frame_stride=FRAME, stream=None)
# a call every check of which passes, up to its last refusal (null buffers) -- or, for the calls without one, a plain success
BASE = {
    "ofdm_dft_size_ok": dict(M=12),
    "ofdm_dft_plan_info": dict(M=12, n_pass=None, radix8=None, rows_per_group=None),
    "ofdm_alloc_layout": dict(n_alloc=1, M=[4], mod=[2], n_seg=1, rows=1, bits_mode=0, sym_off=None, llr_off=None, bits_off=None,
                              totals=None),
    "ofdm_rx_set_allocations": dict(h="RX", n_alloc=0, h_start=None, h_M=None, h_mod=None),
    "ofdm_tx_set_allocations": dict(h="TX", n_alloc=0, h_start=None, h_M=None),
    "ofdm_tx_reserve_spread": dict(h="TX", M=12, n_rows=0),
    "ofdm_tx_dft_spread": dict(h="TX", d_sym=None, n_rows=1, M=12, d_out=None, stream=None),
    "ofdm_tx_modulate_frames_spread": _TX_COMP,
    "ofdm_tx_reserve_spread_alloc": dict(h="TX", n_rows=0),
    "ofdm_tx_dft_spread_alloc": dict(h="TX", d_sym=None, n_rows=1, row_len=12, d_out=None, stream=None),
    "ofdm_tx_modulate_frames_alloc": _TX_COMP,
    "ofdm_rx_reserve_despread": dict(h="RX", M=12, n_seg=0),
    "ofdm_dft_despread_frames": dict(_DS, M=12, modulation=2),
    "ofdm_rx_demod_frames_despread": _DS_COMP,
    "ofdm_rx_reserve_mrc_despread": dict(h="RX", M=12, n_branch=2, n_seg=0),
    "ofdm_combine_despread_frames": dict(_MRC, M=12, modulation=2),
    "ofdm_rx_demod_frames_mrc_despread": _MRC_COMP,
    "ofdm_rx_reserve_despread_alloc": dict(h="RX", n_seg=0),
    "ofdm_dft_despread_alloc_frames": dict(_DS, row_len=12),
    "ofdm_rx_demod_frames_despread_alloc": _DS_COMP,
    "ofdm_rx_reserve_mrc_despread_alloc": dict(h="RX", n_branch=2, n_seg=0, row_len=12),
    "ofdm_combine_despread_alloc_frames": dict(_MRC, row_len=12, d_csi="BUF"),
    "ofdm_rx_demod_frames_mrc_despread_alloc": _MRC_COMP,
    "ofdm_rx_reserve_mrc": dict(h="RX", n_branch=2, n_seg=0, rows=0, row_len=0),
    "ofdm_combine_csi_frames": {k: v for k, v in dict(_MRC, row_len=12, modulation=2).items() if k != "bits_mode"},
    "ofdm_rx_demod_frames_mrc": dict(_COMP, n_branch=2, noise_mode=M_GIVEN, h_noise_var=[1.0, 1.0], out=LLR, d_sigma2_out=None),
}

CASES = []                                   # (id, call, keyword arguments, states)
EVERY, WITH_A_SET = tuple(STATES), ("set", "odd")
states = EVERY                               # of the cases that follow


def case(call, name, **over):
    unknown = set(over) - set(CALLS[call])
    assert not unknown, (call, unknown)
    CASES.append(("%s/%s" % (call[5:], name), call, dict(BASE[call], **over),
                  states if "h" in CALLS[call] and call not in SETTERS else ("none",)))


def edge(call, name, bad, good=None):
    """the first value(s) a refusal triggers at, and the last that it does not"""
    case(call, name + "-refused", **bad)
    if good is not None:
        case(call, name + "-passes", **good)


def size_edges(call, **room):
    """M must be 2^a 3^b 5^c in 1 .. 4096; room: what has to grow with M"""
    edge(call, "M-low", dict(M=0), dict(M=1))
    edge(call, "M-high", dict(M=4097), dict(M=4096, **{k: 4096 for k in room}))
    edge(call, "M-factor-7", dict(M=7), dict(M=8))


def branch_edges(call, nv="h_noise_var"):
    wide = {nv: [1.0] * 8} if nv in CALLS[call] else {}
    edge(call, "n_branch-low", dict(n_branch=0), dict(n_branch=1))
    edge(call, "n_branch-high", dict(n_branch=9, **wide), dict(n_branch=8, **wide))


def want_edges(call, bits=True):
    """the out struct and, where the stage makes hard bits, their mode"""
    case(call, "out-null-refused", out=None)
    case(call, "out-empty-refused", out={})
    case(call, "out-weight-alone-passes", out={"weight": "BUF"})
    if OUT_TYPES[call] == "MrcDespreadOut":
        case(call, "out-comb-alone-passes", out={"comb": "BUF"})
    if bits:
        edge(call, "bits_mode-low", dict(out={"bits": "BUF"}, bits_mode=0), dict(out={"bits": "BUF"}, bits_mode=P))
        edge(call, "bits_mode-high", dict(out={"bits": "BUF"}, bits_mode=3), dict(out={"bits": "BUF"}, bits_mode=U))
        case(call, "bits_mode-unread-without-bits", bits_mode=3)


def ds_noise_edges(call, csi):
    """noise_mode, noise_var, d_sigma2 of the despreading stages; csi: what gives the stage its |H|^2 rows (composites: {})"""
    edge(call, "noise_mode-low", dict(noise_mode=-1, **csi), dict(noise_mode=RHO, **csi))
    edge(call, "noise_mode-high", dict(noise_mode=3, d_sigma2="BUF", **csi), dict(noise_mode=SEG, d_sigma2="BUF", **csi))
    edge(call, "noise_var-zero", dict(noise_mode=GIVEN, noise_var=0.0, **csi), dict(noise_mode=GIVEN, noise_var=5e-324, **csi))
    case(call, "noise_var-inf-refused", noise_mode=GIVEN, noise_var=INF, **csi)
    case(call, "noise_var-nan-refused", noise_mode=GIVEN, noise_var=NAN, **csi)
    case(call, "noise_var-unread-passes", noise_mode=RHO, noise_var=NAN, **csi)
    case(call, "seg-null-d_sigma2-refused", noise_mode=SEG, **csi)


def rho_edges(call, csi):
    edge(call, "rho-negative", dict(rho=-1e-30, **csi), dict(rho=0.0, **csi))
    case(call, "rho-inf-refused", rho=INF, **csi)
    case(call, "rho-nan-refused", rho=NAN, **csi)


def mrc_noise_edges(call, est="refused"):
    """noise_mode, h_noise_var, d_sigma2 of the combiners"""
    case(call, "noise_mode-est-" + est, noise_mode=M_EST)
    edge(call, "noise_mode-low", dict(noise_mode=-1), dict(noise_mode=M_GIVEN))
    if "d_sigma2" in CALLS[call]:
        edge(call, "noise_mode-high", dict(noise_mode=3, d_sigma2="BUF"), dict(noise_mode=M_SEG, d_sigma2="BUF"))
        case(call, "seg-null-d_sigma2-refused", noise_mode=M_SEG)
    else:
        case(call, "noise_mode-high-refused", noise_mode=3)
        case(call, "noise_mode-seg-refused", noise_mode=M_SEG)
    case(call, "given-null-h_noise_var-refused", h_noise_var=None)
    edge(call, "noise_var-zero", dict(h_noise_var=[1.0, 0.0]), dict(h_noise_var=[1.0, 5e-324]))
    case(call, "noise_var-inf-refused", h_noise_var=[INF, 1.0])
    case(call, "noise_var-nan-refused", h_noise_var=[1.0, NAN])
    case(call, "noise_var-behind-n_branch-unread-passes", n_branch=1, h_noise_var=[1.0, 0.0])


def mrc_arg_edges(call):
    """what mrc_bad_args decides for a stage call"""
    edge(call, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
    edge(call, "rows-negative", dict(rows=-1), dict(rows=0))
    branch_edges(call)
    big = LEN // 12
    edge(call, "rows-range", dict(rows=big + 1, seg_stride=LEN), dict(rows=big, seg_stride=big * 12, n_branch=1))
    edge(call, "seg_stride-short", dict(seg_stride=11), dict(seg_stride=12))
    edge(call, "csi_stride-short", dict(csi_stride=11), dict(csi_stride=12))
    mrc_noise_edges(call)
    rho_edges(call, {})
    edge(call, "units-range", dict(n_seg=N31 // 2 + 1), dict(n_seg=N31 // 2))
    edge(call, "units-seg_stride", dict(seg_stride=LEN // 2 + 1), dict(seg_stride=LEN // 2))
    edge(call, "units-csi_stride", dict(csi_stride=LEN // 2 + 1), dict(csi_stride=LEN // 2))
    case(call, "noop-no-segments", n_seg=0, d_sym="BUF", d_csi="BUF")
    case(call, "noop-no-rows", rows=0, d_sym="BUF", d_csi="BUF")
    case(call, "null-d_sym", d_csi="BUF")
    case(call, "null-d_csi", d_sym="BUF", d_csi=None)


def open_edges(call):
    """the opening of the calls that run stages behind ofdm_rx_demod_frames, and the batch that call takes"""
    case(call, "fine-no-frames")
    case(call, "null-handle", h=None)
    case(call, "null-d_iq-refused", d_iq=None)
    edge(call, "n_frames-negative", dict(n_frames=-1), dict(n_frames=0))
    case(call, "frame_len-negative-refused", frame_len=-1)
    edge(call, "frame_stride-short", dict(frame_stride=FRAME - 1), dict(frame_stride=FRAME))
    case(call, "null-d_eq-refused", d_eq=None)
    case(call, "null-d_eq-behind-d_iq-refused", d_eq=None, d_iq=None)
    pat = DEMOD_MAX // 3 + 1                                # sync/data patterns of a frame with more than DEMOD_MAX data symbols
    edge(call, "data-symbols-range", dict(frame_len=pat * FRAME, frame_stride=pat * FRAME),
         dict(frame_len=(pat - 1) * FRAME, frame_stride=(pat - 1) * FRAME))
    case(call, "short-frame-no-data-symbols-passes", frame_len=FRAME - 1, frame_stride=FRAME - 1)


def tx_composite_edges(call):
    case(call, "null-handle", h=None)
    edge(call, "n_frames-negative", dict(n_frames=-1), dict(n_frames=0))
    edge(call, "n_sym-negative", dict(n_sym=-4, frame_stride=-FRAME), dict(n_sym=0, frame_stride=0))
    edge(call, "bits_mode-low", dict(bits_mode=0), dict(bits_mode=P))
    edge(call, "bits_mode-high", dict(bits_mode=3), dict(bits_mode=U))
    edge(call, "n_sym-multiple", dict(n_sym=5, frame_stride=400), dict(n_sym=8, frame_stride=2 * FRAME))
    edge(call, "frame_stride-above", dict(frame_stride=FRAME + 1), dict(frame_stride=FRAME))
    case(call, "frame_stride-below-refused", frame_stride=FRAME - 1)
    edge(call, "batch-range", dict(n_frames=1 << 29), dict(n_frames=(1 << 29) - 1))
    case(call, "null-d_bits", d_iq="BUF")
    case(call, "null-d_iq", d_bits="BUF")
    case(call, "bits_mode-in-front-of-n_sym-refused", bits_mode=0, n_sym=5)


# ------------------------------------------------------------------------------------------ no handle
c = "ofdm_dft_size_ok"
for m in (0, 1, 7, 12, 4050, 4096, 4097):
    case(c, "M-%d" % m, M=m)
c = "ofdm_dft_plan_info"
case(c, "fine-no-outputs")
case(c, "fine", n_pass="I32", radix8="I32", rows_per_group="I32")
size_edges(c)
c = "ofdm_alloc_layout"
case(c, "fine")
case(c, "fine-outputs", sym_off=[0, 0], llr_off=[0, 0], bits_off=[0, 0], totals=[0] * 6)
edge(c, "n_alloc-low", dict(n_alloc=0), dict(n_alloc=1))
edge(c, "n_alloc-high", dict(n_alloc=33, M=[4] * 33, mod=[2] * 33), dict(n_alloc=32, M=[4] * 32, mod=[2] * 32))
case(c, "null-M-refused", M=None)
case(c, "null-mod-refused", mod=None)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "rows-negative", dict(rows=-1), dict(rows=0))
edge(c, "bits_mode-low", dict(bits_mode=-1), dict(bits_mode=0))
edge(c, "bits_mode-high", dict(bits_mode=3), dict(bits_mode=U))
edge(c, "n_seg-range", dict(n_seg=N31 + 1, rows=0), dict(n_seg=N31, rows=0))
edge(c, "rows-range", dict(rows=LEN + 1), dict(rows=LEN))
edge(c, "product-range", dict(n_seg=N31, rows=513), dict(n_seg=N31, rows=512))
edge(c, "M-factor-7", dict(M=[7]), dict(M=[8]))
edge(c, "modulation-bpsk", dict(mod=[1]), dict(mod=[2]))
edge(c, "packed-whole-bytes", dict(M=[6], bits_mode=P), dict(M=[4], bits_mode=P))
case(c, "packed-second-allocation-refused", n_alloc=2, M=[4, 6], mod=[2, 2], bits_mode=P)
for c in SETTERS:
    mod = c == "ofdm_rx_set_allocations"

    def lists(start, M, m=2, mod=mod):
        return dict(n_alloc=len(M), h_start=start, h_M=M, **({"h_mod": [m] * len(M)} if mod else {}))

    case(c, "clear-without-a-set")
    case(c, "null-handle", h=None)
    case(c, "n_alloc-negative-refused", n_alloc=-1)
    case(c, "n_alloc-high-refused", n_alloc=33)
    case(c, "null-start-refused", **dict(lists([0], [4]), h_start=None))
    case(c, "null-M-refused", **dict(lists([0], [4]), h_M=None))
    case(c, "start-negative-refused", **lists([-1], [4]))
    case(c, "M-factor-7-refused", **lists([0], [7]))
    case(c, "end-beyond-4096-refused", **lists([4089], [8]))
    case(c, "overlap-refused", **lists([0, 3], [4, 4]))
    case(c, "overlap-inside-refused", **lists([0, 2], [12, 4]))
    if mod:
        case(c, "null-mod-refused", **dict(lists([0], [4]), h_mod=None))
        case(c, "modulation-bpsk-refused", **lists([0], [4], 1))
        case(c, "modulation-3-refused", **lists([0], [4], 3))

# ------------------------------------------------------------------------------------------ transmitter
c = "ofdm_tx_reserve_spread"
case(c, "fine")
case(c, "null-handle", h=None)
size_edges(c)
edge(c, "n_rows-negative", dict(n_rows=-1), dict(n_rows=0))
case(c, "n_rows-range-refused", n_rows=1 << 31)
c = "ofdm_tx_dft_spread"
case(c, "null-handle", h=None)
size_edges(c)
edge(c, "n_rows-negative", dict(n_rows=-1), dict(n_rows=0))
edge(c, "index-range", dict(n_rows=LEN // 12 + 1), dict(n_rows=LEN // 12))
edge(c, "workgroups", dict(M=1, n_rows=GROUPS * 256 + 1), dict(M=1, n_rows=GROUPS * 256))
case(c, "noop-no-rows", n_rows=0, d_sym="BUF", d_out="BUF")
case(c, "null-d_sym", d_out="BUF")
case(c, "null-d_out", d_sym="BUF")
c = "ofdm_tx_modulate_frames_spread"
tx_composite_edges(c)
c = "ofdm_tx_reserve_spread_alloc"
case(c, "fine")
case(c, "null-handle", h=None)
edge(c, "n_rows-negative", dict(n_rows=-1), dict(n_rows=0))
case(c, "n_rows-range-refused", n_rows=1 << 31)
c = "ofdm_tx_dft_spread_alloc"
case(c, "null-handle", h=None)
edge(c, "n_rows-negative", dict(n_rows=-1), dict(n_rows=0))
states = WITH_A_SET
edge(c, "row_len-short", dict(row_len=11), dict(row_len=12))
case(c, "row_len-short-odd-set", row_len=5)
edge(c, "row_len-range", dict(row_len=ROW + 1), dict(row_len=ROW))
edge(c, "rows-range", dict(n_rows=LEN // ROW + 1, row_len=ROW), dict(n_rows=LEN // ROW, row_len=ROW))
edge(c, "workgroups-two-allocations", dict(n_rows=GROUPS // 4 + 1), dict(n_rows=GROUPS // 4))
edge(c, "workgroups-one-allocation", dict(n_rows=GROUPS // 2 + 1), dict(n_rows=GROUPS // 2))
case(c, "noop-no-rows", n_rows=0, d_sym="BUF", d_out="BUF")
case(c, "null-d_sym", d_out="BUF")
states = EVERY
case(c, "null-d_out", d_sym="BUF")
c = "ofdm_tx_modulate_frames_alloc"
tx_composite_edges(c)

# ------------------------------------------------------------------------------------------ receiver: one M
c = "ofdm_rx_reserve_despread"
case(c, "fine")
case(c, "null-handle", h=None)
size_edges(c)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
case(c, "n_seg-range-refused", n_seg=N31 + 1)
c = "ofdm_dft_despread_frames"
CSI = dict(d_csi="BUF", csi_stride=12)
case(c, "null-handle", h=None)
size_edges(c, seg_stride=1)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "rows-negative", dict(rows=-1), dict(rows=0))
edge(c, "rows-range", dict(rows=LEN // 12 + 1, seg_stride=LEN), dict(rows=LEN // 12, seg_stride=LEN // 12 * 12))
edge(c, "seg_stride-short", dict(seg_stride=11), dict(seg_stride=12))
edge(c, "modulation-bpsk", dict(modulation=1), dict(modulation=2))
edge(c, "modulation-3", dict(modulation=3), dict(modulation=4))
edge(c, "modulation-high", dict(modulation=7), dict(modulation=6))
edge(c, "csi_stride-short", dict(d_csi="BUF", csi_stride=11), CSI)
case(c, "csi_stride-unread-without-d_csi", csi_stride=-1, noise_mode=7, rho=NAN)
ds_noise_edges(c, CSI)
rho_edges(c, CSI)
want_edges(c)
edge(c, "packed-whole-bytes", dict(M=6, out={"bits": "BUF"}, bits_mode=P), dict(M=4, out={"bits": "BUF"}, bits_mode=P))
case(c, "unpacked-any-M-passes", M=6, out={"bits": "BUF"}, bits_mode=U)
edge(c, "in-place-strides", dict(n_seg=0, d_sym="BUF", out={"sym": "BUF"}, seg_stride=13), dict(n_seg=0, d_sym="BUF", out={"sym": "BUF"}))
edge(c, "n_seg-range", dict(n_seg=N31 + 1), dict(n_seg=GROUPS))
case(c, "n_seg-2^31-workgroups-refused", n_seg=N31)
edge(c, "batch-seg_stride", dict(n_seg=2, seg_stride=LEN // 2 + 1), dict(n_seg=2, seg_stride=LEN // 2))
edge(c, "batch-csi_stride", dict(n_seg=2, d_csi="BUF", csi_stride=LEN // 2 + 1), dict(n_seg=2, d_csi="BUF", csi_stride=LEN // 2))
WG = dict(M=1, n_seg=1 << 23, seg_stride=1 << 17)           # rows_per_group 256: 255 workgroups per segment are the last that fit
edge(c, "workgroups", dict(WG, rows=255 * 256 + 1), dict(WG, rows=255 * 256))
case(c, "noop-no-segments", n_seg=0, d_sym="BUF")
case(c, "noop-no-rows", rows=0, d_sym="BUF")
case(c, "null-d_sym")
c = "ofdm_rx_demod_frames_despread"
open_edges(c)
case(c, "batch-range-refused", n_frames=DEMOD_MAX + 1)
ds_noise_edges(c, {})
want_edges(c)
case(c, "packed-passes", out={"bits": "BUF"}, bits_mode=P)
case(c, "in-place-passes", out={"sym": "BUF"})

# ------------------------------------------------------------------------------------------ receiver: B branches, one M
c = "ofdm_rx_reserve_mrc_despread"
case(c, "fine")
case(c, "null-handle", h=None)
size_edges(c)
branch_edges(c)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
case(c, "units-range-refused", n_seg=N31 // 2 + 1)
case(c, "M-in-front-of-n_branch-refused", M=7, n_branch=0)
c = "ofdm_combine_despread_frames"
case(c, "null-handle", h=None)
size_edges(c, seg_stride=1, csi_stride=1)
case(c, "M-in-front-of-est-refused", M=7, noise_mode=M_EST)
case(c, "est-in-front-of-negative-count-refused", noise_mode=M_EST, n_seg=-1)
mrc_arg_edges(c)
edge(c, "modulation-bpsk", dict(modulation=1), dict(modulation=2))
edge(c, "modulation-high", dict(modulation=7), dict(modulation=6))
want_edges(c)
edge(c, "packed-whole-bytes", dict(M=6, out={"bits": "BUF"}, bits_mode=P), dict(M=4, out={"bits": "BUF"}, bits_mode=P))
case(c, "rho-in-front-of-out-refused", rho=NAN, out=None)
WG = dict(M=1, n_branch=1, n_seg=1 << 23, seg_stride=1 << 17, h_noise_var=[1.0])
edge(c, "workgroups", dict(WG, rows=255 * 256 + 1), dict(WG, rows=255 * 256))
c = "ofdm_rx_demod_frames_mrc_despread"
open_edges(c)
branch_edges(c)
case(c, "n_branch-in-front-of-d_eq-refused", n_branch=0, d_eq=None)
case(c, "units-range-refused", n_frames=N31 // 2 + 1)
case(c, "units-2^31-batch-refused", n_frames=N31 // 2)
case(c, "batch-range-refused", n_frames=(DEMOD_MAX + 1) // 2)
mrc_noise_edges(c)
want_edges(c)
case(c, "packed-passes", out={"bits": "BUF"}, bits_mode=P)

# ------------------------------------------------------------------------------------------ receiver: the allocation set
c = "ofdm_rx_reserve_despread_alloc"
case(c, "fine-or-no-set")
case(c, "null-handle", h=None)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
case(c, "n_seg-range-one-allocation-refused", n_seg=GROUPS + 1)
states = ("none", "set")                     # a set of one allocation would reserve this many segments
case(c, "n_seg-range-two-allocations-refused", n_seg=GROUPS // 2 + 1)
states = EVERY
c = "ofdm_dft_despread_alloc_frames"
case(c, "null-handle", h=None)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
states = WITH_A_SET
edge(c, "rows-negative", dict(rows=-1), dict(rows=0))
edge(c, "row_len-short", dict(row_len=11, seg_stride=11), dict(row_len=12))
case(c, "row_len-short-odd-set", row_len=5, seg_stride=5)
edge(c, "row_len-range", dict(row_len=ROW + 1, seg_stride=ROW + 1), dict(row_len=ROW, seg_stride=ROW))
edge(c, "rows-range", dict(rows=LEN // 12 + 1, seg_stride=LEN), dict(rows=LEN // 12, seg_stride=LEN // 12 * 12))
edge(c, "seg_stride-short", dict(seg_stride=11), dict(seg_stride=12))
edge(c, "csi_stride-short", dict(d_csi="BUF", csi_stride=11), CSI)
case(c, "in-place-refused", n_seg=0, d_sym="BUF", out={"sym": "BUF"})
case(c, "in-place-behind-no-set-null-out-refused", n_seg=0, d_sym="BUF", out=None)
ds_noise_edges(c, CSI)
rho_edges(c, CSI)
want_edges(c)
edge(c, "packed", dict(out={"bits": "BUF"}, bits_mode=P), dict(out={"bits": "BUF"}, bits_mode=U))
edge(c, "n_seg-range", dict(n_seg=N31 + 1), dict(n_seg=N31))
edge(c, "workgroups-sum-two-allocations", dict(n_seg=1 << 30), dict(n_seg=(1 << 30) - 1))
edge(c, "batch-seg_stride", dict(n_seg=2, seg_stride=LEN // 2 + 1), dict(n_seg=2, seg_stride=LEN // 2))
case(c, "noop-no-segments", n_seg=0, d_sym="BUF")
case(c, "noop-no-rows", rows=0, d_sym="BUF")
states = EVERY
case(c, "null-d_sym")
c = "ofdm_rx_demod_frames_despread_alloc"
open_edges(c)
case(c, "batch-range-refused", n_frames=DEMOD_MAX + 1)
case(c, "no-set-in-front-of-the-checks-of-the-stage", noise_mode=-1)
states = WITH_A_SET
ds_noise_edges(c, {})
want_edges(c)
edge(c, "packed", dict(out={"bits": "BUF"}, bits_mode=P), dict(out={"bits": "BUF"}, bits_mode=U))
case(c, "in-place-refused", out={"sym": "BUF"})
states = EVERY

# ------------------------------------------------------------------------------------------ receiver: B branches per allocation
c = "ofdm_rx_reserve_mrc_despread_alloc"
case(c, "fine")
case(c, "null-handle", h=None)
branch_edges(c)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "row_len-negative", dict(row_len=-1), dict(row_len=0))
case(c, "units-range-refused", n_seg=N31 // 2 + 1)
edge(c, "row_len-range", dict(row_len=ROW + 1), dict(row_len=ROW))
case(c, "units-row_len-refused", n_branch=1, n_seg=N31, row_len=513)
c = "ofdm_combine_despread_alloc_frames"
case(c, "null-handle", h=None)
case(c, "null-d_csi-in-front-of-the-arguments-refused", d_csi=None, n_seg=-1)
case(c, "est-in-front-of-negative-count-refused", noise_mode=M_EST, n_seg=-1)
mrc_arg_edges(c)
edge(c, "row_len-negative", dict(row_len=-1, seg_stride=0), dict(row_len=0, seg_stride=0, csi_stride=0))
edge(c, "row_len-short", dict(row_len=11, seg_stride=11, csi_stride=11), dict(row_len=12))
edge(c, "row_len-range", dict(row_len=ROW + 1, seg_stride=ROW + 1, csi_stride=ROW + 1), dict(row_len=ROW, seg_stride=ROW, csi_stride=ROW))
want_edges(c)
edge(c, "packed", dict(out={"bits": "BUF"}, bits_mode=P), dict(out={"bits": "BUF"}, bits_mode=U))
case(c, "in-place-sym-refused", d_sym="BUF", out={"sym": "BUF"})
case(c, "in-place-comb-refused", d_sym="BUF", out={"comb": "BUF"})
case(c, "in-place-in-front-of-no-set-refused", d_sym="BUF", out={"sym": "BUF"}, row_len=0, seg_stride=0, csi_stride=0)
ONE = dict(n_branch=1, h_noise_var=[1.0])
edge(c, "workgroups-arguments-alone", dict(ONE, n_seg=N31), dict(ONE, n_seg=GROUPS))
case(c, "workgroups-unread-without-rows-passes", rows=0, **dict(ONE, n_seg=N31))
edge(c, "workgroups-sum-two-allocations", dict(ONE, n_seg=1 << 30), dict(ONE, n_seg=(1 << 30) - 1))
c = "ofdm_rx_demod_frames_mrc_despread_alloc"
open_edges(c)
branch_edges(c)
case(c, "n_branch-in-front-of-d_eq-refused", n_branch=0, d_eq=None)
case(c, "units-range-refused", n_frames=N31 // 2 + 1)
case(c, "units-2^31-batch-refused", n_frames=N31 // 2)
case(c, "batch-range-refused", n_frames=(DEMOD_MAX + 1) // 2)
mrc_noise_edges(c)
want_edges(c)
edge(c, "packed", dict(out={"bits": "BUF"}, bits_mode=P), dict(out={"bits": "BUF"}, bits_mode=U))
case(c, "in-place-refused", out={"sym": "BUF"})

# ------------------------------------------------------------------------------------------ capi_mrc
c = "ofdm_rx_reserve_mrc"
case(c, "fine")
case(c, "null-handle", h=None)
edge(c, "n_seg-negative", dict(n_seg=-1), dict(n_seg=0))
edge(c, "rows-negative", dict(rows=-1), dict(rows=0))
edge(c, "row_len-negative", dict(row_len=-1), dict(row_len=0))
branch_edges(c)
case(c, "negative-count-in-front-of-n_branch-refused", n_seg=-1, n_branch=0)
case(c, "units-range-refused", n_seg=N31 // 2 + 1)
edge(c, "row_len-range", dict(row_len=ROW + 1), dict(row_len=ROW))
edge(c, "rows-range", dict(row_len=12, rows=LEN // 12 + 1), dict(row_len=12, rows=LEN // 12))
case(c, "units-row_len-refused", n_branch=1, n_seg=N31, row_len=513)
c = "ofdm_combine_csi_frames"
case(c, "null-handle", h=None)
mrc_arg_edges(c)
edge(c, "row_len-negative", dict(row_len=-1, seg_stride=0), dict(row_len=0, seg_stride=0, csi_stride=0))
edge(c, "row_len-range", dict(row_len=ROW + 1, seg_stride=ROW + 1, csi_stride=ROW + 1), dict(row_len=ROW, seg_stride=ROW, csi_stride=ROW))
edge(c, "modulation-bpsk", dict(modulation=1), dict(modulation=2))
edge(c, "modulation-high", dict(modulation=7), dict(modulation=6))
case(c, "noop-null-out", out=None, d_sym="BUF", d_csi="BUF")
case(c, "noop-nothing-wanted", out={}, d_sym="BUF", d_csi="BUF")
case(c, "noop-no-row", row_len=0, seg_stride=0, csi_stride=0, d_sym="BUF", d_csi="BUF")
case(c, "negative-count-in-front-of-n_branch-refused", n_seg=-1, n_branch=0)
c = "ofdm_rx_demod_frames_mrc"
open_edges(c)
branch_edges(c)
case(c, "units-range-refused", n_frames=N31 // 2 + 1)
case(c, "units-2^31-batch-refused", n_frames=N31 // 2)
case(c, "batch-range-refused", n_frames=(DEMOD_MAX + 1) // 2)
mrc_noise_edges(c, est="passes")
case(c, "noop-null-out", out=None)
case(c, "noop-nothing-wanted", out={})

IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)


class Runner(codec.Runner):
    """the codec table's Runner over this table's calls: host arrays for the lists, and the allocation sets of the two handles"""
    calls, out_types = CALLS, OUT_TYPES

    def value(self, call, name, v):
        if isinstance(v, list):
            a = ((C.c_double if name == "h_noise_var" else C.c_int32) * len(v))(*v)
            self.keep.append(a)
            return a if name == "h_noise_var" else C.cast(a, C.c_void_p)
        return super().value(call, name, v)

    def set_state(self, state):
        self.rx.set_allocations(STATES[state])
        self.tx.set_allocations([a[:2] for a in STATES[state]])

    def run_all(self, calls=None):
        """{call: {case: [status, text], or {state: [status, text]} where the states of the case differ}}"""
        out = {}
        for state in STATES:
            self.set_state(state)
            for cid, call, kwargs, where in CASES:
                if state in where and (calls is None or call in calls):
                    out.setdefault(call, {}).setdefault(cid.split("/")[1], {})[state] = self.run(call, kwargs)
        self.set_state("none")
        return {call: {n: next(iter(v.values())) if len(set(map(str, v.values()))) == 1 else v for n, v in of.items()}
                for call, of in out.items()}
