"""Host-side engines over the C ABI: receive chain, transmit chain, loop-back channel, de-mapper.

Nothing here computes samples on the CPU; NumPy is used for buffers and for the small fp64
constant tables the reference exposes as block attributes (Zadoff-Chu sequence, bin lists).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BITS_NONE, BITS_PACKED, BITS_UNPACKED, CSI_NOISE_EST, CSI_ROWS_ALL, CSI_ROWS_DATA, MODULATION_BITS, MRC_NOISE_EST,
                   MRC_NOISE_GIVEN, MRC_NOISE_SEG, PILOT_CPE, check, ptr)


def bins_p(num_bins: int, nfft: int) -> np.ndarray:
    """binsP(K): [-K/2..-1, 1..K/2] + N mod N  (gr-utsa_ofdm/python/SynchAndChanEst.py:38-41,66-70)."""
    h = int(num_bins / 2)
    return (np.array(list(range(-h, 0)) + list(range(1, h + 1)), dtype=np.int64) + nfft) % nfft


def zadoff_chu(mm: int, root: int, parity_of: int | None = None) -> np.ndarray:
    """SynchAndChanEst.py:52-59 (root 23) / gr-RXOFDM synch_and_chan_est.py:54-64 (root 37)."""
    par = mm if parity_of is None else parity_of
    x0 = np.arange(mm, dtype=np.float64)
    q = x0 ** 2 / 2 if par % 2 == 0 else x0 * (x0 + 1) / 2
    return np.exp(-1j * (2 * np.pi / mm) * root * q)


def _mod_bits(modulation) -> int:
    if isinstance(modulation, str):
        return MODULATION_BITS[modulation.upper().replace("-", "")]
    return int(modulation)


def _addr(x):
    """Address of a buffer as an int (None stays None): the pointer fields of the *Out structures."""
    p = ptr(x)
    return None if p is None else p.value


def _work(fn, handle, report, in0: np.ndarray, out: np.ndarray) -> int:
    """One work() call of a stream block (fn = ofdm_rx_work / ofdm_fo_work): raw status; `out` is written through a
    contiguous complex64 copy where it is not one itself."""
    in0 = np.ascontiguousarray(in0, dtype=np.complex64)
    if out.dtype != np.complex64 or not out.flags.c_contiguous:
        tmp = np.ascontiguousarray(out, dtype=np.complex64)
        rc = fn(handle, ptr(in0), in0.size, ptr(tmp), tmp.size, C.byref(report))
        if rc >= 0:
            out[...] = tmp
        return int(rc)
    return int(fn(handle, ptr(in0), in0.size, ptr(out), out.size, C.byref(report)))


class _Handle:
    """What the four engines share: the library handle `_h`, destroyed once by the library function named in `_destroy`
    (close(), or when the object is collected)."""
    _destroy = ""

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self.lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """Plain HBM allocation through the C ABI (for hosts that do not use torch)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.lib = _lib.load()
        self.device = device
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(self.lib.ofdm_device_malloc(device, C.byref(p), self.nbytes))
        self._ptr = p.value or 0

    def data_ptr(self) -> int:
        return self._ptr

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(self.lib.ofdm_memcpy_h2d(self.device, ptr(self), ptr(arr), arr.nbytes))
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        """Blocking device-to-host copy; waits for ALL streams of the device first (the batch entry points
        are asynchronous on the handles' non-blocking streams)."""
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self.lib.ofdm_device_synchronize(self.device))
        check(self.lib.ofdm_memcpy_d2h(self.device, ptr(out), ptr(self), out.nbytes))
        return out

    def free(self):
        if self._ptr:
            self.lib.ofdm_device_free(self.device, C.c_void_p(self._ptr))
            self._ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def count_bit_errors(d_a, d_b, n_bytes: int, d_count, stream=None, device: int = 0):
    """*d_count (device uint64, zeroed by the caller) += popcount(a ^ b) over n_bytes of two device byte strings."""
    check(_lib.load().ofdm_count_bit_errors(int(device), ptr(d_a), ptr(d_b), int(n_bytes), ptr(d_count), ptr(stream)))


def tbcc_blocks(seg_bits: int, K: int) -> int:
    """ofdm_tbcc_blocks: the TBCC code blocks of K information bits (3K coded bits each) a segment of seg_bits bits can carry."""
    return int(check(_lib.load().ofdm_tbcc_blocks(int(seg_bits), int(K))))


def tbcc_rm_blocks(seg_bits: int, K: int, E: int) -> int:
    """ofdm_tbcc_rm_blocks: the rate-matched TBCC code blocks (K information bits in E coded bits) a segment of seg_bits carries."""
    return int(check(_lib.load().ofdm_tbcc_rm_blocks(int(seg_bits), int(K), int(E))))


def turbo_blocks(seg_bits: int, K: int) -> int:
    """ofdm_turbo_blocks: the turbo code blocks of K information bits (3K + 12 coded bits each) a segment of seg_bits carries."""
    return int(check(_lib.load().ofdm_turbo_blocks(int(seg_bits), int(K))))


def turbo_rm_blocks(seg_bits: int, K: int, E: int) -> int:
    """ofdm_turbo_rm_blocks: the rate-matched turbo code blocks (K information bits in E coded bits) a segment of seg_bits carries."""
    return int(check(_lib.load().ofdm_turbo_rm_blocks(int(seg_bits), int(K), int(E))))


def turbo_rm_info(K: int, Ncb: int = 0, rv: int = 0) -> tuple:
    """ofdm_turbo_rm_info: (k0, Navail) of the turbo rate matcher's circular buffer for block size K, buffer length Ncb (0 = all
    of it) and redundancy version rv; host arithmetic."""
    k0, navail = C.c_int32(), C.c_int32()
    check(_lib.load().ofdm_turbo_rm_info(int(K), int(Ncb), int(rv), C.byref(k0), C.byref(navail)))
    return int(k0.value), int(navail.value)


def turbo_qpp_check(K: int, f1: int, f2: int) -> bool:
    """ofdm_turbo_qpp_check: True iff K is a valid block size, 0 <= f1, f2 < K and (f1 i + f2 i^2) mod K is a permutation."""
    return _lib.load().ofdm_turbo_qpp_check(int(K), int(f1), int(f2)) == 0


def dft_size_ok(M: int) -> bool:
    """ofdm_dft_size_ok: True iff M = 2^a 3^b 5^c and 1 <= M <= 4096, the sizes of the DFT-spread OFDM transforms."""
    return -2 ** 31 <= int(M) < 2 ** 31 and _lib.load().ofdm_dft_size_ok(int(M)) == 1


def dft_plan_info(M: int) -> tuple:
    """ofdm_dft_plan_info: (passes, radix-8 passes among them, rows a workgroup transforms at once) of the plan for M."""
    n_pass, radix8, rpg = C.c_int32(), C.c_int32(), C.c_int32()
    check(_lib.load().ofdm_dft_plan_info(int(M), C.byref(n_pass), C.byref(radix8), C.byref(rpg)))
    return int(n_pass.value), int(radix8.value), int(rpg.value)


def _alloc_arrays(allocs, width):
    """(n, start, M[, mod]) of a list of allocations as contiguous int32 arrays"""
    a = np.asarray(list(allocs), dtype=np.int64).reshape(-1, width) if len(allocs) else np.zeros((0, width), np.int64)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("allocation entries must fit int32")
    return (int(a.shape[0]),) + tuple(np.ascontiguousarray(a[:, k], dtype=np.int32) for k in range(width))


def alloc_layout(M, mod, n_seg: int, rows: int, bits_mode: int = BITS_NONE) -> dict:
    """ofdm_alloc_layout: where the blocks of an allocation set lie in the allocation-major outputs of
    RxEngine.dft_despread_alloc_frames.  M and mod are the sizes and bits per symbol of the allocations in list order.  Returns
    dict(sym_off, llr_off, bits_off: int64 arrays; sym, llr, bits: the totals) in complex items, floats and bytes."""
    M = np.ascontiguousarray(M, dtype=np.int32)
    mod = np.ascontiguousarray(mod, dtype=np.int32)
    if M.ndim != 1 or M.shape != mod.shape:
        raise ValueError("M and mod must be lists of one length")
    n = int(M.size)
    so, lo, bo = (np.zeros(max(n, 1), np.int64) for _ in range(3))
    tot = np.zeros(3, np.int64)
    check(_lib.load().ofdm_alloc_layout(n, ptr(M) if n else None, ptr(mod) if n else None, int(n_seg), int(rows), int(bits_mode),
                                        ptr(so), ptr(lo), ptr(bo), ptr(tot)))
    return dict(sym_off=so[:n], llr_off=lo[:n], bits_off=bo[:n], sym=int(tot[0]), llr=int(tot[1]), bits=int(tot[2]))


def crc_bits(kind: int) -> int:
    """ofdm_crc_bits: the parity bits L of a CRC kind (CRC24A, CRC24B: 24, CRC16: 16, CRC8: 8)."""
    return int(check(_lib.load().ofdm_crc_bits(int(kind))))


def crc_compute(kind: int, bits_packed, A: int | None = None) -> int:
    """ofdm_crc_compute: the unmasked parity (an L-bit integer, p0 on top) of A payload bits packed MSB-first; host arithmetic."""
    buf = np.ascontiguousarray(bits_packed, dtype=np.uint8)
    A = 8 * buf.size if A is None else int(A)
    if A > 8 * buf.size:
        raise ValueError("crc_compute: A = %d bits from %d bytes" % (A, buf.size))
    crc = C.c_uint32(0)
    check(_lib.load().ofdm_crc_compute(int(kind), ptr(buf), A, C.byref(crc)))
    return int(crc.value)


def crc_compute_long(kind: int, bits_packed, n_bits: int | None = None) -> int:
    """ofdm_crc_compute_long: crc_compute for up to 2^30 bits, through the kernels' chunk-and-combine routine; host arithmetic."""
    buf = np.ascontiguousarray(bits_packed, dtype=np.uint8)
    n_bits = 8 * buf.size if n_bits is None else int(n_bits)
    if n_bits > 8 * buf.size:
        raise ValueError("crc_compute_long: %d bits from %d bytes" % (n_bits, buf.size))
    crc = C.c_uint32(0)
    check(_lib.load().ofdm_crc_compute_long(int(kind), ptr(buf), n_bits, C.byref(crc)))
    return int(crc.value)


def turbo_k_next(bits: int) -> int:
    """ofdm_turbo_k_next: the smallest of LTE's 188 turbo block sizes that holds `bits` bits."""
    return int(check(_lib.load().ofdm_turbo_k_next(int(bits))))


def tb_geometry(A: int, Z: int = 0, G: int = 0, q: int = 1, N_IR: int = 0) -> dict:
    """ofdm_tb_geometry: segmentation of a transport block of A bits at maximum block size Z (0 = 6144), and with G > 0 the
    rate-matching sizes for G coded bits in units of q under the soft-buffer limit N_IR (0 = none); host arithmetic.  A dict of
    the fields of ofdm_tb_geom, `groups` a list of dicts (first, count, K, E, cw_bit_offset, soft_offset)."""
    g = _lib.TbGeom()
    check(_lib.load().ofdm_tb_geometry(int(A), int(Z), int(G), int(q), int(N_IR), C.byref(g)))
    out = {n: int(getattr(g, n)) for n, _ in _lib.TbGeom._fields_ if n != "group"}
    out["groups"] = [{n: int(getattr(g.group[i], n)) for n, _ in _lib.TbGroup._fields_} for i in range(g.n_groups)]
    return out


def gold_bits(c_init: int, first: int, n: int) -> np.ndarray:
    """ofdm_gold_bits: c(first .. first + n - 1) of TS 36.211 7.2 for c_init, one bit per byte; host arithmetic, random access."""
    out = np.empty(max(int(n), 0), np.uint8)
    check(_lib.load().ofdm_gold_bits(int(c_init) & 0xFFFFFFFF, int(first), int(n), ptr(out)))
    return out


class RxEngine(_Handle):
    """Receive chain handle (sync search, LS channel estimate, FFT + equalise, de-map)."""
    _destroy = "ofdm_rx_destroy"

    def __init__(self, num_ofdm_symb, nfft, cp_len, num_synch_bins, synch_dat, num_data_bins, snr,
                 scale_factor_gate=0.7, compat=_lib.COMPAT_UTSA, modulation="QPSK", device=0):
        self.lib = _lib.load()
        self.cfg = _lib.RxCfg(int(num_ofdm_symb), int(nfft), int(cp_len), int(num_synch_bins), int(synch_dat[0]),
                              int(synch_dat[1]), int(num_data_bins), float(snr), float(scale_factor_gate),
                              int(compat), _mod_bits(modulation), int(device), 0)
        h = C.c_void_p()
        check(self.lib.ofdm_rx_create(C.byref(self.cfg), C.byref(h)))
        self._h = h
        self.report = _lib.RxReport()

    # ---- stream block -----------------------------------------------------------------------
    def work(self, in0: np.ndarray, out: np.ndarray) -> int:
        """Returns the raw status; the caller copies `self.report` (valid even when the reference would have
        raised after its sync search) and then passes the status to `_lib.check`."""
        return _work(self.lib.ofdm_rx_work, self._h, self.report, in0, out)

    def state(self, row: int = 0):
        c = self.cfg
        mm = c.synch_S * c.num_synch_bins
        H = np.zeros(c.nfft, np.complex64)
        ht = np.zeros(c.nfft, np.complex64)
        esf = np.zeros(mm, np.complex64)
        eqg = np.zeros(c.num_synch_bins, np.complex64)
        edf = np.zeros((c.num_ofdm_symb, c.num_data_bins), np.complex64)
        check(self.lib.ofdm_rx_get_state(self._h, row, ptr(H), ptr(ht), ptr(esf), ptr(eqg), ptr(edf)))
        return dict(chan_freq=H, chan_time=ht, synch_freq=esf, eq_gain=eqg, data_freq=edf)

    # ---- frame batches on device buffers ----------------------------------------------------
    def data_symbols_per_frame(self, frame_len: int) -> int:
        c = self.cfg
        return (frame_len // (c.nfft + c.cp_len)) // (c.synch_S + c.synch_D) * c.synch_D

    def reserve(self, n_frames: int):
        check(self.lib.ofdm_rx_reserve(self._h, int(n_frames)))

    def demod_frames(self, d_iq, n_frames, frame_stride, frame_len, d_eq=None, d_bits=None,
                     bits_mode=BITS_NONE, d_tsr=None, stream=None) -> int:
        return int(check(self.lib.ofdm_rx_demod_frames(self._h, ptr(d_iq), int(n_frames), int(frame_stride),
                                                       int(frame_len), ptr(d_eq), ptr(d_bits), int(bits_mode),
                                                       ptr(d_tsr), ptr(stream))))

    def set_profiling(self, enable: bool = True):
        check(self.lib.ofdm_rx_set_profiling(self._h, int(bool(enable))))

    def kernel_ms(self):
        """(sync_ms, demod_ms) of the last demod_frames call (needs set_profiling(True))."""
        a, b = C.c_float(), C.c_float()
        check(self.lib.ofdm_rx_get_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def set_sync_search(self, exhaustive: bool) -> bool:
        """True if the screened sync search is active afterwards (False: the exhaustive, trial-by-trial one)."""
        return bool(check(self.lib.ofdm_rx_set_sync_search(self._h, int(bool(exhaustive)))))

    def set_max_trials(self, n: int):
        check(self.lib.ofdm_rx_set_max_trials(self._h, int(n)))

    def frame_state(self, frame: int):
        c = self.cfg
        H = np.zeros(c.nfft, np.complex64)
        g = np.zeros(c.num_data_bins, np.complex64)
        ht = np.zeros(c.nfft, np.complex64)
        check(self.lib.ofdm_rx_get_frame_state(self._h, int(frame), ptr(H), ptr(g), ptr(ht)))
        return dict(chan_freq=H, gain=g, chan_time=ht)

    def demap(self, d_sym, n, modulation="QPSK", d_hard=None, d_soft0=None, d_soft1=None, stream=None):
        check(self.lib.ofdm_demap(self._h, ptr(d_sym), int(n), _mod_bits(modulation), ptr(d_hard), ptr(d_soft0),
                                  ptr(d_soft1), ptr(stream)))

    # ---- segmented soft de-mapper: one sigma per segment (per frame of a batch) ----------------------------------
    @staticmethod
    def _soft_out(d_soft0, d_soft1, d_llr, d_sigma):
        return _lib.SoftOut(_addr(d_soft0), _addr(d_soft1), _addr(d_llr), _addr(d_sigma))

    def reserve_soft(self, n_seg: int, seg_len: int):
        """Workspace of demap_frames / demod_frames_soft for n_seg segments of seg_len symbols (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_soft(self._h, int(n_seg), int(seg_len)))

    def demap_frames(self, d_sym, n_seg, seg_len, seg_stride, modulation, d_soft0=None, d_soft1=None, d_llr=None, d_sigma=None,
                     stream=None):
        """ofdm_demap_frames: segment s = seg_len complex64 symbols at d_sym + s*seg_stride, each de-mapped as ofdm_demap would
        de-map it alone.  Outputs [n_seg][seg_len*bps] float32 soft0 / soft1 / llr = soft0 - soft1, sigma [n_seg] float64."""
        out = self._soft_out(d_soft0, d_soft1, d_llr, d_sigma)
        check(self.lib.ofdm_demap_frames(self._h, ptr(d_sym), int(n_seg), int(seg_len), int(seg_stride), _mod_bits(modulation),
                                         C.byref(out), ptr(stream)))

    def demod_frames_soft(self, d_iq, n_frames, frame_stride, frame_len, d_eq, d_soft0=None, d_soft1=None, d_llr=None,
                          d_sigma=None, d_bits=None, bits_mode=BITS_NONE, d_tsr=None, stream=None) -> int:
        """demod_frames, then demap_frames over d_eq with one segment per frame (n_dsym*Kd symbols, the handle's modulation).
        Returns n_dsym."""
        out = self._soft_out(d_soft0, d_soft1, d_llr, d_sigma)
        return int(check(self.lib.ofdm_rx_demod_frames_soft(self._h, ptr(d_iq), int(n_frames), int(frame_stride),
                                                            int(frame_len), ptr(d_eq), ptr(d_bits), int(bits_mode),
                                                            ptr(d_tsr), C.byref(out), ptr(stream))))

    # ---- pilot-aided phase tracking: cfg.num_data_bins = occupied bins K, Kd' = K - n_pilots data entries per row ---------
    def set_pilots(self, locations, value=1.0 + 0.0j):
        """Signed bin offsets of the pilots (e.g. -21, -7, 7, 21) and their value, as TxEngine.set_pilots; () clears them."""
        loc = np.ascontiguousarray(list(locations), dtype=np.int32)
        check(self.lib.ofdm_rx_set_pilots(self._h, ptr(loc) if loc.size else None, int(loc.size), float(np.real(value)),
                                          float(np.imag(value))))
        self.n_pilots = int(loc.size)

    @staticmethod
    def _pilot_out(d_data, d_bits, bits_mode, d_cpe, d_slope, d_cfo):
        return _lib.PilotOut(_addr(d_data), _addr(d_bits), int(bits_mode), _addr(d_cpe), _addr(d_slope), _addr(d_cfo))

    def reserve_pilots(self, n_seg: int, rows: int):
        """Workspace of the cfo output for n_seg segments of `rows` rows (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_pilots(self._h, int(n_seg), int(rows)))

    def pilot_track_frames(self, d_sym, n_seg, rows, seg_stride, rows_per_pattern, mode=PILOT_CPE, d_data=None, d_bits=None,
                           bits_mode=BITS_NONE, d_cpe=None, d_slope=None, d_cfo=None, stream=None):
        """ofdm_pilot_track_frames: segment s = `rows` rows of K complex64 symbols at d_sym + s*seg_stride.  Outputs per segment:
        data [rows][Kd'] complex64, its hard bits, cpe [rows] complex64, slope [rows] float32, cfo float64."""
        out = self._pilot_out(d_data, d_bits, bits_mode, d_cpe, d_slope, d_cfo)
        check(self.lib.ofdm_pilot_track_frames(self._h, ptr(d_sym), int(n_seg), int(rows), int(seg_stride), int(rows_per_pattern),
                                               int(mode), C.byref(out), ptr(stream)))

    def demod_frames_pilots(self, d_iq, n_frames, frame_stride, frame_len, d_eq, mode=PILOT_CPE, d_data=None, d_bits=None,
                            bits_mode=BITS_NONE, d_cpe=None, d_slope=None, d_cfo=None, d_soft0=None, d_soft1=None, d_llr=None,
                            d_sigma=None, d_tsr=None, stream=None) -> int:
        """demod_frames (d_eq: rows of K symbols), the pilot stage over d_eq with one segment per frame, then demap_frames over
        d_data (n_dsym*Kd' symbols per frame) if a soft output is given.  Returns n_dsym."""
        out = self._pilot_out(d_data, d_bits, bits_mode, d_cpe, d_slope, d_cfo)
        soft = self._soft_out(d_soft0, d_soft1, d_llr, d_sigma)
        return int(check(self.lib.ofdm_rx_demod_frames_pilots(self._h, ptr(d_iq), int(n_frames), int(frame_stride),
                                                              int(frame_len), ptr(d_eq), ptr(d_tsr), int(mode), C.byref(out),
                                                              C.byref(soft), ptr(stream))))

    # ---- channel-state-weighted LLRs: every symbol weighed with |H|^2 of its bin (include/ofdm_mi355x.h) ---------------------
    @staticmethod
    def _csi_out(d_llr, d_sigma2, d_n_used):
        return _lib.CsiOut(_addr(d_llr), _addr(d_sigma2), _addr(d_n_used))

    @property
    def csi_rho(self) -> float:
        """1/SNR of the handle's data equaliser as the library holds it (float32): the rho of demap_csi_frames behind this
        receiver (SynchAndChanEst.py:99,245 takes 10^(snr/20); the RXOFDM blocks take snr itself)."""
        snr = 10.0 ** (self.cfg.snr / 20.0) if self.cfg.compat == _lib.COMPAT_UTSA else self.cfg.snr
        return float(np.float32(1.0 / snr))

    def reserve_csi(self, n_seg: int, rows: int, row_len: int):
        """Workspace of csi_frames / demap_csi_frames / demod_frames_csi for n_seg segments of `rows` rows of row_len symbols
        (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_csi(self._h, int(n_seg), int(rows), int(row_len)))

    def csi_frames(self, n_frames, d_csi, csi_stride=None, layout=CSI_ROWS_ALL, stream=None):
        """ofdm_rx_csi_frames: d_csi[f][j] = |H|^2 (float32) of frame f of the last demod_frames call, j over bins_p(Kd)
        (CSI_ROWS_ALL) or over the non-pilot entries (CSI_ROWS_DATA).  csi_stride defaults to the entries per row."""
        if csi_stride is None:
            csi_stride = self.cfg.num_data_bins - (getattr(self, "n_pilots", 0) if layout == CSI_ROWS_DATA else 0)
        check(self.lib.ofdm_rx_csi_frames(self._h, int(n_frames), int(layout), ptr(d_csi), int(csi_stride), ptr(stream)))

    def demap_csi_frames(self, d_sym, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, modulation, d_llr=None,
                         d_sigma2=None, d_n_used=None, noise_mode=CSI_NOISE_EST, noise_var=0.0, stream=None):
        """ofdm_demap_csi_frames: segment s = `rows` rows of row_len complex64 symbols at d_sym + s*seg_stride, entry j of every
        row weighed with d_csi[s*csi_stride + j].  Outputs llr [n_seg][rows*row_len*bps] float32 (positive favours bit 0),
        sigma2 [n_seg] float64, n_used [n_seg] int64."""
        out = self._csi_out(d_llr, d_sigma2, d_n_used)
        check(self.lib.ofdm_demap_csi_frames(self._h, ptr(d_sym), int(n_seg), int(rows), int(row_len), int(seg_stride), ptr(d_csi),
                                             int(csi_stride), float(rho), _mod_bits(modulation), int(noise_mode), float(noise_var),
                                             C.byref(out), ptr(stream)))

    def demod_frames_csi(self, d_iq, n_frames, frame_stride, frame_len, d_eq, d_llr=None, d_sigma2=None, d_n_used=None,
                         noise_mode=CSI_NOISE_EST, noise_var=0.0, d_bits=None, bits_mode=BITS_NONE, d_tsr=None, stream=None) -> int:
        """demod_frames, then csi_frames(CSI_ROWS_ALL) and demap_csi_frames over d_eq with one segment per frame (n_dsym rows of
        Kd symbols, the handle's rho and modulation).  Returns n_dsym."""
        out = self._csi_out(d_llr, d_sigma2, d_n_used)
        return int(check(self.lib.ofdm_rx_demod_frames_csi(self._h, ptr(d_iq), int(n_frames), int(frame_stride), int(frame_len),
                                                           ptr(d_eq), ptr(d_bits), int(bits_mode), ptr(d_tsr), int(noise_mode),
                                                           float(noise_var), C.byref(out), ptr(stream))))

    # ---- DFT-spread OFDM (SC-FDMA): despreading behind the equaliser (include/ofdm_mi355x.h, "DFT-spread OFDM") ----------------
    @staticmethod
    def _despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight):
        return _lib.DespreadOut(_addr(d_sym_out), _addr(d_llr), _addr(d_bits), _addr(d_beta), _addr(d_weight))

    def reserve_despread(self, M: int, n_seg: int = 0):
        """ofdm_rx_reserve_despread: the plan for M and the tables of n_seg segments (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_despread(self._h, int(M), int(n_seg)))

    def dft_despread_frames(self, d_sym, n_seg, rows, M, seg_stride, d_csi, csi_stride, rho, modulation, d_sym_out=None, d_llr=None,
                            d_bits=None, bits_mode=BITS_NONE, d_beta=None, d_weight=None, noise_mode=_lib.DESPREAD_NOISE_RHO,
                            noise_var=0.0, d_sigma2=None, stream=None):
        """ofdm_dft_despread_frames: segment s = `rows` rows of M equalised complex64 symbols at d_sym + s*seg_stride, entry k of
        every row with the channel power d_csi[s*csi_stride + k] (d_csi None: the plain inverse transform).  Outputs sym
        [n_seg][rows*M] complex64 (may be d_sym), llr [n_seg][rows*M*bps] (positive favours bit 0), hard bits, beta and weight
        [n_seg] float32."""
        out = self._despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight)
        check(self.lib.ofdm_dft_despread_frames(self._h, ptr(d_sym), int(n_seg), int(rows), int(M), int(seg_stride), ptr(d_csi),
                                                int(csi_stride), float(rho), _mod_bits(modulation), int(noise_mode), float(noise_var),
                                                ptr(d_sigma2), int(bits_mode), C.byref(out), ptr(stream)))

    def demod_frames_despread(self, d_iq, n_frames, frame_stride, frame_len, d_eq, d_sym_out=None, d_llr=None, d_bits=None,
                              bits_mode=BITS_NONE, d_beta=None, d_weight=None, noise_mode=_lib.DESPREAD_NOISE_RHO, noise_var=0.0,
                              d_sigma2=None, d_tsr=None, stream=None) -> int:
        """demod_frames, then csi_frames(CSI_ROWS_ALL) into the workspace and dft_despread_frames over d_eq with one segment per
        frame (n_dsym rows of M = Kd symbols, the handle's rho and modulation).  Returns n_dsym."""
        out = self._despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight)
        return int(check(self.lib.ofdm_rx_demod_frames_despread(self._h, ptr(d_iq), int(n_frames), int(frame_stride), int(frame_len),
                                                                ptr(d_eq), ptr(d_tsr), int(noise_mode), float(noise_var),
                                                                ptr(d_sigma2), int(bits_mode), C.byref(out), ptr(stream))))

    # ---- multi-user allocations of DFT-spread OFDM (include/ofdm_mi355x.h, "multi-user allocations of DFT-spread OFDM") ---------
    def set_allocations(self, allocs):
        """ofdm_rx_set_allocations: a list of (start, M, bits per symbol), at most 32, not overlapping; () clears the set."""
        n, start, M, mod = _alloc_arrays([(a[0], a[1], _mod_bits(a[2])) for a in allocs], 3)
        check(self.lib.ofdm_rx_set_allocations(self._h, n, ptr(start) if n else None, ptr(M) if n else None, ptr(mod) if n else None))

    def reserve_despread_alloc(self, n_seg: int = 0):
        """ofdm_rx_reserve_despread_alloc: the tables of n_seg segments for the set in force (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_despread_alloc(self._h, int(n_seg)))

    def dft_despread_alloc_frames(self, d_sym, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, d_sym_out=None, d_llr=None,
                                  d_bits=None, bits_mode=BITS_NONE, d_beta=None, d_weight=None, noise_mode=_lib.DESPREAD_NOISE_RHO,
                                  noise_var=0.0, d_sigma2=None, stream=None):
        """ofdm_dft_despread_alloc_frames: every allocation of the set despread in one pass over rows of row_len symbols.  The
        outputs are allocation-major and dense (alloc_layout); beta and weight are [n_alloc][n_seg]."""
        out = self._despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight)
        check(self.lib.ofdm_dft_despread_alloc_frames(self._h, ptr(d_sym), int(n_seg), int(rows), int(row_len), int(seg_stride),
                                                      ptr(d_csi), int(csi_stride), float(rho), int(noise_mode), float(noise_var),
                                                      ptr(d_sigma2), int(bits_mode), C.byref(out), ptr(stream)))

    def demod_frames_despread_alloc(self, d_iq, n_frames, frame_stride, frame_len, d_eq, d_sym_out=None, d_llr=None, d_bits=None,
                                    bits_mode=BITS_NONE, d_beta=None, d_weight=None, noise_mode=_lib.DESPREAD_NOISE_RHO,
                                    noise_var=0.0, d_sigma2=None, d_tsr=None, stream=None) -> int:
        """demod_frames, then csi_frames(CSI_ROWS_ALL) into the workspace and dft_despread_alloc_frames over d_eq with one segment
        per frame (n_dsym rows of row_len = Kd symbols, the handle's rho).  Returns n_dsym."""
        out = self._despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight)
        return int(check(self.lib.ofdm_rx_demod_frames_despread_alloc(self._h, ptr(d_iq), int(n_frames), int(frame_stride),
                                                                      int(frame_len), ptr(d_eq), ptr(d_tsr), int(noise_mode),
                                                                      float(noise_var), ptr(d_sigma2), int(bits_mode), C.byref(out),
                                                                      ptr(stream))))

    # ---- receive-diversity combining: B branches added with maximum-ratio weights, LLRs of the sum (include/ofdm_mi355x.h) ------
    @staticmethod
    def _mrc_out(d_llr, d_sym_out, d_weight):
        return _lib.MrcOut(_addr(d_llr), _addr(d_sym_out), _addr(d_weight))

    @staticmethod
    def _mrc_noise(who, n_branch, noise_var, d_sigma2=None, other=MRC_NOISE_SEG):
        """(noise_mode, host array) of the combiners: OFDM_MRC_NOISE_GIVEN with the n_branch doubles of noise_var, or `other` with
        None.  who: the method whose caller gives exactly one of noise_var and d_sigma2 (None: noise_var alone decides)."""
        if who and (noise_var is None) == (d_sigma2 is None):
            raise ValueError("%s: give exactly one of noise_var and d_sigma2" % who)
        if noise_var is None:
            return other, None
        nv = [float(v) for v in noise_var]
        if len(nv) != int(n_branch):
            raise ValueError("noise_var must hold n_branch = %d numbers, got %d" % (int(n_branch), len(nv)))
        return MRC_NOISE_GIVEN, (C.c_double * len(nv))(*nv)

    def reserve_mrc(self, n_branch: int, n_seg: int, rows: int, row_len: int):
        """Workspace of combine_csi_frames / demod_frames_mrc for n_branch branches of n_seg segments of `rows` rows of row_len
        symbols (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_mrc(self._h, int(n_branch), int(n_seg), int(rows), int(row_len)))

    def combine_csi_frames(self, d_sym, n_branch, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, modulation,
                           noise_var=None, d_sigma2=None, d_llr=None, d_sym_out=None, d_weight=None, stream=None):
        """ofdm_combine_csi_frames: branch b of segment s is the unit g = b*n_seg + s, `rows` rows of row_len complex64 symbols at
        d_sym + g*seg_stride with the channel powers d_csi[g*csi_stride + j].  Exactly one of noise_var (n_branch numbers, one
        variance per branch) and d_sigma2 (device, [n_branch*n_seg] float64, one per unit) is given.  Outputs per segment: llr
        [rows*row_len*bps] float32 (positive favours bit 0), sym [rows*row_len] complex64, weight [rows*row_len] float32."""
        mode, nv = self._mrc_noise("combine_csi_frames", n_branch, noise_var, d_sigma2)
        out = self._mrc_out(d_llr, d_sym_out, d_weight)
        check(self.lib.ofdm_combine_csi_frames(self._h, ptr(d_sym), int(n_branch), int(n_seg), int(rows), int(row_len),
                                               int(seg_stride), ptr(d_csi), int(csi_stride), float(rho), _mod_bits(modulation),
                                               mode, nv, ptr(d_sigma2), C.byref(out),
                                               ptr(stream)))

    def demod_frames_mrc(self, d_iq, n_branch, n_frames, frame_stride, frame_len, d_eq, noise_var=None, d_llr=None, d_sym_out=None,
                         d_weight=None, d_sigma2=None, d_tsr=None, stream=None) -> int:
        """demod_frames over the n_branch*n_frames frames of d_iq (frame f of branch b at index b*n_frames + f), then
        csi_frames(CSI_ROWS_ALL) and combine_csi_frames over d_eq with one segment per frame (n_dsym rows of Kd symbols, the
        handle's rho and modulation).  noise_var: n_branch numbers, or None for the per-frame estimate of demod_frames_csi.
        d_sigma2 [n_branch*n_frames] float64 receives the variances used.  Returns n_dsym."""
        mode, nv = self._mrc_noise(None, n_branch, noise_var, other=MRC_NOISE_EST)
        out = self._mrc_out(d_llr, d_sym_out, d_weight)
        return int(check(self.lib.ofdm_rx_demod_frames_mrc(self._h, ptr(d_iq), int(n_branch), int(n_frames), int(frame_stride),
                                                           int(frame_len), ptr(d_eq), ptr(d_tsr),
                                                           mode, nv, C.byref(out),
                                                           ptr(d_sigma2), ptr(stream))))

    # ---- receive diversity for DFT-spread OFDM: B branches combined per bin, then despread (include/ofdm_mi355x.h) ---------------
    @staticmethod
    def _mrc_despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight, d_comb):
        return _lib.MrcDespreadOut(_addr(d_sym_out), _addr(d_llr), _addr(d_bits), _addr(d_beta), _addr(d_weight), _addr(d_comb))

    def reserve_mrc_despread(self, M: int, n_branch: int, n_seg: int = 0):
        """ofdm_rx_reserve_mrc_despread: the plan for M, the table of n_branch*n_seg units and the |H|^2 rows of
        demod_frames_mrc_despread for as many frames (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_mrc_despread(self._h, int(M), int(n_branch), int(n_seg)))

    def combine_despread_frames(self, d_sym, n_branch, n_seg, rows, M, seg_stride, d_csi, csi_stride, rho, modulation,
                                noise_var=None, d_sigma2=None, d_sym_out=None, d_llr=None, d_bits=None, bits_mode=BITS_NONE,
                                d_beta=None, d_weight=None, d_comb=None, stream=None):
        """ofdm_combine_despread_frames: branch b of segment s is the unit g = b*n_seg + s, `rows` rows of M equalised complex64
        symbols at d_sym + g*seg_stride with the channel powers d_csi[g*csi_stride + k].  Exactly one of noise_var (n_branch
        numbers, one variance per branch) and d_sigma2 (device, [n_branch*n_seg] float64, one per unit) is given; their absolute
        level matters.  Outputs per segment: sym [rows*M] complex64, llr [rows*M*bps] float32 (positive favours bit 0), hard
        bits, beta and weight [rows] float32 (one per ROW), comb [rows*M] complex64 (the combined symbols before the transform)."""
        mode, nv = self._mrc_noise("combine_despread_frames", n_branch, noise_var, d_sigma2)
        out = self._mrc_despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight, d_comb)
        check(self.lib.ofdm_combine_despread_frames(self._h, ptr(d_sym), int(n_branch), int(n_seg), int(rows), int(M),
                                                    int(seg_stride), ptr(d_csi), int(csi_stride), float(rho), _mod_bits(modulation),
                                                    mode, nv, ptr(d_sigma2), int(bits_mode),
                                                    C.byref(out), ptr(stream)))

    def demod_frames_mrc_despread(self, d_iq, n_branch, n_frames, frame_stride, frame_len, d_eq, noise_var=None, d_sigma2=None,
                                  d_sym_out=None, d_llr=None, d_bits=None, bits_mode=BITS_NONE, d_beta=None, d_weight=None,
                                  d_comb=None, d_tsr=None, stream=None) -> int:
        """demod_frames over the n_branch*n_frames frames of d_iq (frame f of branch b at index b*n_frames + f), then
        csi_frames(CSI_ROWS_ALL) into the workspace and combine_despread_frames over d_eq with one segment per frame (n_dsym rows
        of M = Kd symbols, the handle's rho and modulation).  Exactly one of noise_var (n_branch numbers) and d_sigma2 (device,
        [n_branch*n_frames] float64).  Returns n_dsym."""
        mode, nv = self._mrc_noise("demod_frames_mrc_despread", n_branch, noise_var, d_sigma2)
        out = self._mrc_despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight, d_comb)
        return int(check(self.lib.ofdm_rx_demod_frames_mrc_despread(self._h, ptr(d_iq), int(n_branch), int(n_frames),
                                                                    int(frame_stride), int(frame_len), ptr(d_eq), ptr(d_tsr),
                                                                    mode, nv, ptr(d_sigma2),
                                                                    int(bits_mode), C.byref(out), ptr(stream))))

    # ---- receive diversity for multi-user allocations of DFT-spread OFDM (include/ofdm_mi355x.h) ---------------------------------
    def reserve_mrc_despread_alloc(self, n_branch: int, n_seg: int = 0, row_len: int = 0):
        """ofdm_rx_reserve_mrc_despread_alloc: the table of n_branch*n_seg units of row_len entries and the |H|^2 rows of
        demod_frames_mrc_despread_alloc for as many frames (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_mrc_despread_alloc(self._h, int(n_branch), int(n_seg), int(row_len)))

    def combine_despread_alloc_frames(self, d_sym, n_branch, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, noise_var=None,
                                      d_sigma2=None, d_sym_out=None, d_llr=None, d_bits=None, bits_mode=BITS_NONE, d_beta=None,
                                      d_weight=None, d_comb=None, stream=None):
        """ofdm_combine_despread_alloc_frames: combine_despread_frames for every allocation of the set (set_allocations) in one
        pass over rows of row_len symbols: unit g = b*n_seg + s is `rows` rows at d_sym + g*seg_stride with the channel powers
        d_csi[g*csi_stride + k].  Exactly one of noise_var (n_branch numbers) and d_sigma2 (device, [n_branch*n_seg] float64).
        sym, comb, llr and bits are allocation-major and dense (alloc_layout; comb at the sym offsets); beta and weight are
        [n_alloc][n_seg][rows]."""
        mode, nv = self._mrc_noise("combine_despread_alloc_frames", n_branch, noise_var, d_sigma2)
        out = self._mrc_despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight, d_comb)
        check(self.lib.ofdm_combine_despread_alloc_frames(self._h, ptr(d_sym), int(n_branch), int(n_seg), int(rows), int(row_len),
                                                          int(seg_stride), ptr(d_csi), int(csi_stride), float(rho),
                                                          mode, nv, ptr(d_sigma2),
                                                          int(bits_mode), C.byref(out), ptr(stream)))

    def demod_frames_mrc_despread_alloc(self, d_iq, n_branch, n_frames, frame_stride, frame_len, d_eq, noise_var=None, d_sigma2=None,
                                        d_sym_out=None, d_llr=None, d_bits=None, bits_mode=BITS_NONE, d_beta=None, d_weight=None,
                                        d_comb=None, d_tsr=None, stream=None) -> int:
        """demod_frames over the n_branch*n_frames frames of d_iq (frame f of branch b at index b*n_frames + f), then
        csi_frames(CSI_ROWS_ALL) into the workspace and combine_despread_alloc_frames over d_eq with one segment per frame (n_dsym
        rows of row_len = Kd symbols, the handle's rho).  Exactly one of noise_var (n_branch numbers) and d_sigma2 (device,
        [n_branch*n_frames] float64).  Returns n_dsym."""
        mode, nv = self._mrc_noise("demod_frames_mrc_despread_alloc", n_branch, noise_var, d_sigma2)
        out = self._mrc_despread_out(d_sym_out, d_llr, d_bits, d_beta, d_weight, d_comb)
        return int(check(self.lib.ofdm_rx_demod_frames_mrc_despread_alloc(self._h, ptr(d_iq), int(n_branch), int(n_frames),
                                                                          int(frame_stride), int(frame_len), ptr(d_eq), ptr(d_tsr),
                                                                          mode, nv,
                                                                          ptr(d_sigma2), int(bits_mode), C.byref(out), ptr(stream))))

    # ---- delay-window denoising of the LS channel estimate (include/ofdm_mi355x.h) ----------------------------------------------
    def set_chan_window(self, pre: int, post: int):
        """ofdm_rx_set_chan_window: while (pre, post) != (0, 0), demod_frames -- and every demod_frames_* call -- refines its
        channel estimates by keeping the taps [0, post) and [nfft - pre, nfft) of their inverse FFT.  (0, 0) switches it off."""
        check(self.lib.ofdm_rx_set_chan_window(self._h, int(pre), int(post)))

    def chan_window_frames(self, d_H_in, d_tsr, n_rows, pre, post, d_H_out, d_gain_out=None, d_tail=None, stream=None):
        """ofdm_chan_window_frames: the stage on n_rows rows of nfft complex64 at d_H_in with d_tsr [n_rows][4] int32.  Outputs
        H' [n_rows][nfft] complex64 (may be d_H_in), gain [n_rows][Kd] complex64, tail [n_rows] float32."""
        check(self.lib.ofdm_chan_window_frames(self._h, ptr(d_H_in), ptr(d_tsr), int(n_rows), int(pre), int(post), ptr(d_H_out),
                                               ptr(d_gain_out), ptr(d_tail), ptr(stream)))

    def chan_noise_frames(self, n_frames, d_sigma2, stream=None):
        """ofdm_rx_chan_noise_frames: d_sigma2[f] (float64) = the tail power of frame f of the last demod_frames call, the per-unit
        variances combine_csi_frames takes as d_sigma2."""
        check(self.lib.ofdm_rx_chan_noise_frames(self._h, int(n_frames), ptr(d_sigma2), ptr(stream)))

    # ---- channel estimate averaged over every sync symbol of a frame (include/ofdm_mi355x.h) ------------------------------------
    CHANAVG_CHUNK = 16               # OFDM_CHANAVG_CHUNK: consecutive patterns whose sums one work item forms

    def set_chan_average(self, n_avg: int):
        """ofdm_rx_set_chan_average: while n_avg != 0, demod_frames -- and every demod_frames_* call -- replaces its channel
        estimates by the phase-aligned mean of the LS estimates of the first n_avg sync symbols of each frame (-1 = all of them),
        ahead of the delay window.  0 switches it off.  Needs synch_dat[0] == 1."""
        check(self.lib.ofdm_rx_set_chan_average(self._h, int(n_avg)))

    def reserve_chan_average(self, n_frames: int, frame_len: int):
        """ofdm_rx_reserve_chan_average: workspace for averaging n_frames frames of frame_len samples (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_chan_average(self._h, int(n_frames), int(frame_len)))

    def chan_average_frames(self, d_iq, n_frames, frame_stride, frame_len, d_tsr, n_avg, d_H_out=None, d_gain_out=None,
                            d_spread=None, d_n_used=None, d_rot=None, stream=None):
        """ofdm_chan_average_frames: the stage on any device IQ buffer with d_tsr [n_frames][4] int32.  Outputs, each optional but
        not all: Hbar [n_frames][nfft] complex64, gain [n_frames][Kd] complex64, spread [n_frames] float32, n_used [n_frames]
        int32, rot [n_frames][P] complex64 with P = min(n_avg, patterns per frame)."""
        check(self.lib.ofdm_chan_average_frames(self._h, ptr(d_iq), int(n_frames), int(frame_stride), int(frame_len), ptr(d_tsr),
                                                int(n_avg), ptr(d_H_out), ptr(d_gain_out), ptr(d_spread), ptr(d_n_used), ptr(d_rot),
                                                ptr(stream)))

    def chan_spread_frames(self, n_frames, d_sigma2, stream=None):
        """ofdm_rx_chan_spread_frames: d_sigma2[f] (float64) = the spread of frame f of the last demod_frames call, the per-unit
        variances combine_csi_frames takes as d_sigma2."""
        check(self.lib.ofdm_rx_chan_spread_frames(self._h, int(n_frames), ptr(d_sigma2), ptr(stream)))

    # ---- channel tracked across the sync symbols of a frame (include/ofdm_mi355x.h) ---------------------------------------------
    TRACK_HOLD, TRACK_LINEAR = _lib.TRACK_HOLD, _lib.TRACK_LINEAR

    @staticmethod
    def _track_out(d_eq, d_bits, d_csi, d_H_pat, d_takes):
        return _lib.TrackOut(_addr(d_eq), _addr(d_bits), _addr(d_csi), _addr(d_H_pat), _addr(d_takes))

    def reserve_chan_track(self, n_frames: int, frame_len: int):
        """ofdm_rx_reserve_chan_track: workspace for tracking n_frames frames of frame_len samples (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_chan_track(self._h, int(n_frames), int(frame_len)))

    def chan_track_frames(self, d_iq, n_frames, frame_stride, frame_len, d_tsr, mode=_lib.TRACK_LINEAR, pre=0, post=0, d_eq=None,
                          d_bits=None, bits_mode=BITS_NONE, d_csi=None, d_H_pat=None, d_takes=None, stream=None) -> int:
        """ofdm_chan_track_frames: one LS estimate per sync symbol of every frame and every data symbol equalised with the estimate
        interpolated (TRACK_LINEAR) or held (TRACK_HOLD) between them; (pre, post) != (0, 0) denoises every estimate with the
        delay window.  Outputs per frame, each optional but not all: eq [n_dsym][Kd] complex64, its hard bits, csi [n_dsym][Kd]
        float32, H_pat [n_pat][nfft] complex64, takes [n_pat] int32.  Returns n_dsym."""
        out = self._track_out(d_eq, d_bits, d_csi, d_H_pat, d_takes)
        return int(check(self.lib.ofdm_chan_track_frames(self._h, ptr(d_iq), int(n_frames), int(frame_stride), int(frame_len),
                                                         ptr(d_tsr), int(mode), int(pre), int(post), int(bits_mode), C.byref(out),
                                                         ptr(stream))))

    def demod_frames_track(self, d_iq, n_frames, frame_stride, frame_len, mode=_lib.TRACK_LINEAR, d_eq=None, d_bits=None,
                           bits_mode=BITS_NONE, d_csi=None, d_H_pat=None, d_takes=None, d_tsr=None, stream=None) -> int:
        """ofdm_rx_demod_frames_track: the sync search of demod_frames, then chan_track_frames with the window of set_chan_window.
        The averaging setting is not applied.  Returns n_dsym."""
        out = self._track_out(d_eq, d_bits, d_csi, d_H_pat, d_takes)
        return int(check(self.lib.ofdm_rx_demod_frames_track(self._h, ptr(d_iq), int(n_frames), int(frame_stride), int(frame_len),
                                                             int(mode), int(bits_mode), ptr(d_tsr), C.byref(out), ptr(stream))))

    # ---- LTE tail-biting convolutional code: the decoder behind d_llr of demap_frames / demod_frames_soft / demod_frames_pilots ----
    def reserve_tbcc(self, n_blocks: int, K: int):
        """Prepares decoding of up to n_blocks code blocks of K bits per call (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_tbcc(self._h, int(n_blocks), int(K)))

    def tbcc_decode_frames(self, d_llr, n_seg, seg_stride, blocks_per_seg, K, d_bits=None, bits_mode=BITS_UNPACKED, d_metric=None,
                           d_tb_ok=None, stream=None):
        """ofdm_tbcc_decode_frames: block (s, b) = the 3K float32 LLRs at d_llr + s*seg_stride + b*3K (seg_stride in floats).
        Outputs dense per block: bits [K] (one per byte, or packed MSB-first), metric float32, tb_ok int32."""
        out = _lib.TbccOut(_addr(d_bits), int(bits_mode), _addr(d_metric), _addr(d_tb_ok))
        check(self.lib.ofdm_tbcc_decode_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(blocks_per_seg), int(K),
                                               C.byref(out), ptr(stream)))

    # ---- the same code behind the rate matching of TS 36.212 5.1.4.2: E LLRs per block in place of 3K ----
    def tbcc_rate_dematch_frames(self, d_llr, n_seg, seg_stride, blocks_per_seg, K, E, d_out, out_stride, stream=None):
        """ofdm_tbcc_rate_dematch_frames: block (s, b) = the E float32 LLRs at d_llr + s*seg_stride + b*E -> its 3K de-matched
        LLRs at d_out + s*out_stride + b*3K, the layout tbcc_decode_frames reads (strides in floats)."""
        check(self.lib.ofdm_tbcc_rate_dematch_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(blocks_per_seg), int(K),
                                                     int(E), ptr(d_out), int(out_stride), ptr(stream)))

    def tbcc_decode_rm_frames(self, d_llr, n_seg, seg_stride, blocks_per_seg, K, E, d_bits=None, bits_mode=BITS_UNPACKED,
                              d_metric=None, d_tb_ok=None, stream=None):
        """ofdm_tbcc_decode_rm_frames: tbcc_decode_frames on rate-matched LLRs (block (s, b) = E floats at d_llr + s*seg_stride +
        b*E), de-matched inside the decoder's launch.  reserve_tbcc prepares this call too."""
        out = _lib.TbccOut(_addr(d_bits), int(bits_mode), _addr(d_metric), _addr(d_tb_ok))
        check(self.lib.ofdm_tbcc_decode_rm_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(blocks_per_seg), int(K),
                                                  int(E), C.byref(out), ptr(stream)))

    # ---- LTE turbo code (TS 36.212 5.1.3.2): the iterative max-log-MAP decoder behind the same LLR buffers ----
    def reserve_turbo(self, n_blocks: int, K: int):
        """Sizes the decoder's workspace for up to n_blocks code blocks of K bits per call (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_turbo(self._h, int(n_blocks), int(K)))

    def turbo_decode_frames(self, d_llr, n_seg, seg_stride, blocks_per_seg, K, f1, f2, n_iter, d_bits=None, bits_mode=BITS_UNPACKED,
                            d_llr_out=None, stream=None):
        """ofdm_turbo_decode_frames: block (s, b) = the 3K + 12 float32 LLRs at d_llr + s*seg_stride + b*(3K + 12) (seg_stride in
        floats), QPP interleaver (f1, f2), n_iter iterations.  Outputs dense per block: bits [K] (one per byte, or packed
        MSB-first), a-posteriori llr [K] float32."""
        out = _lib.TurboOut(_addr(d_bits), int(bits_mode), _addr(d_llr_out))
        check(self.lib.ofdm_turbo_decode_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(blocks_per_seg), int(K),
                                                int(f1), int(f2), int(n_iter), C.byref(out), ptr(stream)))

    def reserve_turbo_es(self, n_blocks: int, K: int):
        """reserve_turbo for turbo_decode_es_frames (a second K-float array per block)."""
        check(self.lib.ofdm_rx_reserve_turbo_es(self._h, int(n_blocks), int(K)))

    def turbo_decode_es_frames(self, d_llr, n_seg, seg_stride, blocks_per_seg, K, f1, f2, crc_kind, min_iter, max_iter, d_bits=None,
                               bits_mode=BITS_UNPACKED, d_llr_out=None, d_iters=None, d_crc_ok=None, stat_stride=0, stream=None):
        """ofdm_turbo_decode_es_frames: turbo_decode_frames with early termination -- from min_iter on a block stops after the
        first iteration whose hard decisions are divisible by the generator of crc_kind (all K bits, zero mask), at max_iter
        otherwise; its bits and llr are those of turbo_decode_frames at that n_iter.  iters / crc_ok: uint8 per block at
        s*stat_stride + b (0 = blocks_per_seg)."""
        out = _lib.TurboEsOut(_addr(d_bits), int(bits_mode), _addr(d_llr_out), _addr(d_iters), _addr(d_crc_ok), int(stat_stride))
        check(self.lib.ofdm_turbo_decode_es_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(blocks_per_seg), int(K),
                                                   int(f1), int(f2), int(crc_kind), int(min_iter), int(max_iter), C.byref(out),
                                                   ptr(stream)))

    def reserve_turbo_rm(self):
        """Loads the turbo rate-matching kernels (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_turbo_rm(self._h))

    def turbo_rate_dematch_frames(self, d_llr, n_seg, seg_stride, blocks_per_seg, K, E, d_out, out_stride, Ncb=0, rv=0, d_rv=None,
                                  accumulate=False, stream=None):
        """ofdm_turbo_rate_dematch_frames: block (s, b) = the E float32 LLRs at d_llr + s*seg_stride + b*E -> its 3K + 12
        de-matched LLRs at d_out + s*out_stride + b*(3K + 12), what turbo_decode_frames reads; redundancy version rv (or d_rv, one
        device int32 per segment), buffer length Ncb (0 = all of it).  accumulate adds into the floats already there (HARQ)."""
        check(self.lib.ofdm_turbo_rate_dematch_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(blocks_per_seg), int(K),
                                                      int(E), int(Ncb), int(rv), ptr(d_rv), int(bool(accumulate)), ptr(d_out),
                                                      int(out_stride), ptr(stream)))

    # ---- transport-block layer (TS 36.212 5.1.1, 5.1.2, 5.1.5): de-match per group, decode per K, desegment ----
    def reserve_tb(self, n_tb: int, A: int, Z: int = 0):
        """Sizes the workspaces (this layer's and the turbo decoder's) for n_tb transport blocks of A bits per call and loads
        the kernels (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_tb(self._h, int(n_tb), int(A), int(Z)))

    def tb_decode_frames(self, d_llr, n_tb, llr_stride, A, G, qpp_plus, d_soft, soft_stride, n_iter, qpp_minus=(0, 0), Z=0, q=1,
                         N_IR=0, rv=0, d_rv=None, accumulate=False, d_payload=None, payload_mode=BITS_UNPACKED, d_tb_ok=None,
                         d_cb_ok=None, d_syndrome=None, stream=None):
        """ofdm_tb_decode_frames: the G LLRs of transport block t at d_llr + t*llr_stride -> its HARQ soft buffer at
        d_soft + t*soft_stride (written, or added to with accumulate) -> payload [n_tb][A], tb_ok [n_tb], cb_ok [n_tb][C],
        syndrome [n_tb] (each only where given).  qpp_plus / qpp_minus: (f1, f2) for K+ and K- of tb_geometry(A, Z)."""
        out = _lib.TbOut(_addr(d_payload), int(payload_mode), _addr(d_tb_ok), _addr(d_cb_ok), _addr(d_syndrome))
        check(self.lib.ofdm_tb_decode_frames(self._h, ptr(d_llr), int(n_tb), int(llr_stride), int(A), int(Z), int(G), int(q), int(N_IR),
                                             int(qpp_minus[0]), int(qpp_minus[1]), int(qpp_plus[0]), int(qpp_plus[1]), int(rv), ptr(d_rv),
                                             int(n_iter), int(bool(accumulate)), ptr(d_soft), int(soft_stride), C.byref(out), ptr(stream)))

    def reserve_tb_es(self, n_tb: int, A: int, Z: int = 0):
        """reserve_tb for tb_decode_es_frames (the larger decoder workspace)."""
        check(self.lib.ofdm_rx_reserve_tb_es(self._h, int(n_tb), int(A), int(Z)))

    def tb_decode_es_frames(self, d_llr, n_tb, llr_stride, A, G, qpp_plus, d_soft, soft_stride, min_iter, max_iter, qpp_minus=(0, 0),
                            Z=0, q=1, N_IR=0, rv=0, d_rv=None, accumulate=False, d_payload=None, payload_mode=BITS_UNPACKED,
                            d_tb_ok=None, d_cb_ok=None, d_syndrome=None, d_cb_iters=None, stream=None):
        """ofdm_tb_decode_es_frames: tb_decode_frames with every code block stopped at its first passing CRC (CRC24B, or the
        transport block's CRC24A when C = 1) between min_iter and max_iter; cb_iters [n_tb][C] uint8 = the iterations it ran."""
        out = _lib.TbEsOut(_addr(d_payload), int(payload_mode), _addr(d_tb_ok), _addr(d_cb_ok), _addr(d_syndrome), _addr(d_cb_iters))
        check(self.lib.ofdm_tb_decode_es_frames(self._h, ptr(d_llr), int(n_tb), int(llr_stride), int(A), int(Z), int(G), int(q),
                                                int(N_IR), int(qpp_minus[0]), int(qpp_minus[1]), int(qpp_plus[0]), int(qpp_plus[1]),
                                                int(rv), ptr(d_rv), int(min_iter), int(max_iter), int(bool(accumulate)), ptr(d_soft),
                                                int(soft_stride), C.byref(out), ptr(stream)))

    # ---- Gold-sequence descrambling in front of the decoder, CRC check behind it (TS 36.211 7.2, TS 36.212 5.1.1) ----
    def reserve_bitproc(self):
        """Loads the descrambling and CRC kernels (before a graph capture)."""
        check(self.lib.ofdm_rx_reserve_bitproc(self._h))

    def descramble_llr_frames(self, d_llr, n_seg, seg_stride, seg_bits, d_cinit, d_out, out_stride=None, stream=None):
        """ofdm_descramble_llr_frames: the sign bit of float n of segment s is XORed with c(n) of c_init = d_cinit[s] (device
        uint32); strides in floats, d_out may be d_llr at the same stride."""
        check(self.lib.ofdm_descramble_llr_frames(self._h, ptr(d_llr), int(n_seg), int(seg_stride), int(seg_bits), ptr(d_cinit),
                                                  ptr(d_out), int(seg_stride if out_stride is None else out_stride), ptr(stream)))

    def crc_check_frames(self, d_info, n_blocks, A, kind, mask=0, d_mask=None, info_mode=BITS_UNPACKED, d_ok=None, d_syndrome=None,
                         d_payload=None, payload_mode=BITS_UNPACKED, stream=None):
        """ofdm_crc_check_frames: d_info dense [n_blocks][A + L] bits as the decoders write them -> ok uint8 (syndrome == mask),
        syndrome uint32 (CRC of the first A bits ^ the received parity), payload dense [n_blocks][A]; mask: the scalar, or
        d_mask one device uint32 per block."""
        out = _lib.CrcOut(_addr(d_ok), _addr(d_syndrome), _addr(d_payload), int(payload_mode))
        check(self.lib.ofdm_crc_check_frames(self._h, ptr(d_info), int(info_mode), int(n_blocks), int(A), int(kind), int(mask),
                                             ptr(d_mask), C.byref(out), ptr(stream)))


class FoEngine(_Handle):
    """CFO-search receiver handle (reference: LEGACY/gr-ofdm-rx/python/SynchEstAndFO.py): trial x candidate sync table,
    up to 100 syncs per call, one equalised data symbol per sync."""
    _destroy = "ofdm_fo_destroy"

    def __init__(self, num_ofdm_symb, nfft, cp_len, num_synch_bins, synch_dat, num_data_bins, snr, rotators, device=0,
                 spread_code=None):
        """rotators: [len(fo_range)][nfft] candidate rotators, or None = no carrier-offset stage (gr-RXOFDM table mode).
        spread_code: None = SynchEstAndFO; a complex sequence of length DSSS = SynchEstFOAndDSSS (despread output)."""
        self.lib = _lib.load()
        rot = None if rotators is None else np.ascontiguousarray(rotators, dtype=np.complex64)
        if rot is not None and (rot.ndim != 2 or rot.shape[1] != int(nfft) or rot.shape[0] < 1):
            raise ValueError("rotators must be [len(fo_range) >= 1][nfft]")
        code = None if spread_code is None else np.ascontiguousarray(spread_code, dtype=np.complex64).ravel()
        self.dsss = 0 if code is None else int(code.size)
        self.n_spread = int(num_data_bins) // self.dsss if self.dsss else 0
        self.cfg = _lib.FoCfg(int(num_ofdm_symb), int(nfft), int(cp_len), int(num_synch_bins), int(synch_dat[0]),
                              int(synch_dat[1]), int(num_data_bins), 1 if rot is None else int(rot.shape[0]), float(snr),
                              None if rot is None else rot.ctypes.data, int(device), self.dsss,
                              None if code is None else code.ctypes.data)
        h = C.c_void_p()
        check(self.lib.ofdm_fo_create(C.byref(self.cfg), C.byref(h)))
        self.cfg.rotators = None          # the library copied the tables
        self.cfg.spread_code = None
        self._h = h
        self.report = _lib.FoReport()

    def work(self, in0: np.ndarray, out: np.ndarray) -> int:
        """Raw status (see RxEngine.work)."""
        return _work(self.lib.ofdm_fo_work, self._h, self.report, in0, out)

    def state(self):
        c = self.cfg
        R = _lib.FO_MAX_SYNC
        mm = c.synch_S * c.num_synch_bins
        tsr = np.zeros((R, 3), np.float64)
        H = np.zeros((R, c.nfft), np.complex64)
        ht = np.zeros((R, c.nfft), np.complex64)
        esf = np.zeros((R, mm), np.complex64)
        edf = np.zeros((R, c.num_data_bins), np.complex64)
        eqg = np.zeros(c.num_synch_bins, np.complex64)
        check(self.lib.ofdm_fo_get_state(self._h, ptr(tsr), ptr(H), ptr(ht), ptr(esf), ptr(edf), ptr(eqg)))
        return dict(time_synch_ref=tsr, chan_freq=H, chan_time=ht, synch_freq=esf, data_freq=edf, eq_gain=eqg)

    def despread(self):
        out = np.zeros((_lib.FO_MAX_SYNC, self.n_spread), np.complex64)
        check(self.lib.ofdm_fo_get_despread(self._h, ptr(out)))
        return out

    # ---- frame batches on device buffers (each frame: first work() call of a fresh instance) ----------------------
    def reserve(self, n_frames: int, frame_len: int):
        check(self.lib.ofdm_fo_reserve(self._h, int(n_frames), int(frame_len)))

    def demod_frames(self, d_iq, n_frames, frame_stride, frame_len, d_status, d_tsr=None, d_fo_idx=None, d_data_freq=None,
                     d_bits=None, bits_mode=BITS_NONE, d_data_freq_d=None, d_chan_freq=None, d_chan_time=None,
                     d_synch_freq=None, stream=None) -> int:
        """ofdm_fo_demod_frames on device buffers; returns the rows per frame (FO_MAX_SYNC).  Per frame: status = n_sync or
        OFDM_ERR_INDEX (a 101st sync), tsr [100][3] int32, fo_idx int32, data_freq [100][Kd] complex64, bits, data_freq_d
        [100][Kd/DSSS], chan_freq / chan_time [100][nfft], synch_freq [100][S*Ks]; rows >= n_sync are zero."""
        out = _lib.FoBatchOut(_addr(d_status), _addr(d_tsr), _addr(d_fo_idx), _addr(d_data_freq), _addr(d_bits), int(bits_mode),
                              _addr(d_data_freq_d), _addr(d_chan_freq), _addr(d_chan_time), _addr(d_synch_freq))
        return int(check(self.lib.ofdm_fo_demod_frames(self._h, ptr(d_iq), int(n_frames), int(frame_stride), int(frame_len),
                                                       C.byref(out), ptr(stream))))


class TrkEngine(_Handle):
    """Device primitives of the regression-tracking receiver (reference: LEGACY/gr-ofdm-rx/python/SynchronizeAndEstimate.py):
    strided / single sync trials, LS estimate per accepted sync, data stage.  The sequential pointer logic lives in the
    block mirror (`blocks.SynchronizeAndEstimate`)."""
    _destroy = "ofdm_trk_destroy"

    def __init__(self, nfft, cp_len, num_synch_bins, num_data_bins, synch_D, rows_sync, rows_data, snr, zc_root=23, device=0):
        self.lib = _lib.load()
        self.cfg = _lib.TrkCfg(int(nfft), int(cp_len), int(num_synch_bins), int(num_data_bins), int(synch_D), int(rows_sync),
                               int(rows_data), int(zc_root), float(snr), int(device), 0)
        h = C.c_void_p()
        check(self.lib.ofdm_trk_create(C.byref(self.cfg), C.byref(h)))
        self._h = h

    def load(self, in0: np.ndarray):
        in0 = np.ascontiguousarray(in0, dtype=np.complex64)
        check(self.lib.ofdm_trk_load(self._h, ptr(in0), in0.size))

    def trials(self, first_ptr: int, step: int, count: int):
        peak = np.zeros(max(count, 1), np.float32)
        lag = np.zeros(max(count, 1), np.int32)
        check(self.lib.ofdm_trk_trials(self._h, int(first_ptr), int(step), int(count), ptr(peak), ptr(lag)))
        return peak[:count], lag[:count]

    def accept(self, row: int, window_ptr: int, lag_sync: int, lag_data: int):
        check(self.lib.ofdm_trk_accept(self._h, int(row), int(window_ptr), int(lag_sync), int(lag_data)))

    def demod(self, ptrs, guards):
        n = len(ptrs)
        p = np.ascontiguousarray(ptrs, dtype=np.int64)
        g = np.ascontiguousarray(guards, dtype=np.uint8)
        last = np.zeros(self.cfg.num_data_bins, np.complex64)
        row = C.c_int32(-1)
        check(self.lib.ofdm_trk_demod(self._h, n, ptr(p) if n else None, ptr(g) if n else None, ptr(last), C.byref(row)))
        return int(row.value), last

    def state(self):
        c = self.cfg
        H = np.zeros((c.rows_sync, c.nfft), np.complex64)
        imp = np.zeros((c.rows_sync, c.nfft), np.complex64)
        esf = np.zeros((c.rows_sync, c.num_synch_bins), np.complex64)
        edf = np.zeros((max(c.rows_data, 0), c.num_data_bins), np.complex64)
        check(self.lib.ofdm_trk_get_state(self._h, ptr(H), ptr(imp), ptr(esf), ptr(edf) if c.rows_data > 0 else None))
        return dict(chan_freq=H, chan_impulse=imp, synch_freq=esf, data_freq=edf)


class TxEngine(_Handle):
    """Transmit chain handle (bit map, resource grid + ZC sync symbols, IFFT + CP + normalise) and channel."""
    _destroy = "ofdm_tx_destroy"

    def __init__(self, nfft, cp_len, num_synch_bins, num_data_bins, synch_dat=(1, 3), modulation="QPSK",
                 zc_root=23, device=0):
        self.lib = _lib.load()
        self.cfg = _lib.TxCfg(int(nfft), int(cp_len), int(num_synch_bins), int(num_data_bins), int(synch_dat[0]),
                              int(synch_dat[1]), _mod_bits(modulation), int(zc_root), int(device), 0)
        h = C.c_void_p()
        check(self.lib.ofdm_tx_create(C.byref(self.cfg), C.byref(h)))
        self._h = h

    def data_symbols(self, n_sym: int) -> int:
        c = self.cfg
        sd = c.synch_S + c.synch_D
        n = (n_sym // sd) * c.synch_D
        rem = n_sym % sd
        return n + max(0, rem - c.synch_S)

    def bits_per_frame(self, n_sym: int) -> int:
        return self.data_symbols(n_sym) * self.cfg.num_data_bins * self.cfg.modulation

    def modulate_frames(self, d_bits, n_frames, n_sym, d_iq, frame_stride=None, bits_mode=BITS_UNPACKED, stream=None):
        L = self.cfg.nfft + self.cfg.cp_len
        if frame_stride is None:
            frame_stride = n_sym * L
        check(self.lib.ofdm_tx_modulate_frames(self._h, ptr(d_bits), int(bits_mode), int(n_frames), int(n_sym),
                                               ptr(d_iq), int(frame_stride), ptr(stream)))

    def tbcc_encode_frames(self, d_info, n_seg, blocks_per_seg, K, d_coded, seg_bits, info_mode=BITS_UNPACKED,
                           coded_mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_tbcc_encode_frames: d_info dense [n_seg][blocks_per_seg][K] bits -> d_coded [n_seg][seg_bits]: 3K coded bits per
        block from bit 0 of the segment, then zeros; seg_bits = bits_per_frame(n_sym) feeds modulate_frames directly."""
        check(self.lib.ofdm_tx_tbcc_encode_frames(self._h, ptr(d_info), int(info_mode), int(n_seg), int(blocks_per_seg), int(K),
                                                  ptr(d_coded), int(coded_mode), int(seg_bits), ptr(stream)))

    def tbcc_encode_rm_frames(self, d_info, n_seg, blocks_per_seg, K, E, d_coded, seg_bits, info_mode=BITS_UNPACKED,
                              coded_mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_tbcc_encode_rm_frames: tbcc_encode_frames with the sub-block interleaver and circular-buffer rate matching of
        TS 36.212 5.1.4.2: E coded bits per block from bit 0 of the segment, then zeros."""
        check(self.lib.ofdm_tx_tbcc_encode_rm_frames(self._h, ptr(d_info), int(info_mode), int(n_seg), int(blocks_per_seg), int(K),
                                                     int(E), ptr(d_coded), int(coded_mode), int(seg_bits), ptr(stream)))

    def turbo_encode_frames(self, d_info, n_seg, blocks_per_seg, K, f1, f2, d_coded, seg_bits, info_mode=BITS_UNPACKED,
                            coded_mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_turbo_encode_frames: d_info dense [n_seg][blocks_per_seg][K] bits -> d_coded [n_seg][seg_bits]: 3K + 12 coded
        bits per block (QPP interleaver f1, f2; 12 tail bits) from bit 0 of the segment, then zeros."""
        check(self.lib.ofdm_tx_turbo_encode_frames(self._h, ptr(d_info), int(info_mode), int(n_seg), int(blocks_per_seg), int(K),
                                                   int(f1), int(f2), ptr(d_coded), int(coded_mode), int(seg_bits), ptr(stream)))

    def reserve_turbo_rm(self):
        """Loads the turbo rate-matching kernels (before a graph capture)."""
        check(self.lib.ofdm_tx_reserve_turbo_rm(self._h))

    def turbo_encode_rm_frames(self, d_info, n_seg, blocks_per_seg, K, f1, f2, E, d_coded, seg_bits, Ncb=0, rv=0, d_rv=None,
                               info_mode=BITS_UNPACKED, coded_mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_turbo_encode_rm_frames: turbo_encode_frames with the sub-block interleavers and circular-buffer rate matching of
        TS 36.212 5.1.4.1: E coded bits per block from redundancy version rv (or d_rv, one device int32 per segment) of a buffer
        of Ncb entries (0 = all of it)."""
        check(self.lib.ofdm_tx_turbo_encode_rm_frames(self._h, ptr(d_info), int(info_mode), int(n_seg), int(blocks_per_seg), int(K),
                                                      int(f1), int(f2), int(E), int(Ncb), int(rv), ptr(d_rv), ptr(d_coded),
                                                      int(coded_mode), int(seg_bits), ptr(stream)))

    # ---- transport-block layer (TS 36.212 5.1.1, 5.1.2, 5.1.5): segment, encode per group, concatenate ----
    def reserve_tb(self, n_tb: int, A: int, G: int, Z: int = 0, q: int = 1):
        """Sizes the workspace for n_tb transport blocks of A bits in G coded bits per call and loads the kernels (before a graph
        capture)."""
        check(self.lib.ofdm_tx_reserve_tb(self._h, int(n_tb), int(A), int(Z), int(G), int(q)))

    def tb_encode_frames(self, d_payload, n_tb, A, G, qpp_plus, d_cw, cw_bits, qpp_minus=(0, 0), Z=0, q=1, N_IR=0, rv=0, d_rv=None,
                         payload_mode=BITS_UNPACKED, cw_mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_tb_encode_frames: d_payload dense [n_tb][A] bits -> CRC24A, segmentation at Z (0 = 6144) with CRC24B per code
        block, turbo coding and rate matching to G bits (units of q, redundancy version rv or d_rv per transport block, soft-buffer
        limit N_IR), concatenated into d_cw [n_tb][cw_bits].  qpp_plus / qpp_minus: (f1, f2) for K+ and K- of tb_geometry(A, Z)."""
        check(self.lib.ofdm_tx_tb_encode_frames(self._h, ptr(d_payload), int(payload_mode), int(n_tb), int(A), int(Z), int(G), int(q),
                                                int(N_IR), int(qpp_minus[0]), int(qpp_minus[1]), int(qpp_plus[0]), int(qpp_plus[1]),
                                                int(rv), ptr(d_rv), ptr(d_cw), int(cw_mode), int(cw_bits), ptr(stream)))

    # ---- CRC attach in front of the encoder, Gold-sequence scrambling behind it (TS 36.212 5.1.1, TS 36.211 7.2) ----
    def reserve_bitproc(self):
        """Loads the CRC and scrambling kernels (before a graph capture)."""
        check(self.lib.ofdm_tx_reserve_bitproc(self._h))

    def crc_attach_frames(self, d_payload, n_blocks, A, kind, d_info, mask=0, d_mask=None, payload_mode=BITS_UNPACKED,
                          info_mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_crc_attach_frames: d_payload dense [n_blocks][A] bits -> d_info dense [n_blocks][A + L]: the payload, then the
        parity XORed with the mask (the scalar, or d_mask one device uint32 per block); what tbcc_encode(_rm)_frames reads."""
        check(self.lib.ofdm_tx_crc_attach_frames(self._h, ptr(d_payload), int(payload_mode), int(n_blocks), int(A), int(kind),
                                                 int(mask), ptr(d_mask), ptr(d_info), int(info_mode), ptr(stream)))

    def scramble_frames(self, d_in, n_seg, seg_bits, d_cinit, d_out, mode=BITS_UNPACKED, stream=None):
        """ofdm_tx_scramble_frames: bit n of segment s ^ c(n) of c_init = d_cinit[s] (device uint32), in the segment layout of
        tbcc_encode_frames' coded output; d_out may be d_in."""
        check(self.lib.ofdm_tx_scramble_frames(self._h, ptr(d_in), int(mode), int(n_seg), int(seg_bits), ptr(d_cinit), ptr(d_out),
                                               ptr(stream)))

    # ---- decomposed stages (device buffers)
    def random_bits(self, seed, offset, d_bits, n_bits, stream=None):
        check(self.lib.ofdm_tx_random_bits(self._h, int(seed), int(offset), ptr(d_bits), int(n_bits), ptr(stream)))

    def map(self, d_bits, n_symbols, d_sym, bits_mode=BITS_UNPACKED, stream=None):
        check(self.lib.ofdm_tx_map(self._h, ptr(d_bits), int(bits_mode), int(n_symbols), ptr(d_sym), ptr(stream)))

    def set_pilots(self, locations, value=1.0 + 0.0j):
        loc = np.ascontiguousarray(list(locations), dtype=np.int32)
        check(self.lib.ofdm_tx_set_pilots(self._h, ptr(loc) if loc.size else None, int(loc.size), float(np.real(value)), float(np.imag(value))))

    def grid(self, d_sym, n_rows, d_grid, stream=None):
        check(self.lib.ofdm_tx_grid(self._h, ptr(d_sym), int(n_rows), ptr(d_grid), ptr(stream)))

    def ifft_cp(self, d_in, n_rows, d_out, do_ifft=True, add_cp=True, stream=None):
        check(self.lib.ofdm_tx_ifft_cp(self._h, ptr(d_in), int(n_rows), int(bool(do_ifft)), int(bool(add_cp)), ptr(d_out), ptr(stream)))

    def mux_symbols(self, n_data_sym: int) -> int:
        c = self.cfg
        full, rem = divmod(int(n_data_sym), c.synch_D)
        return full * (c.synch_S + c.synch_D) + (c.synch_S + rem if rem else 0)

    def mux(self, d_data, n_data_sym, d_out, stream=None) -> int:
        return int(check(self.lib.ofdm_tx_mux(self._h, ptr(d_data), int(n_data_sym), ptr(d_out), ptr(stream))))

    # ---- DFT-spread OFDM (SC-FDMA): transform precoding (include/ofdm_mi355x.h, "DFT-spread OFDM")
    def reserve_spread(self, M: int, n_rows: int = 0):
        """ofdm_tx_reserve_spread: the plan for M and the workspace of modulate_frames_spread for n_rows data symbols (before a
        graph capture)."""
        check(self.lib.ofdm_tx_reserve_spread(self._h, int(M), int(n_rows)))

    def dft_spread(self, d_sym, n_rows, M, d_out, stream=None):
        """ofdm_tx_dft_spread: n_rows contiguous rows of M complex64 -> their orthonormal M-point DFTs; d_out may be d_sym."""
        check(self.lib.ofdm_tx_dft_spread(self._h, ptr(d_sym), int(n_rows), int(M), ptr(d_out), ptr(stream)))

    def modulate_frames_spread(self, d_bits, n_frames, n_sym, d_iq, frame_stride=None, bits_mode=BITS_UNPACKED, stream=None) -> int:
        """ofdm_tx_modulate_frames_spread: map -> dft_spread (M = num_data_bins) -> grid -> ifft_cp -> mux over the handle's
        workspace.  n_sym must be a multiple of S + D and frame_stride n_sym*(nfft+cp).  Returns the symbols written."""
        if frame_stride is None:
            frame_stride = int(n_sym) * (self.cfg.nfft + self.cfg.cp_len)
        return int(check(self.lib.ofdm_tx_modulate_frames_spread(self._h, ptr(d_bits), int(bits_mode), int(n_frames), int(n_sym),
                                                                 ptr(d_iq), int(frame_stride), ptr(stream))))

    # ---- multi-user allocations of DFT-spread OFDM (include/ofdm_mi355x.h, "multi-user allocations of DFT-spread OFDM")
    def set_allocations(self, allocs):
        """ofdm_tx_set_allocations: a list of (start, M), at most 32, not overlapping; () clears the set."""
        n, start, M = _alloc_arrays([(a[0], a[1]) for a in allocs], 2)
        check(self.lib.ofdm_tx_set_allocations(self._h, n, ptr(start) if n else None, ptr(M) if n else None))

    def reserve_spread_alloc(self, n_rows: int = 0):
        """ofdm_tx_reserve_spread_alloc: the workspace of modulate_frames_alloc for n_rows data symbols (before a graph capture)."""
        check(self.lib.ofdm_tx_reserve_spread_alloc(self._h, int(n_rows)))

    def dft_spread_alloc(self, d_sym, n_rows, row_len, d_out, stream=None):
        """ofdm_tx_dft_spread_alloc: every allocation of every row replaced by its orthonormal DFT, every other entry by 0; d_out
        may be d_sym."""
        check(self.lib.ofdm_tx_dft_spread_alloc(self._h, ptr(d_sym), int(n_rows), int(row_len), ptr(d_out), ptr(stream)))

    def modulate_frames_alloc(self, d_bits, n_frames, n_sym, d_iq, frame_stride=None, bits_mode=BITS_UNPACKED, stream=None) -> int:
        """ofdm_tx_modulate_frames_alloc: modulate_frames_spread with dft_spread_alloc (row_len = num_data_bins) in place of the
        single transform.  Returns the symbols written."""
        if frame_stride is None:
            frame_stride = int(n_sym) * (self.cfg.nfft + self.cfg.cp_len)
        return int(check(self.lib.ofdm_tx_modulate_frames_alloc(self._h, ptr(d_bits), int(bits_mode), int(n_frames), int(n_sym),
                                                                ptr(d_iq), int(frame_stride), ptr(stream))))

    def sync_symbol(self) -> np.ndarray:
        c = self.cfg
        out = np.zeros((c.synch_S, c.nfft + c.cp_len), np.complex64)
        check(self.lib.ofdm_tx_get_sync_symbol(self._h, ptr(out)))
        return out

    def channel(self, d_in, n_frames, in_stride, in_len, d_taps, n_taps, d_out, out_stride, out_len,
                noise_var=0.0, seed=0, per_frame_taps=False, stream=None):
        check(self.lib.ofdm_channel_apply(self._h, ptr(d_in), int(n_frames), int(in_stride), int(in_len), ptr(d_taps),
                                          int(n_taps), int(bool(per_frame_taps)), float(noise_var), int(seed),
                                          ptr(d_out), int(out_stride), int(out_len), ptr(stream)))
