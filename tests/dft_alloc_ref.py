"""The multi-user allocation contract of include/ofdm_mi355x.h ("multi-user allocations of DFT-spread OFDM") restated: a loop
over the allocations that gathers each one's columns and hands them to tests/dft_spread_ref.py.  An allocation is
(start, M, bits per symbol); the transmit side reads (start, M) alone.  Shares no code with the library."""
import numpy as np

import dft_spread_ref as ref


def check_set(allocs, row_len=4096):
    """the rules of ofdm_rx_set_allocations; -> the reason a set is refused, or None"""
    if len(allocs) > 32:
        return "too many"
    seen = np.zeros(4096, bool)
    for a in allocs:
        start, M = int(a[0]), int(a[1])
        if start < 0:
            return "start < 0"
        if not ref.size_ok(M):
            return "bad M"
        if start + M > 4096:
            return "start + M > 4096"
        if len(a) > 2 and a[2] not in (2, 4, 6):
            return "bad modulation"
        if seen[start:start + M].any():
            return "overlap"
        seen[start:start + M] = True
    if allocs and max(a[0] + a[1] for a in allocs) > row_len:
        return "row too short"
    return None


def layout(allocs, n_seg, rows, packed=False):
    """-> (sym_off, llr_off, bits_off, (sym, llr, bits) totals): block u of sym starts n_seg*rows*sum_{v<u} M_v complex items in,
    llr and bits likewise with M_v*bps_v (packed bits: / 8)"""
    sr = n_seg * rows
    so, lo, bo = [], [], []
    sym = bit = 0
    for _, M, bps in allocs:
        so.append(sr * sym)
        lo.append(sr * bit)
        bo.append(sr * bit // 8 if packed else sr * bit)
        sym += M
        bit += M * bps
    return so, lo, bo, (sr * sym, sr * bit, sr * bit // 8 if packed else sr * bit)


def spread_alloc(x, allocs):
    """transmit precoder: rows [.., row_len] -> every allocation replaced by its orthonormal DFT, every other entry 0 (fp64)"""
    x = np.asarray(x, np.complex128)
    out = np.zeros_like(x)
    for a in allocs:
        s, M = int(a[0]), int(a[1])
        out[..., s:s + M] = ref.spread(x[..., s:s + M])
    return out


def despread_alloc_segment(z, a_row, allocs, rho, sigma2):
    """One segment: z [rows][row_len] complex64, a_row [row_len] or None -> per allocation what dft_spread_ref.despread_segment
    gives on its gathered columns: a list of (sym [rows][M_u] complex128, the weights dict, erased [rows])"""
    z = np.asarray(z, np.complex64)
    out = []
    for s, M, _ in allocs:
        cols = np.ascontiguousarray(z[:, s:s + M])
        out.append(ref.despread_segment(cols, None if a_row is None else np.asarray(a_row, np.float32)[s:s + M], rho, sigma2))
    return out
