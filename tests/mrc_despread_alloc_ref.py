"""The contract "receive diversity for multi-user allocations of DFT-spread OFDM" of include/ofdm_mi355x.h restated: a loop over
the allocations that gathers each one's columns of every branch and of every branch's channel powers and hands them to
tests/mrc_despread_ref.py, plus the layout of the outputs.  An allocation is (start, M, bits per symbol).  Shares no code with
the library."""
import numpy as np

import dft_alloc_ref
import mrc_despread_ref as ref

layout = dft_alloc_ref.layout            # sym, llr and bits: allocation-major and dense; comb uses the sym offsets
check_set = dft_alloc_ref.check_set


def row_layout(n_alloc, n_seg, rows):
    """beta and weight are per row, [n_alloc][n_seg][rows]: -> (index of (u, s, r), total)"""
    return (lambda u, s, r: (u * n_seg + s) * rows + r), n_alloc * n_seg * rows


def combine_despread_alloc_segment(z, a, allocs, rho, sigma2):
    """One output segment: z [B][rows][row_len] complex64, a [B][row_len] channel powers, sigma2 [B] doubles (a unit's variance
    is shared by all its allocations) -> per allocation what mrc_despread_ref.combine_despread_segment gives on its gathered
    columns: a list of that function's dicts"""
    z = np.asarray(z, np.complex64)
    a = np.asarray(a, np.float32)
    out = []
    for start, M, _ in allocs:
        out.append(ref.combine_despread_segment(np.ascontiguousarray(z[:, :, start:start + M]),
                                                np.ascontiguousarray(a[:, start:start + M]), rho, sigma2))
    return out


def combine_despread_alloc(z, a, allocs, rho, sigma2):
    """The stage: z [B][n_seg][rows][row_len], a [B][n_seg][row_len], sigma2 [B][n_seg] -> dict of the outputs in the contract's
    layout: sym, comb (complex128 / complex64, allocation-major and dense), llr float32 and bits uint8 (one per byte) from the
    restated sym rounded to float32, beta and weight float32 [n_alloc*n_seg*rows], and segs[u][s] the segments' dicts"""
    z = np.asarray(z, np.complex64)
    B, n_seg, rows, _ = z.shape
    sigma2 = np.asarray(sigma2, np.float64).reshape(B, n_seg)
    so, lo, _, tot = layout(allocs, n_seg, rows)
    at, n_row = row_layout(len(allocs), n_seg, rows)
    sym, comb = np.zeros(tot[0], np.complex128), np.zeros(tot[0], np.complex64)
    llr, bits = np.zeros(tot[1], np.float32), np.zeros(tot[1], np.uint8)
    beta, weight = np.zeros(n_row, np.float32), np.zeros(n_row, np.float32)
    segs = [[None] * n_seg for _ in allocs]
    for s in range(n_seg):
        per = combine_despread_alloc_segment(z[:, s], np.asarray(a)[:, s], allocs, rho, sigma2[:, s])
        for u, ((_, M, mod), seg) in enumerate(zip(allocs, per)):
            n = rows * M
            sym[so[u] + s * n:so[u] + (s + 1) * n] = seg["sym"].ravel()
            comb[so[u] + s * n:so[u] + (s + 1) * n] = seg["comb"].ravel()
            l, b = ref.segment_llr(seg, mod)
            llr[lo[u] + s * n * mod:lo[u] + (s + 1) * n * mod] = l
            bits[lo[u] + s * n * mod:lo[u] + (s + 1) * n * mod] = b
            beta[at(u, s, 0):at(u, s, 0) + rows] = seg["beta32"]
            weight[at(u, s, 0):at(u, s, 0) + rows] = seg["weight32"]
            segs[u][s] = seg
    return dict(sym=sym, comb=comb, llr=llr, bits=bits, beta=beta, weight=weight, segs=segs)
