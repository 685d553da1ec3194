// mrc_despread_alloc.hip -- receive diversity for multi-user allocations of DFT-spread OFDM on the batch path (gfx950): for every
// allocation of the handle's set the B branches of a group of rows are combined per bin (MMSE) straight into LDS, the combined
// rows go through the allocation's inverse transform there, and every row gets its own gain and weight from the combined channel
// of its own columns.  Definition: include/ofdm_mi355x.h, "receive diversity for multi-user allocations of DFT-spread OFDM";
// DESIGN.md 9.2.18.  No reference code: the reference has one antenna, one user, and transmits plain OFDM.
//
//   mrc_table_kernel (rx_mrc.hip)                  tab[g][k] = {c, t} per (unit g = b*n_seg + s, entry k of the whole row): an
//                                                  entry depends on (unit, entry) alone, so entry start_u + i is the same bits as
//                                                  entry i of a table built on the allocation's columns; gaps are computed, not read
//   mrc_despread_alloc_rows_kernel<MOD, MORE, CAP> one workgroup per (allocation, segment, group of rows_per_group(M_u) rows) of one
//                                                  class (CAP and, where llr or bits are wanted, the modulation): the allocation by
//                                                  the wave-uniform prefix-sum walk (alloc_of, dft_rows_launch.hpp), the plan and the
//                                                  twiddles from the set's table, then combine_row, row_weights, dft_rows_in_lds
//                                                  and despread_epilogue_rows (dft_rows_device.hpp) on rows that are row_len apart
//                                                  and start at the allocation's first entry.  The first two and the last are the
//                                                  stages that mrc_despread_rows_kernel (mrc_despread.hip) carries as its own text
// A row's bits depend on (B, M_u) and its own columns alone: they are those of mrc_despread_rows_kernel on a dense copy of the
// allocation's columns of every branch.  Every float32 product, sum and quotient is rounded on its own (contraction off).
#include "dft_rows_device.hpp"
#include "dft_rows_launch.hpp"

namespace ofdm {

template <int MOD, bool MORE, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) mrc_despread_alloc_rows_kernel(MrcDespreadAllocArgs a, DftAllocClass c,
                                                                              const DftAllocDesc* __restrict__ set) {
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    unsigned first;
    const int u = c.idx[alloc_of(c, blockIdx.x, first)];
    const DftAllocDesc& d = set[u];
    const DftPlan& pl = d.pl;
    const int M = pl.M;
    const int64_t groups = (a.rows + pl.rows_per_group - 1) / pl.rows_per_group;
    const int64_t wg = int64_t(blockIdx.x - first);
    const int64_t s = wg / groups;
    const int64_t row0 = (wg - s * groups) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.rows - row0));
    const int64_t seg_rows = a.n_seg * a.rows;
    const int64_t c0 = seg_rows * d.sym_before + (s * a.rows + row0) * M;                  // the group's first symbol, block u
    const int64_t b0 = seg_rows * d.bit_before + (s * a.rows + row0) * M * MOD;            //             first bit
    // A row belongs to its own pl.lanes lanes from the load to the stores (the lanes of dft_rows_in_lds).
    const int r = int(threadIdx.x) / pl.lanes;
    const bool active = r < nrows;
    CombSums sums{0.0, 0.0, 0};
    if (active)                                                          // branch to branch: n_seg*seg_stride symbols, n_seg*row_len table entries
        sums = combine_row(pl, a.sym + s * a.seg_stride + (row0 + r) * a.row_len + d.start, a.n_seg * a.seg_stride,
                           a.tab + s * a.row_len + d.start, a.n_seg * a.row_len, a.n_branch, lds + r * pl.row_elems,
                           a.comb ? a.comb + c0 + r * M : nullptr);
    const RowWeights w = row_weights(pl, sums);                          // with the barrier: the rows of v are in LDS
    if (active && int(threadIdx.x) == r * pl.lanes) {
        const int64_t at = (int64_t(u) * a.n_seg + s) * a.rows + row0 + r;
        if (a.beta) a.beta[at] = w.beta;
        if (a.weight) a.weight[at] = w.wgt;
    }
    if (!a.osym && !a.llr && !a.bits) return;                            // uniform: comb, beta or weight alone
    dft_rows_in_lds<CAP>(pl, d.tw, lds, nrows);
    cf* osym = a.osym ? a.osym + c0 : nullptr;
    float* llr = (MORE && a.llr) ? a.llr + b0 : nullptr;
    uint8_t* bits = (MORE && a.bits) ? a.bits + (a.bits_mode == 2 ? b0 : b0 / 8) : nullptr;
    despread_epilogue_rows<MOD, MORE>(pl, lds, nrows, w.inv, w.wgt, osym, llr, bits, a.bits_mode);
}

// The caller has checked the arguments (every class fits the grid, packed bits fill every allocation's row bytes) and run the
// table over the whole rows.  h_set: the host copy of the set's table.
hipError_t launch_mrc_despread_alloc(const MrcDespreadAllocArgs& a, const DftAllocDesc* h_set, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0 || a.n_alloc <= 0) return hipSuccess;
    const bool more = a.llr || a.bits;
    return for_each_alloc_class(h_set, a.n_alloc, a.n_seg, a.rows, more, [&](const DftAllocClass& c, bool small, int mod) {
        return with_row_instance(small, more, mod, [&](auto I) {
            hipLaunchKernelGGL((mrc_despread_alloc_rows_kernel<I.mod, I.more, I.cap>), dim3(c.end[c.n - 1]), dim3(DFT_THREADS), 0, s, a, c,
                               a.set);
            return hipGetLastError();
        });
    });
}

hipError_t mrc_despread_alloc_prepare() {
    const hipError_t e = mrc_table_prepare();
    if (e != hipSuccess) return e;
    return each_row_instance([](auto I) { return load_kernels(mrc_despread_alloc_rows_kernel<I.mod, I.more, I.cap>); });
}

}  // namespace ofdm
