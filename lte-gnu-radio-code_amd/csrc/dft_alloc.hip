// dft_alloc.hip -- multi-user allocations of DFT-spread OFDM on the batch path (gfx950): several users share a row, each with a
// contiguous run of entries, its own transform size and (receiver) its own modulation, gain and weight.  Definition:
// include/ofdm_mi355x.h, "multi-user allocations of DFT-spread OFDM"; DESIGN.md 9.2.17.  No reference code.
//
//   despread_alloc_table_kernel               one workgroup of 256 per (allocation, segment): segment_weights (dft_rows_device.hpp),
//                                             which despread_table_kernel (dft_spread.hip) calls too, over the allocation's entries
//   despread_alloc_rows_kernel<MOD, MORE, CAP> one workgroup per (allocation, segment, group of rows_per_group(M_u) rows): strided
//                                             staging, dft_rows_in_lds, despread_epilogue (dft_rows_device.hpp)
//   dft_alloc_rows_kernel<CAP>                the transmitter: every allocation of a row replaced by its DFT, the gaps by +0
//
// The number of launches does not grow with the number of allocations: a launch serves every allocation of one class -- CAP
// (M <= DFT_SMALL_M or not, the occupancy classes of dft_mixed.hpp) and, where llr or bits are wanted, the modulation -- and a
// workgroup finds its allocation from blockIdx.x by a wave-uniform walk over the class's prefix sums (<= 32 entries, in the
// kernel arguments: they depend on the call's rows and n_seg, the set's table on the device does not).  The plan and the
// twiddles are read from the set's table.  An element's bits depend on (M_u, the row's entries) alone: they are those of the
// single-M kernels on a dense copy of the allocation's columns -- segment_weights, dft_rows_in_lds and despread_epilogue are the
// functions those kernels call; what differs is the addressing.  The classes and the lookup are in dft_rows_launch.hpp.
#include "dft_rows_device.hpp"
#include "dft_rows_launch.hpp"

namespace ofdm {

__global__ void __launch_bounds__(256) despread_alloc_table_kernel(DespreadAllocArgs a, const DftAllocDesc* __restrict__ set) {
    __shared__ double sh0[4], sh1[4];
    const int64_t u = int64_t(blockIdx.x) / a.n_seg, s = int64_t(blockIdx.x) - u * a.n_seg;
    float4 t{1.f, 1.f, 1.f, 1.f};
    if (a.csi) {
        const double sigma2 = a.noise_mode == 0 ? double(a.rho) : a.noise_mode == 1 ? a.noise_var : a.sigma2[s];
        t = segment_weights(a.csi + s * a.csi_stride + set[u].start, set[u].pl.M, double(a.rho), sigma2, sh0, sh1);
    }
    if (threadIdx.x == 0) {
        a.tab[blockIdx.x] = t;
        if (a.beta) a.beta[blockIdx.x] = t.z;
        if (a.weight) a.weight[blockIdx.x] = t.y;
    }
}

template <int MOD, bool MORE, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) despread_alloc_rows_kernel(DespreadAllocArgs a, DftAllocClass c,
                                                                          const DftAllocDesc* __restrict__ set) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    __shared__ int row_nz[DFT_THREADS];
    unsigned first;
    const int u = c.idx[alloc_of(c, blockIdx.x, first)];
    const DftAllocDesc& d = set[u];
    const DftPlan& pl = d.pl;
    const int64_t groups = (a.rows + pl.rows_per_group - 1) / pl.rows_per_group;
    const int64_t b = int64_t(blockIdx.x - first);
    const int64_t s = b / groups;
    const int64_t row0 = (b - s * groups) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.rows - row0));
    const int cnt = nrows * pl.M;
    row_nz[threadIdx.x] = 0;
    __syncthreads();
    stage_in_strided<true, true>(pl, a.sym + s * a.seg_stride + row0 * a.row_len + d.start, a.row_len, nrows, lds,
                                 a.csi ? a.csi + s * a.csi_stride + d.start : nullptr, row_nz);
    __syncthreads();
    dft_rows_in_lds<CAP>(pl, d.tw, lds, nrows);
    const float4 t = a.tab[int64_t(u) * a.n_seg + s];                    // {float(1/beta), weight, beta, usable}
    const int64_t seg_rows = a.n_seg * a.rows;
    const int64_t c0 = seg_rows * d.sym_before + (s * a.rows + row0) * pl.M;               // the group's first symbol, block u
    const int64_t b0 = seg_rows * d.bit_before + (s * a.rows + row0) * pl.M * MOD;         //             first bit
    cf* osym = a.osym ? a.osym + c0 : nullptr;
    float* llr = (MORE && a.llr) ? a.llr + b0 : nullptr;
    uint8_t* bits = (MORE && a.bits) ? a.bits + (a.bits_mode == 2 ? b0 : b0 / 8) : nullptr;
    despread_epilogue<MOD, MORE>(pl, lds, row_nz, cnt, t, osym, llr, bits, a.bits_mode);
}

template <int CAP>
__global__ void __launch_bounds__(DFT_THREADS) dft_alloc_rows_kernel(DftAllocRowsArgs a, DftAllocClass c,
                                                                     const DftAllocDesc* __restrict__ set) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    const unsigned own = c.end[c.n - 1];
    if (blockIdx.x >= own) {                                             // uniform: the gaps of rows zb, zb + zero_groups, ...
        for (int64_t r = blockIdx.x - own; r < a.n_rows; r += a.zero_groups) {
            cf* row = a.out + r * a.row_len;
            for (int g = 0; g < a.n_gap; ++g)
                for (int i = threadIdx.x; i < a.gap_len[g]; i += DFT_THREADS)
                    store_stream8(reinterpret_cast<float*>(row + a.gap_start[g] + i), float2{0.f, 0.f});
        }
        return;
    }
    unsigned first;
    const DftAllocDesc& d = set[c.idx[alloc_of(c, blockIdx.x, first)]];
    const DftPlan& pl = d.pl;
    const int64_t row0 = int64_t(blockIdx.x - first) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.n_rows - row0));
    stage_in_strided<false, false>(pl, a.in + row0 * a.row_len + d.start, a.row_len, nrows, lds, nullptr, nullptr);
    __syncthreads();
    dft_rows_in_lds<CAP>(pl, d.tw, lds, nrows);                          // ends with a barrier: every load of the group is done
    cf* dst = a.out + row0 * a.row_len + d.start;
    const int pairs = nrows * ((pl.M + 1) >> 1);
    for (int j = int(threadIdx.x); j < pairs; j += DFT_THREADS) {
        const PairRef at = pair_of(j, pl.M);
        cf* row = dst + at.r * a.row_len;
        const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
        const cf* p = &lds[at.r * pl.row_elems];
        const cf u0 = p[dft_phys(at.i, pl.pad)] * pl.scale;
        const cf u1 = at.two ? p[dft_phys(at.i + 1, pl.pad)] * pl.scale : cf{0.f, 0.f};
        store_sym_pair(row, at.i, at.two, wide, u0, u1);
    }
}

hipError_t launch_despread_alloc(const DespreadAllocArgs& a, const DftAllocDesc* h_set, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0 || a.n_alloc <= 0) return hipSuccess;
    hipLaunchKernelGGL(despread_alloc_table_kernel, dim3(unsigned(a.n_alloc * a.n_seg)), dim3(256), 0, s, a, a.set);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!a.osym && !a.llr && !a.bits)) return e;
    const bool more = a.llr || a.bits;
    return for_each_alloc_class(h_set, a.n_alloc, a.n_seg, a.rows, more, [&](const DftAllocClass& c, bool small, int mod) {
        return with_row_instance(small, more, mod, [&](auto I) {
            hipLaunchKernelGGL((despread_alloc_rows_kernel<I.mod, I.more, I.cap>), dim3(c.end[c.n - 1]), dim3(DFT_THREADS), 0, s, a, c, a.set);
            return hipGetLastError();
        });
    });
}

hipError_t launch_dft_alloc_rows(DftAllocRowsArgs a, const DftAllocDesc* h_set, int n_alloc, hipStream_t s) {
    if (a.n_rows <= 0 || n_alloc <= 0) return hipSuccess;
    a.zero_groups = a.n_gap > 0 ? unsigned(std::min<int64_t>(a.n_rows, 1024)) : 0u;
    return for_each_alloc_class(h_set, n_alloc, 1, a.n_rows, false, [&](const DftAllocClass& c, bool small, int) {
        const dim3 g(c.end[c.n - 1] + a.zero_groups), b(DFT_THREADS);
        if (small)
            hipLaunchKernelGGL((dft_alloc_rows_kernel<DFT_SMALL_M>), g, b, 0, s, a, c, a.set);
        else
            hipLaunchKernelGGL((dft_alloc_rows_kernel<DFT_MAX_M>), g, b, 0, s, a, c, a.set);
        a.zero_groups = 0;                                               // the gaps are written by the first launch
        return hipGetLastError();
    });
}

hipError_t dft_alloc_prepare() {
    const hipError_t e = load_kernels(despread_alloc_table_kernel, dft_alloc_rows_kernel<DFT_SMALL_M>, dft_alloc_rows_kernel<DFT_MAX_M>);
    if (e != hipSuccess) return e;
    return each_row_instance([](auto I) { return load_kernels(despread_alloc_rows_kernel<I.mod, I.more, I.cap>); });
}

}  // namespace ofdm
