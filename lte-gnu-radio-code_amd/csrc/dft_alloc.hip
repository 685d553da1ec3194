// dft_alloc.hip -- multi-user allocations of DFT-spread OFDM on the batch path (gfx950): several users share a row, each with a
// contiguous run of entries, its own transform size and (receiver) its own modulation, gain and weight.  Definition:
// include/ofdm_mi355x.h, "multi-user allocations of DFT-spread OFDM"; DESIGN.md 9.2.17.  No reference code.
//
//   despread_alloc_table_kernel               one workgroup of 256 per (allocation, segment): the sums of despread_table_kernel
//                                             (dft_spread.hip) over the allocation's entries, same lane order, same block_sum
//   despread_alloc_rows_kernel<MOD, MORE, CAP> one workgroup per (allocation, segment, group of rows_per_group(M_u) rows): strided
//                                             staging, dft_rows_in_lds, despread_epilogue (dft_rows_device.hpp)
//   dft_alloc_rows_kernel<CAP>                the transmitter: every allocation of a row replaced by its DFT, the gaps by +0
//
// The number of launches does not grow with the number of allocations: a launch serves every allocation of one class -- CAP
// (M <= DFT_SMALL_M or not, the occupancy classes of dft_mixed.hpp) and, where llr or bits are wanted, the modulation -- and a
// workgroup finds its allocation from blockIdx.x by a wave-uniform walk over the class's prefix sums (<= 32 entries, in the
// kernel arguments: they depend on the call's rows and n_seg, the set's table on the device does not).  The plan and the
// twiddles are read from the set's table.  An element's bits depend on (M_u, the row's entries) alone: they are those of the
// single-M kernels on a dense copy of the allocation's columns.
#include "dft_rows_device.hpp"

namespace ofdm {

namespace {

// the class's allocation of workgroup b: k with end[k-1] <= b < end[k]; uniform over the workgroup
__device__ __forceinline__ int alloc_of(const DftAllocClass& c, unsigned b, unsigned& first) {
    int k = 0;
    first = 0;
    while (k < c.n - 1 && b >= c.end[k]) first = c.end[k++];
    return k;
}

}  // namespace

__global__ void __launch_bounds__(256) despread_alloc_table_kernel(DespreadAllocArgs a, const DftAllocDesc* __restrict__ set) {
    __shared__ double sh0[4], sh1[4];
    const int64_t u = int64_t(blockIdx.x) / a.n_seg, s = int64_t(blockIdx.x) - u * a.n_seg;
    const int M = set[u].pl.M;
    float inv = 1.f, wgt = 1.f, bet = 1.f;
    if (a.csi) {
        const float* csi = a.csi + s * a.csi_stride + set[u].start;
        const double rho = double(a.rho);
        const double sigma2 = a.noise_mode == 0 ? rho : a.noise_mode == 1 ? a.noise_var : a.sigma2[s];
        double sb = 0.0;
        for (int k = threadIdx.x; k < M; k += 256) {
            const float av = csi[k];
            if (soft_finite(av) && av > 0.f) sb += double(av) / (double(av) + rho);
        }
        const double beta = block_sum(sb, sh0) / double(M);
        double sv = 0.0;
        for (int k = threadIdx.x; k < M; k += 256) {
            const float av = csi[k];
            const bool ok = soft_finite(av) && av > 0.f;
            const double ad = double(av), den = ad + rho;
            const double b = ok ? ad / den : 0.0;
            double t = (b - beta) * (b - beta);
            if (ok) t += sigma2 * ad / (den * den);
            sv += t;
        }
        const double nu = block_sum(sv, sh1) / double(M);
        const double w = beta * beta / nu;
        auto good = [](double x) { return fabs(x) < __builtin_inf() && x > 0.0; };
        const float inv_f = float(1.0 / beta), w_f = float(w), b_f = float(beta);
        const bool usable = good(beta) && good(nu) && good(w) && soft_finite(inv_f) && soft_finite(w_f);
        inv = usable ? inv_f : 0.f;
        wgt = usable ? w_f : 0.f;
        bet = usable ? b_f : 0.f;
    }
    if (threadIdx.x == 0) {
        a.tab[blockIdx.x] = float4{inv, wgt, bet, inv != 0.f ? 1.f : 0.f};
        if (a.beta) a.beta[blockIdx.x] = bet;
        if (a.weight) a.weight[blockIdx.x] = wgt;
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

namespace {

// the allocations of h_set[0 .. n) that `pick` accepts, with their workgroups: units (segments, or 1) times the groups of `rows`
template <class Pick>
DftAllocClass make_class(const DftAllocDesc* h_set, int n, int64_t units, int64_t rows, Pick pick) {
    DftAllocClass c{};
    uint64_t end = 0;
    for (int u = 0; u < n; ++u) {
        if (!pick(h_set[u])) continue;
        const int rpg = h_set[u].pl.rows_per_group;
        end += uint64_t(units) * uint64_t((rows + rpg - 1) / rpg);
        c.idx[c.n] = uint8_t(u);
        c.end[c.n++] = unsigned(end);
    }
    return c;
}
bool cap_small(const DftAllocDesc& d) { return d.pl.M <= DFT_SMALL_M; }

template <int CAP>
hipError_t launch_rows_class(const DespreadAllocArgs& a, const DftAllocClass& c, int mod, bool more, hipStream_t s) {
    const dim3 g(c.end[c.n - 1]), b(DFT_THREADS);
    if (!more) {
        hipLaunchKernelGGL((despread_alloc_rows_kernel<2, false, CAP>), g, b, 0, s, a, c, a.set);
    } else {
        switch (mod) {
            case 2: hipLaunchKernelGGL((despread_alloc_rows_kernel<2, true, CAP>), g, b, 0, s, a, c, a.set); break;
            case 4: hipLaunchKernelGGL((despread_alloc_rows_kernel<4, true, CAP>), g, b, 0, s, a, c, a.set); break;
            case 6: hipLaunchKernelGGL((despread_alloc_rows_kernel<6, true, CAP>), g, b, 0, s, a, c, a.set); break;
            default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_despread_alloc(const DespreadAllocArgs& a, const DftAllocDesc* h_set, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0 || a.n_alloc <= 0) return hipSuccess;
    hipLaunchKernelGGL(despread_alloc_table_kernel, dim3(unsigned(a.n_alloc * a.n_seg)), dim3(256), 0, s, a, a.set);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!a.osym && !a.llr && !a.bits)) return e;
    const bool more = a.llr || a.bits;
    for (int small = 1; small >= 0; --small) {
        for (int mod = 2; mod <= (more ? 6 : 2); mod += 2) {
            const DftAllocClass c = make_class(h_set, a.n_alloc, a.n_seg, a.rows, [&](const DftAllocDesc& d) {
                return cap_small(d) == bool(small) && (!more || d.mod == mod);
            });
            if (c.n == 0) continue;
            e = small ? launch_rows_class<DFT_SMALL_M>(a, c, mod, more, s) : launch_rows_class<DFT_MAX_M>(a, c, mod, more, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_dft_alloc_rows(DftAllocRowsArgs a, const DftAllocDesc* h_set, int n_alloc, hipStream_t s) {
    if (a.n_rows <= 0 || n_alloc <= 0) return hipSuccess;
    unsigned zero = a.n_gap > 0 ? unsigned(std::min<int64_t>(a.n_rows, 1024)) : 0u;
    for (int small = 1; small >= 0; --small) {
        const DftAllocClass c = make_class(h_set, n_alloc, 1, a.n_rows, [&](const DftAllocDesc& d) { return cap_small(d) == bool(small); });
        if (c.n == 0) continue;
        a.zero_groups = zero;
        const dim3 g(c.end[c.n - 1] + zero), b(DFT_THREADS);
        if (small)
            hipLaunchKernelGGL((dft_alloc_rows_kernel<DFT_SMALL_M>), g, b, 0, s, a, c, a.set);
        else
            hipLaunchKernelGGL((dft_alloc_rows_kernel<DFT_MAX_M>), g, b, 0, s, a, c, a.set);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        zero = 0;                                                        // the gaps are written by the first launch
    }
    return hipSuccess;
}

template <int CAP>
static hipError_t dft_alloc_prepare_cap() {
    return load_kernels(dft_alloc_rows_kernel<CAP>, despread_alloc_rows_kernel<2, false, CAP>, despread_alloc_rows_kernel<2, true, CAP>,
                        despread_alloc_rows_kernel<4, true, CAP>, despread_alloc_rows_kernel<6, true, CAP>);
}
hipError_t dft_alloc_prepare() {
    hipError_t e = load_kernels(despread_alloc_table_kernel);
    if (e == hipSuccess) e = dft_alloc_prepare_cap<DFT_SMALL_M>();
    if (e == hipSuccess) e = dft_alloc_prepare_cap<DFT_MAX_M>();
    return e;
}

}  // namespace ofdm
