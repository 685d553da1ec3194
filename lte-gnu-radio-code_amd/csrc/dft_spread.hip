// dft_spread.hip -- DFT-spread OFDM (SC-FDMA, TS 36.211 5.3.3) on the batch path (gfx950): the M-point transform precoder of the
// transmitter and the despreading stage of the receiver with its per-segment weights.  Definition: include/ofdm_mi355x.h,
// "DFT-spread OFDM"; DESIGN.md 9.2.15.  No reference code: the reference transmits plain OFDM.
//
//   dft_rows_kernel<DIR, CAP>       rows of M symbols in, rows out: ofdm_tx_dft_spread (DIR 0) and the plain inverse (DIR 1)
//   despread_table_kernel           one workgroup per segment: beta, float(1/beta), the weight, in double and a fixed order
//                                   (segment_weights)
//   despread_rows_kernel<MOD, MORE, CAP> the inverse transform of a group of rows with its epilogue (unbias, sym, llr, hard bits:
//                                   despread_epilogue)
// segment_weights and despread_epilogue are those of dft_rows_device.hpp, which despread_alloc_*_kernel (dft_alloc.hip) call too.
//
// CAP: the row kernels are compiled for M <= DFT_SMALL_M and for every M (dft_mixed.hpp, DftLaneWork).
// A workgroup owns rows_per_group consecutive rows (of one segment): it copies them into LDS (16-byte non-temporal loads where
// the group's first row is 16-byte aligned, 8-byte loads of the same values otherwise), runs the passes of dft_mixed.hpp with
// two barriers each, and writes from LDS in natural order (16-byte stores where aligned).  The arithmetic of an element does
// not depend on the load or store width nor on the row's place in the batch, so its bits depend on (M, the row's data) alone.
// Every float32 product, sum and quotient of the epilogue is rounded on its own (contraction off).
#include "dft_rows_device.hpp"
#include "dft_rows_launch.hpp"

namespace ofdm {

struct DftRowsArgs {
    DftPlan pl;
    const cf* tw;            // [M] e^(-2 pi i j / M)
    const cf* in;            // [n_rows][M]
    cf* out;                 // [n_rows][M], may be `in`
    int64_t n_rows;
};

template <int DIR, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) dft_rows_kernel(DftRowsArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    const DftPlan& pl = a.pl;
    const int64_t row0 = int64_t(blockIdx.x) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.n_rows - row0));
    const int cnt = nrows * pl.M;
    stage_in<false, DIR == 1>(pl, a.in + row0 * pl.M, cnt, lds, nullptr, nullptr);
    __syncthreads();
    dft_rows_in_lds<CAP>(pl, a.tw, lds, nrows);
    cf* dst = a.out + row0 * pl.M;
    const bool wide = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    for (int e = 2 * int(threadIdx.x); e < cnt; e += 2 * DFT_THREADS) {
        const bool two = e + 1 < cnt;
        cf u[2] = {cf{0.f, 0.f}, cf{0.f, 0.f}};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 0 || two) {
                const RowRef at = row_of(e + h, pl.M);
                u[h] = lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)] * pl.scale;
                if (DIR == 1) u[h].y = -u[h].y;
            }
        }
        store_sym_pair(dst, e, two, wide, u[0], u[1]);
    }
}

// tab[s] = {float(1/beta), weight, beta, usable}: step 3 of the contract, segment_weights (dft_rows_device.hpp).  One workgroup per
// segment.
__global__ void __launch_bounds__(256) despread_table_kernel(DespreadArgs a) {
    __shared__ double sh0[4], sh1[4];
    const int64_t s = blockIdx.x;
    float4 t{1.f, 1.f, 1.f, 1.f};
    if (a.csi) {
        const double sigma2 = a.noise_mode == 0 ? double(a.rho) : a.noise_mode == 1 ? a.noise_var : a.sigma2[s];
        t = segment_weights(a.csi + s * a.csi_stride, a.pl.M, double(a.rho), sigma2, sh0, sh1);
    }
    if (threadIdx.x == 0) {
        a.tab[s] = t;
        if (a.beta) a.beta[s] = t.z;
        if (a.weight) a.weight[s] = t.y;
    }
}

// One workgroup per (segment, group of rows_per_group rows).  MORE: llr and / or bits are wanted (MOD = bits per symbol).
template <int MOD, bool MORE, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) despread_rows_kernel(DespreadArgs a) {
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    __shared__ int row_nz[DFT_THREADS];
    const DftPlan& pl = a.pl;
    const int64_t s = int64_t(blockIdx.x) / a.groups_per_seg;
    const int64_t row0 = (int64_t(blockIdx.x) - s * a.groups_per_seg) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.rows - row0));
    const int cnt = nrows * pl.M;
    row_nz[threadIdx.x] = 0;
    __syncthreads();
    stage_in<true, true>(pl, a.sym + s * a.seg_stride + row0 * pl.M, cnt, lds, a.csi ? a.csi + s * a.csi_stride : nullptr, row_nz);
    __syncthreads();
    dft_rows_in_lds<CAP>(pl, a.tw, lds, nrows);
    const int64_t c0 = (s * a.rows + row0) * pl.M;                       // first symbol of the group in the dense outputs
    cf* osym = a.osym ? a.osym + c0 : nullptr;
    float* llr = (MORE && a.llr) ? a.llr + c0 * MOD : nullptr;
    uint8_t* bits = (MORE && a.bits) ? a.bits + (a.bits_mode == 2 ? c0 * MOD : c0 * MOD / 8) : nullptr;
    despread_epilogue<MOD, MORE>(pl, lds, row_nz, cnt, a.tab[s], osym, llr, bits, a.bits_mode);
}

template <int CAP>
static void launch_dft_rows_cap(const DftRowsArgs& a, unsigned g, int inverse, hipStream_t s) {
    if (inverse)
        hipLaunchKernelGGL((dft_rows_kernel<1, CAP>), dim3(g), dim3(DFT_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((dft_rows_kernel<0, CAP>), dim3(g), dim3(DFT_THREADS), 0, s, a);
}
hipError_t launch_dft_rows(const DftPlan& pl, const cf* tw, const cf* in, cf* out, int64_t n_rows, int inverse, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    DftRowsArgs a{pl, tw, in, out, n_rows};
    const unsigned g = unsigned((n_rows + pl.rows_per_group - 1) / pl.rows_per_group);
    if (pl.M <= DFT_SMALL_M)
        launch_dft_rows_cap<DFT_SMALL_M>(a, g, inverse, s);
    else
        launch_dft_rows_cap<DFT_MAX_M>(a, g, inverse, s);
    return hipGetLastError();
}

// The caller has checked the arguments (n_seg * groups_per_seg fits the grid) and sized tab.
hipError_t launch_despread(const DespreadArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(despread_table_kernel, dim3(unsigned(a.n_seg)), dim3(256), 0, s, a);
    if (!a.osym && !a.llr && !a.bits) return hipGetLastError();
    const dim3 g(unsigned(a.n_seg * a.groups_per_seg)), b(DFT_THREADS);
    return with_row_instance(a.pl.M <= DFT_SMALL_M, a.llr || a.bits, a.mod, [&](auto I) {
        hipLaunchKernelGGL((despread_rows_kernel<I.mod, I.more, I.cap>), g, b, 0, s, a);
        return hipGetLastError();
    });
}

hipError_t dft_spread_prepare() {
    const hipError_t e = load_kernels(despread_table_kernel, dft_rows_kernel<0, DFT_SMALL_M>, dft_rows_kernel<1, DFT_SMALL_M>,
                                      dft_rows_kernel<0, DFT_MAX_M>, dft_rows_kernel<1, DFT_MAX_M>);
    if (e != hipSuccess) return e;
    return each_row_instance([](auto I) { return load_kernels(despread_rows_kernel<I.mod, I.more, I.cap>); });
}

}  // namespace ofdm
