// dft_spread.hip -- DFT-spread OFDM (SC-FDMA, TS 36.211 5.3.3) on the batch path (gfx950): the M-point transform precoder of the
// transmitter and the despreading stage of the receiver with its per-segment weights.  Definition: include/ofdm_mi355x.h,
// "DFT-spread OFDM"; DESIGN.md 9.2.15.  No reference code: the reference transmits plain OFDM.
//
//   dft_rows_kernel<DIR, CAP>       rows of M symbols in, rows out: ofdm_tx_dft_spread (DIR 0) and the plain inverse (DIR 1)
//   despread_table_kernel           one workgroup per segment: beta, float(1/beta), the weight, in double and a fixed order
//   despread_rows_kernel<MOD, MORE, CAP> the inverse transform of a group of rows with its epilogue (unbias, sym, llr, hard bits)
//
// CAP: the row kernels are compiled for M <= DFT_SMALL_M and for every M (dft_mixed.hpp, DftLaneWork).
// A workgroup owns rows_per_group consecutive rows (of one segment): it copies them into LDS (16-byte non-temporal loads where
// the group's first row is 16-byte aligned, 8-byte loads of the same values otherwise), runs the passes of dft_mixed.hpp with
// two barriers each, and writes from LDS in natural order (16-byte stores where aligned).  The arithmetic of an element does
// not depend on the load or store width nor on the row's place in the batch, so its bits depend on (M, the row's data) alone.
// Every float32 product, sum and quotient of the epilogue is rounded on its own (contraction off).
#include "dft_rows_device.hpp"
#include "demap_hard.hpp"

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

// tab[s] = {float(1/beta), weight, beta, usable}: steps 3 of the contract.  One workgroup per segment; a lane adds the entries
// k = lane, lane + 256, ... in that order, block_sum adds the lanes in a fixed order.
__global__ void __launch_bounds__(256) despread_table_kernel(DespreadArgs a) {
    __shared__ double sh0[4], sh1[4];
    const int64_t s = blockIdx.x;
    const int M = a.pl.M;
    float inv = 1.f, wgt = 1.f, bet = 1.f;
    if (a.csi) {
        const float* csi = a.csi + s * a.csi_stride;
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
        a.tab[s] = float4{inv, wgt, bet, inv != 0.f ? 1.f : 0.f};
        if (a.beta) a.beta[s] = bet;
        if (a.weight) a.weight[s] = wgt;
    }
}

// One workgroup per (segment, group of rows_per_group rows).  MORE: llr and / or bits are wanted (MOD = bits per symbol).
template <int MOD, bool MORE, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) despread_rows_kernel(DespreadArgs a) {
#pragma clang fp contract(off)
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
    const float4 t = a.tab[s];                                           // {float(1/beta), weight, beta, usable}
    const int64_t c0 = (s * a.rows + row0) * pl.M;                       // first symbol of the group in the dense outputs
    cf* osym = a.osym ? a.osym + c0 : nullptr;
    float* llr = (MORE && a.llr) ? a.llr + c0 * MOD : nullptr;
    const bool wide_s = (reinterpret_cast<uintptr_t>(osym) & 15) == 0, wide_l = (reinterpret_cast<uintptr_t>(llr) & 15) == 0;
    for (int e = 2 * int(threadIdx.x); e < cnt; e += 2 * DFT_THREADS) {
        const bool two = e + 1 < cnt;
        cf u[2] = {cf{0.f, 0.f}, cf{0.f, 0.f}};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 0 || two) {
                const RowRef at = row_of(e + h, pl.M);
                cf* p = &lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)];
                cf x = *p * pl.scale;
                x.y = -x.y;
                const cf v = x * t.x;
                const bool ok = t.w != 0.f && row_nz[at.r] != 0 && soft_finite(v.x) && soft_finite(v.y);
                u[h] = ok ? v : cf{0.f, 0.f};
                if (MORE) *p = u[h];                                    // the hard bits below read the stored symbol
            }
        }
        if (osym) store_sym_pair(osym, e, two, wide_s, u[0], u[1]);
        if constexpr (MORE) {
            if (llr) {
                float o[2][MOD];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float dr[MOD / 2], di[MOD / 2], mr, mi;
                    soft_axis<MOD>(u[h].x, dr, mr);
                    soft_axis<MOD>(u[h].y, di, mi);
                    const bool nz = u[h].x != 0.f || u[h].y != 0.f;                     // a zero symbol is an erasure
#pragma unroll
                    for (int j = 0; j < MOD / 2; ++j) {
                        const float vr = t.y * dr[j], vi = t.y * di[j];
                        o[h][2 * j] = (nz && soft_finite(vr) && vr != 0.f) ? vr : 0.f;    // a zero is +0
                        o[h][2 * j + 1] = (nz && soft_finite(vi) && vi != 0.f) ? vi : 0.f;
                    }
                }
                float* q = llr + int64_t(e) * MOD;
                if (wide_l && two) {
                    const float* f = &o[0][0];
#pragma unroll
                    for (int k = 0; k < MOD / 2; ++k) store_stream16(q + 4 * k, float4{f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]});
                } else {
#pragma unroll
                    for (int b = 0; b < MOD; ++b) q[b] = o[0][b];
                    if (two) {
#pragma unroll
                        for (int b = 0; b < MOD; ++b) q[MOD + b] = o[1][b];
                    }
                }
            }
        }
    }
    if constexpr (MORE) {
        if (a.bits) {
            __syncthreads();
            auto stored = [&](int e) {
                const RowRef at = row_of(e, pl.M);
                return lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)];
            };
            if (a.bits_mode == 2) {                                      // one bit per byte
                uint8_t* ob = a.bits + c0 * MOD;
                for (int e = threadIdx.x; e < cnt; e += DFT_THREADS) {
                    const unsigned hb = hard_bits<MOD>(stored(e));
#pragma unroll
                    for (int b = 0; b < MOD; ++b) ob[int64_t(e) * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
                }
            } else {                                                     // packed MSB-first: a row's bits fill bytes (host check)
                constexpr int U = MOD == 4 ? 2 : 4, NB = U * MOD / 8;      // symbols and bytes of a unit
                uint8_t* ob = a.bits + c0 * MOD / 8;
                for (int g = threadIdx.x; g * U < cnt; g += DFT_THREADS) {
                    unsigned w = 0;
#pragma unroll
                    for (int h = 0; h < U; ++h) w = (w << MOD) | hard_bits<MOD>(stored(g * U + h));
#pragma unroll
                    for (int b = 0; b < NB; ++b) ob[int64_t(g) * NB + b] = uint8_t(w >> (8 * (NB - 1 - b)));
                }
            }
        }
    }
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

template <int CAP>
static hipError_t launch_despread_rows_cap(const DespreadArgs& a, hipStream_t s) {
    const dim3 g(unsigned(a.n_seg * a.groups_per_seg)), b(DFT_THREADS);
    if (!a.llr && !a.bits) {
        hipLaunchKernelGGL((despread_rows_kernel<2, false, CAP>), g, b, 0, s, a);
    } else {
        switch (a.mod) {
            case 2: hipLaunchKernelGGL((despread_rows_kernel<2, true, CAP>), g, b, 0, s, a); break;
            case 4: hipLaunchKernelGGL((despread_rows_kernel<4, true, CAP>), g, b, 0, s, a); break;
            case 6: hipLaunchKernelGGL((despread_rows_kernel<6, true, CAP>), g, b, 0, s, a); break;
            default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}
// The caller has checked the arguments (n_seg * groups_per_seg fits the grid) and sized tab.
hipError_t launch_despread(const DespreadArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(despread_table_kernel, dim3(unsigned(a.n_seg)), dim3(256), 0, s, a);
    if (!a.osym && !a.llr && !a.bits) return hipGetLastError();
    return a.pl.M <= DFT_SMALL_M ? launch_despread_rows_cap<DFT_SMALL_M>(a, s) : launch_despread_rows_cap<DFT_MAX_M>(a, s);
}

template <int CAP>
static hipError_t dft_spread_prepare_cap() {
    return load_kernels(dft_rows_kernel<0, CAP>, dft_rows_kernel<1, CAP>, despread_rows_kernel<2, false, CAP>, despread_rows_kernel<2, true, CAP>,
                        despread_rows_kernel<4, true, CAP>, despread_rows_kernel<6, true, CAP>);
}
hipError_t dft_spread_prepare() {
    hipError_t e = load_kernels(despread_table_kernel);
    if (e == hipSuccess) e = dft_spread_prepare_cap<DFT_SMALL_M>();
    if (e == hipSuccess) e = dft_spread_prepare_cap<DFT_MAX_M>();
    return e;
}

}  // namespace ofdm
