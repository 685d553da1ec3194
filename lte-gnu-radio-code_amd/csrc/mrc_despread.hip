// mrc_despread.hip -- receive diversity for DFT-spread OFDM on the batch path (gfx950): the B branches of a group of rows are
// combined per bin (MMSE) straight into LDS, the combined rows go through the inverse transform there, and every row gets its
// own gain and weight from the combined channel.  Definition: include/ofdm_mi355x.h, "receive diversity for DFT-spread OFDM";
// DESIGN.md 9.2.16.  No reference code: the reference has one antenna and transmits plain OFDM.
//
//   mrc_table_kernel (rx_mrc.hip)           tab[g][k] = {c, t} per (unit g = b*n_seg + s, entry k)
//   mrc_despread_rows_kernel<MOD, MORE, CAP> one workgroup per (segment, group of rows_per_group rows):
//     A row belongs to its own lanes (those of dft_rows_in_lds) from the load to the stores: lane l owns the pairs of entries
//     2l, 2l + 2 lanes, ... of its row.
//     load     per pair the B symbols and table entries in rounds of COMB_ROUND branches (16-byte non-temporal loads where that
//              branch's row is 16-byte aligned, 8-byte loads of the same values otherwise), steps 2-4, v conjugated into LDS
//              (and to comb); the lane adds b = A/(A+1) and e = 1/(A+1) of its entries in double as it goes
//     weights  a butterfly over the row's lanes inside the wave, then (rows of 128 and 256 lanes) the waves' totals in wave order:
//              the order depends on M alone, so a row's beta and weight are the same bits wherever it stands.  Every lane of
//              the row ends with the row's float(1/beta) and weight in registers: no table, no atomics, 80 bytes of LDS.
//     passes   dft_rows_in_lds, as the despreading stage
//     epilogue that of despread_rows_kernel with the row's weights, by the row's lanes
// CAP: compiled for M <= DFT_SMALL_M and for every M (dft_mixed.hpp, DftLaneWork).  Every float32 product, sum and quotient is
// rounded on its own (contraction off).
#include "dft_rows_device.hpp"
#include "dft_rows_launch.hpp"

namespace ofdm {

// This kernel keeps the stages as text of its own.  Through combine_row, row_weights and despread_epilogue_rows (dft_rows_device.hpp),
// which mrc_despread_alloc_rows_kernel calls, it measured 1.3 ... 1.9 % slower where the spread of the timed calls was 0.8 ... 1.5 %
// (DESIGN.md 9.2.19); comb_add, comb_finish and COMB_ROUND are the header's.  A change to a stage here is a change to its function
// there: the block-equality tests of test_gpu_mrc_despread_alloc.py compare the two on every output.
template <int MOD, bool MORE, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) mrc_despread_rows_kernel(MrcDespreadArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    __shared__ double part_b[DFT_THREADS / 64], part_e[DFT_THREADS / 64];   // per wave, for rows of more than 64 lanes
    __shared__ int part_nz[DFT_THREADS / 64];
    const DftPlan& pl = a.pl;
    const int M = pl.M, B = a.n_branch;
    const int64_t s = int64_t(blockIdx.x) / a.groups_per_seg;
    const int64_t row0 = (int64_t(blockIdx.x) - s * a.groups_per_seg) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.rows - row0));
    const int cnt = nrows * M;
    const int64_t zb = a.n_seg * a.seg_stride;                           // branch to branch, complex items
    const int64_t tb = a.n_seg * int64_t(M);                             //                   table entries
    const int64_t c0 = (s * a.rows + row0) * M;                          // first symbol of the group in the dense outputs
    // A row belongs to its own pl.lanes lanes from the load to the stores (the lanes of dft_rows_in_lds): lane l owns the pairs
    // of entries 2l, 2l + 2 lanes, ... of its row, so what it adds up, and in which order, depends on M alone.
    const int r = int(threadIdx.x) / pl.lanes, lane = int(threadIdx.x) - r * pl.lanes;
    const bool active = r < nrows;
    cf* row = lds + r * pl.row_elems;
    double sb = 0.0, se = 0.0;                                           // step 6: sums of b = A/(A+1) and e = 1/(A+1)
    int nz = 0;                                                          // the row holds a v that is not 0+0j
    if (active) {
        const cf* p0 = a.sym + s * a.seg_stride + (row0 + r) * M;        // the row in branch 0
        const float2* tab = a.tab + s * M;                               // the segment's entries of branch 0
        unsigned wide_in = 0;                                            // bit b: the row is 16-byte aligned in branch b
        for (int b = 0; b < B; ++b) wide_in |= unsigned((reinterpret_cast<uintptr_t>(p0 + b * zb) & 15) == 0) << b;
        cf* comb = a.comb ? a.comb + c0 + r * M : nullptr;
        const bool wide_c = (reinterpret_cast<uintptr_t>(comb) & 15) == 0;
        for (int i = 2 * lane; i < M; i += 2 * pl.lanes) {
            const bool two = i + 1 < M;
            CombAcc s0{0.f, 0.f, 0.f}, s1{0.f, 0.f, 0.f};
            unsigned m0 = 0, m1 = 0;
            for (int b0 = 0; b0 < B; b0 += COMB_ROUND) {
                cf z0[COMB_ROUND], z1[COMB_ROUND];
                float2 t0[COMB_ROUND], t1[COMB_ROUND];
#pragma unroll
                for (int k = 0; k < COMB_ROUND; ++k) {
                    z0[k] = z1[k] = cf{0.f, 0.f};                        // a slot past the last branch does not take part
                    t0[k] = t1[k] = float2{0.f, 0.f};
                    if (b0 + k < B) {
                        const cf* p = p0 + (b0 + k) * zb;
                        if (((wide_in >> (b0 + k)) & 1u) && two) {
                            const float4 v = load_stream16(reinterpret_cast<const float*>(p + i));
                            z0[k] = cf{v.x, v.y};
                            z1[k] = cf{v.z, v.w};
                        } else {
                            const float2 v0 = load_stream8(reinterpret_cast<const float*>(p + i));
                            z0[k] = cf{v0.x, v0.y};
                            if (two) {
                                const float2 v1 = load_stream8(reinterpret_cast<const float*>(p + i + 1));
                                z1[k] = cf{v1.x, v1.y};
                            }
                        }
                        const float2* tk = tab + (b0 + k) * tb;
                        t0[k] = tk[i];
                        if (two) t1[k] = tk[i + 1];
                    }
                }
#pragma unroll
                for (int k = 0; k < COMB_ROUND; ++k) {
                    m0 |= unsigned(comb_add(s0, z0[k], t0[k]));
                    m1 |= unsigned(comb_add(s1, z1[k], t1[k]));
                }
            }
            const cf v0 = comb_finish(s0, m0), v1 = comb_finish(s1, m1);
            const double A0 = m0 ? double(s0.a) : 0.0, den0 = A0 + 1.0;   // not combined: b = 0, e = 1
            sb += A0 / den0;
            se += 1.0 / den0;
            nz |= int(v0.x != 0.f || v0.y != 0.f);
            row[dft_phys(i, pl.pad)] = cf{v0.x, -v0.y};
            if (two) {
                const double A1 = m1 ? double(s1.a) : 0.0, den1 = A1 + 1.0;
                sb += A1 / den1;
                se += 1.0 / den1;
                nz |= int(v1.x != 0.f || v1.y != 0.f);
                row[dft_phys(i + 1, pl.pad)] = cf{v1.x, -v1.y};
            }
            if (comb) store_sym_pair(comb, i, two, wide_c, v0, v1);
        }
    }
    // The row's lanes add their sums in a butterfly inside the wave (a + b and b + a are the same bits, so every lane of the row
    // ends with the same totals); a row of 128 or 256 lanes then adds its waves' totals in wave order.
    for (int off = min(pl.lanes, 64) >> 1; off > 0; off >>= 1) {
        sb += __shfl_xor(sb, off);
        se += __shfl_xor(se, off);
        nz |= __shfl_xor(nz, off);
    }
    if (pl.lanes > 64 && (threadIdx.x & 63) == 0) {
        part_b[threadIdx.x >> 6] = sb;
        part_e[threadIdx.x >> 6] = se;
        part_nz[threadIdx.x >> 6] = nz;
    }
    __syncthreads();                                                     // the rows of v are in LDS
    if (pl.lanes > 64) {
        const int w0 = r * (pl.lanes >> 6);
        sb = part_b[w0];
        se = part_e[w0];
        nz = part_nz[w0];
        for (int k = 1; k < (pl.lanes >> 6); ++k) {
            sb += part_b[w0 + k];
            se += part_e[w0 + k];
            nz |= part_nz[w0 + k];
        }
    }
    float inv = 0.f, wgt = 0.f;                                          // float(1/beta) (0: the row is not usable) and the weight
    {
        const double beta = sb / double(M), eps = se / double(M);
        const double w = beta / eps;
        auto good = [](double x) { return fabs(x) < __builtin_inf() && x > 0.0; };
        const float inv_f = float(1.0 / beta), w_f = float(w), b_f = float(beta);
        const bool usable = nz != 0 && good(beta) && good(eps) && good(w) && soft_finite(inv_f) && soft_finite(w_f);
        inv = usable ? inv_f : 0.f;                                      // beta <= 1: a usable row has float(1/beta) >= 1
        wgt = usable ? w_f : 0.f;
        if (lane == 0 && active) {
            const int64_t at = s * a.rows + row0 + r;
            if (a.beta) a.beta[at] = usable ? b_f : 0.f;
            if (a.weight) a.weight[at] = wgt;
        }
    }
    if (!a.osym && !a.llr && !a.bits) return;                            // uniform: comb, beta or weight alone
    dft_rows_in_lds<CAP>(pl, a.tw, lds, nrows);
    if (active) {
        cf* osym = a.osym ? a.osym + c0 + r * M : nullptr;
        float* llr = (MORE && a.llr) ? a.llr + (c0 + r * M) * MOD : nullptr;
        const bool wide_s = (reinterpret_cast<uintptr_t>(osym) & 15) == 0, wide_l = (reinterpret_cast<uintptr_t>(llr) & 15) == 0;
        for (int i = 2 * lane; i < M; i += 2 * pl.lanes) {
            const bool two = i + 1 < M;
            cf u[2] = {cf{0.f, 0.f}, cf{0.f, 0.f}};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 0 || two) {
                    cf* p = &row[dft_phys(i + h, pl.pad)];
                    cf x = *p * pl.scale;
                    x.y = -x.y;
                    const cf v = x * inv;
                    const bool ok = inv != 0.f && soft_finite(v.x) && soft_finite(v.y);
                    u[h] = ok ? v : cf{0.f, 0.f};
                    if (MORE) *p = u[h];                                // the hard bits below read the stored symbol
                }
            }
            if (osym) store_sym_pair(osym, i, two, wide_s, u[0], u[1]);
            if constexpr (MORE) {
                if (llr) {
                    float o[2][MOD];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float dr[MOD / 2], di[MOD / 2], mr, mi;
                        soft_axis<MOD>(u[h].x, dr, mr);
                        soft_axis<MOD>(u[h].y, di, mi);
                        const bool nzs = u[h].x != 0.f || u[h].y != 0.f;                  // a zero symbol is an erasure
#pragma unroll
                        for (int j = 0; j < MOD / 2; ++j) {
                            const float vr = wgt * dr[j], vi = wgt * di[j];
                            o[h][2 * j] = (nzs && soft_finite(vr) && vr != 0.f) ? vr : 0.f;   // a zero is +0
                            o[h][2 * j + 1] = (nzs && soft_finite(vi) && vi != 0.f) ? vi : 0.f;
                        }
                    }
                    float* q = llr + int64_t(i) * MOD;
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
    }
    if constexpr (MORE) {
        if (a.bits) {
            __syncthreads();
            auto stored = [&](int e) {
                const RowRef at = row_of(e, M);
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

// The caller has checked the arguments (n_seg * groups_per_seg fits the grid, packed bits fill a row's bytes) and run the table.
hipError_t launch_mrc_despread(const MrcDespreadArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0) return hipSuccess;
    const dim3 g(unsigned(a.n_seg * a.groups_per_seg)), b(DFT_THREADS);
    return with_row_instance(a.pl.M <= DFT_SMALL_M, a.llr || a.bits, a.mod, [&](auto I) {
        hipLaunchKernelGGL((mrc_despread_rows_kernel<I.mod, I.more, I.cap>), g, b, 0, s, a);
        return hipGetLastError();
    });
}

hipError_t mrc_despread_prepare() {
    const hipError_t e = mrc_table_prepare();
    if (e != hipSuccess) return e;
    return each_row_instance([](auto I) { return load_kernels(mrc_despread_rows_kernel<I.mod, I.more, I.cap>); });
}

}  // namespace ofdm
