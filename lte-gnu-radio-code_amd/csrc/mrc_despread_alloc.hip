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
//                                                  the wave-uniform prefix-sum walk of dft_alloc.hip, the plan and the twiddles from
//                                                  the set's table, then what mrc_despread_rows_kernel (mrc_despread.hip) does on
//                                                  rows that are row_len apart and start at the allocation's first entry -- the same
//                                                  lanes per row, the same rounds of loads, the same sums in double in the same
//                                                  butterfly and wave order, dft_rows_in_lds, the same epilogue
// A row's bits depend on (B, M_u) and its own columns alone: they are those of mrc_despread_rows_kernel on a dense copy of the
// allocation's columns of every branch.  Every float32 product, sum and quotient is rounded on its own (contraction off).
//
// comb_add, comb_finish and COMB_ROUND below are a second copy of those of mrc_despread.hip, and alloc_of and make_class a second
// copy of those of dft_alloc.hip: both files keep theirs in an anonymous namespace and stay as they are, so that their code
// objects do not change.  A change to one copy is a change to the other.
#include "dft_rows_device.hpp"
#include "demap_hard.hpp"

namespace ofdm {

namespace {

// Steps 2 and 3 of the combiner for one branch (copy of mrc_despread.hip): t = {c, t} of the entry (c = 0: not usable).
// Returns whether the branch takes part; one that does not leaves the sums.
struct CombAcc {
    float nr, ni, a;
};
__device__ __forceinline__ bool comb_add(CombAcc& s, cf z, float2 t) {
#pragma clang fp contract(off)
    const float pr = z.x * t.x, pi = z.y * t.x;
    const bool in = t.x != 0.f && soft_finite(z.x) && soft_finite(z.y) && (z.x != 0.f || z.y != 0.f) && soft_finite(pr) && soft_finite(pi);
    const float nr = s.nr + pr, ni = s.ni + pi, a = s.a + t.y;
    s.nr = in ? nr : s.nr;
    s.ni = in ? ni : s.ni;
    s.a = in ? a : s.a;
    return in;
}
// Step 4: v = N / (A + 1).  `took` comes back as 0 where the symbol is not combined (then v = 0 and A counts as 0).
__device__ __forceinline__ cf comb_finish(CombAcc s, unsigned& took) {
#pragma clang fp contract(off)
    const float den = s.a + 1.0f;
    const float vr = s.nr / den, vi = s.ni / den;
    const bool ok = took != 0u && soft_finite(s.a) && s.a > 0.f && soft_finite(vr) && soft_finite(vi);
    took = ok ? took : 0u;
    return ok ? cf{vr, vi} : cf{0.f, 0.f};
}

// Branches whose loads a lane issues before any arithmetic: COMB_ROUND of mrc_despread.hip.
constexpr int COMB_ROUND = 2;

// the class's allocation of workgroup b (copy of dft_alloc.hip): k with end[k-1] <= b < end[k]; uniform over the workgroup
__device__ __forceinline__ int alloc_of(const DftAllocClass& c, unsigned b, unsigned& first) {
    int k = 0;
    first = 0;
    while (k < c.n - 1 && b >= c.end[k]) first = c.end[k++];
    return k;
}

}  // namespace

template <int MOD, bool MORE, int CAP>
__global__ void __launch_bounds__(DFT_THREADS) mrc_despread_alloc_rows_kernel(MrcDespreadAllocArgs a, DftAllocClass c,
                                                                              const DftAllocDesc* __restrict__ set) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) cf lds[DFT_LDS_ELEMS];
    __shared__ double part_b[DFT_THREADS / 64], part_e[DFT_THREADS / 64];   // per wave, for rows of more than 64 lanes
    __shared__ int part_nz[DFT_THREADS / 64];
    unsigned first;
    const int u = c.idx[alloc_of(c, blockIdx.x, first)];
    const DftAllocDesc& d = set[u];
    const DftPlan& pl = d.pl;
    const int M = pl.M, B = a.n_branch;
    const int64_t groups = (a.rows + pl.rows_per_group - 1) / pl.rows_per_group;
    const int64_t wg = int64_t(blockIdx.x - first);
    const int64_t s = wg / groups;
    const int64_t row0 = (wg - s * groups) * pl.rows_per_group;
    const int nrows = int(min(int64_t(pl.rows_per_group), a.rows - row0));
    const int cnt = nrows * M;
    const int64_t zb = a.n_seg * a.seg_stride;                           // branch to branch, complex items
    const int64_t tb = a.n_seg * a.row_len;                              //                   table entries
    const int64_t seg_rows = a.n_seg * a.rows;
    const int64_t c0 = seg_rows * d.sym_before + (s * a.rows + row0) * M;                  // the group's first symbol, block u
    const int64_t b0 = seg_rows * d.bit_before + (s * a.rows + row0) * M * MOD;            //             first bit
    // A row belongs to its own pl.lanes lanes from the load to the stores (the lanes of dft_rows_in_lds): lane l owns the pairs
    // of entries 2l, 2l + 2 lanes, ... of its row, so what it adds up, and in which order, depends on M alone.
    const int r = int(threadIdx.x) / pl.lanes, lane = int(threadIdx.x) - r * pl.lanes;
    const bool active = r < nrows;
    cf* row = lds + r * pl.row_elems;
    double sb = 0.0, se = 0.0;                                           // step 6: sums of b = A/(A+1) and e = 1/(A+1)
    int nz = 0;                                                          // the row holds a v that is not 0+0j
    if (active) {
        const cf* p0 = a.sym + s * a.seg_stride + (row0 + r) * a.row_len + d.start;   // the row's columns in branch 0
        const float2* tab = a.tab + s * a.row_len + d.start;             // the segment's entries of branch 0
        unsigned wide_in = 0;                                            // bit b: the row's columns are 16-byte aligned in branch b
        for (int b = 0; b < B; ++b) wide_in |= unsigned((reinterpret_cast<uintptr_t>(p0 + b * zb) & 15) == 0) << b;
        cf* comb = a.comb ? a.comb + c0 + r * M : nullptr;
        const bool wide_c = (reinterpret_cast<uintptr_t>(comb) & 15) == 0;
        for (int i = 2 * lane; i < M; i += 2 * pl.lanes) {
            const bool two = i + 1 < M;
            CombAcc s0{0.f, 0.f, 0.f}, s1{0.f, 0.f, 0.f};
            unsigned m0 = 0, m1 = 0;
            for (int bb = 0; bb < B; bb += COMB_ROUND) {
                cf z0[COMB_ROUND], z1[COMB_ROUND];
                float2 t0[COMB_ROUND], t1[COMB_ROUND];
#pragma unroll
                for (int k = 0; k < COMB_ROUND; ++k) {
                    z0[k] = z1[k] = cf{0.f, 0.f};                        // a slot past the last branch does not take part
                    t0[k] = t1[k] = float2{0.f, 0.f};
                    if (bb + k < B) {
                        const cf* p = p0 + (bb + k) * zb;
                        if (((wide_in >> (bb + k)) & 1u) && two) {
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
                        const float2* tk = tab + (bb + k) * tb;
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
            const int64_t at = (int64_t(u) * a.n_seg + s) * a.rows + row0 + r;
            if (a.beta) a.beta[at] = usable ? b_f : 0.f;
            if (a.weight) a.weight[at] = wgt;
        }
    }
    if (!a.osym && !a.llr && !a.bits) return;                            // uniform: comb, beta or weight alone
    dft_rows_in_lds<CAP>(pl, d.tw, lds, nrows);
    if (active) {
        cf* osym = a.osym ? a.osym + c0 + r * M : nullptr;
        float* llr = (MORE && a.llr) ? a.llr + b0 + int64_t(r) * M * MOD : nullptr;
        const bool wide_s = (reinterpret_cast<uintptr_t>(osym) & 15) == 0, wide_l = (reinterpret_cast<uintptr_t>(llr) & 15) == 0;
        for (int i = 2 * lane; i < M; i += 2 * pl.lanes) {
            const bool two = i + 1 < M;
            cf v[2] = {cf{0.f, 0.f}, cf{0.f, 0.f}};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 0 || two) {
                    cf* p = &row[dft_phys(i + h, pl.pad)];
                    cf x = *p * pl.scale;
                    x.y = -x.y;
                    const cf y = x * inv;
                    const bool ok = inv != 0.f && soft_finite(y.x) && soft_finite(y.y);
                    v[h] = ok ? y : cf{0.f, 0.f};
                    if (MORE) *p = v[h];                                // the hard bits below read the stored symbol
                }
            }
            if (osym) store_sym_pair(osym, i, two, wide_s, v[0], v[1]);
            if constexpr (MORE) {
                if (llr) {
                    float o[2][MOD];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float dr[MOD / 2], di[MOD / 2], mr, mi;
                        soft_axis<MOD>(v[h].x, dr, mr);
                        soft_axis<MOD>(v[h].y, di, mi);
                        const bool nzs = v[h].x != 0.f || v[h].y != 0.f;                  // a zero symbol is an erasure
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
                uint8_t* ob = a.bits + b0;
                for (int e = threadIdx.x; e < cnt; e += DFT_THREADS) {
                    const unsigned hb = hard_bits<MOD>(stored(e));
#pragma unroll
                    for (int b = 0; b < MOD; ++b) ob[int64_t(e) * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
                }
            } else {                                                     // packed MSB-first: a row's bits fill bytes (host check)
                constexpr int U = MOD == 4 ? 2 : 4, NB = U * MOD / 8;      // symbols and bytes of a unit
                uint8_t* ob = a.bits + b0 / 8;
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

namespace {

// the allocations of h_set[0 .. n) that `pick` accepts, with their workgroups (copy of dft_alloc.hip)
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

template <int CAP>
hipError_t launch_rows_class(const MrcDespreadAllocArgs& a, const DftAllocClass& c, int mod, bool more, hipStream_t s) {
    const dim3 g(c.end[c.n - 1]), b(DFT_THREADS);
    if (!more) {
        hipLaunchKernelGGL((mrc_despread_alloc_rows_kernel<2, false, CAP>), g, b, 0, s, a, c, a.set);
    } else {
        switch (mod) {
            case 2: hipLaunchKernelGGL((mrc_despread_alloc_rows_kernel<2, true, CAP>), g, b, 0, s, a, c, a.set); break;
            case 4: hipLaunchKernelGGL((mrc_despread_alloc_rows_kernel<4, true, CAP>), g, b, 0, s, a, c, a.set); break;
            case 6: hipLaunchKernelGGL((mrc_despread_alloc_rows_kernel<6, true, CAP>), g, b, 0, s, a, c, a.set); break;
            default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

}  // namespace

// The caller has checked the arguments (every class fits the grid, packed bits fill every allocation's row bytes) and run the
// table over the whole rows.  h_set: the host copy of the set's table.
hipError_t launch_mrc_despread_alloc(const MrcDespreadAllocArgs& a, const DftAllocDesc* h_set, hipStream_t s) {
    if (a.n_seg <= 0 || a.rows <= 0 || a.n_alloc <= 0) return hipSuccess;
    const bool more = a.llr || a.bits;
    for (int small = 1; small >= 0; --small) {
        for (int mod = 2; mod <= (more ? 6 : 2); mod += 2) {
            const DftAllocClass c = make_class(h_set, a.n_alloc, a.n_seg, a.rows, [&](const DftAllocDesc& d) {
                return (d.pl.M <= DFT_SMALL_M) == bool(small) && (!more || d.mod == mod);
            });
            if (c.n == 0) continue;
            const hipError_t e = small ? launch_rows_class<DFT_SMALL_M>(a, c, mod, more, s) : launch_rows_class<DFT_MAX_M>(a, c, mod, more, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

template <int CAP>
static hipError_t mrc_despread_alloc_prepare_cap() {
    return load_kernels(mrc_despread_alloc_rows_kernel<2, false, CAP>, mrc_despread_alloc_rows_kernel<2, true, CAP>,
                        mrc_despread_alloc_rows_kernel<4, true, CAP>, mrc_despread_alloc_rows_kernel<6, true, CAP>);
}
hipError_t mrc_despread_alloc_prepare() {
    hipError_t e = mrc_table_prepare();
    if (e == hipSuccess) e = mrc_despread_alloc_prepare_cap<DFT_SMALL_M>();
    if (e == hipSuccess) e = mrc_despread_alloc_prepare_cap<DFT_MAX_M>();
    return e;
}

}  // namespace ofdm
