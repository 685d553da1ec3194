// dft_rows_device.hpp -- what the row kernels of DFT-spread OFDM share on the device (gfx950): a group of rows staged into LDS,
// the passes of dft_mixed.hpp over them, the paired symbol store, and every stage of the despreading kernels that more than one
// of them runs, each defined once:
//   despread_epilogue       (unbias, soft_pair, hard_bits_sweep)   despread_rows_kernel, despread_alloc_rows_kernel
//   despread_epilogue_rows  (the same three pieces)                mrc_despread_alloc_rows_kernel
//   combine_row, row_weights (comb_add, comb_finish)               mrc_despread_alloc_rows_kernel
//   segment_weights                                                despread_table_kernel, despread_alloc_table_kernel
// mrc_despread_rows_kernel uses comb_add and comb_finish and keeps the rest as text of its own: through the functions it measured
// 1.3 ... 1.9 % slower, so there a change to a stage is still a change in two places.
// A single-M kernel (dft_spread.hip, mrc_despread.hip) and its allocation kernel (dft_alloc.hip,
// mrc_despread_alloc.hip; 9.2.17, 9.2.18) differ in where a row's entries and its outputs lie, not in what is computed: that block u
// of an allocation call is bit for bit the single-M call follows from the shared code plus the addressing, which the tests check.
#pragma once
#include "ofdm_launch.hpp"
#include "dft_mixed.hpp"
#include "soft_device.hpp"
#include "demap_hard.hpp"

namespace ofdm {

namespace {

struct RowRef {
    int r, i;                // local row, entry
};
__device__ __forceinline__ RowRef row_of(int e, int M) {
    const int r = int(unsigned(e) / unsigned(M));
    return RowRef{r, e - r * M};
}

// Elements 0 .. cnt-1 of the group's rows (contiguous at src) into LDS.  MASK: step 1 of the despread contract (csi: the
// segment's row of channel powers, or null) and the rows that hold anything but zeros marked in row_nz.  CONJ: conjugated.
template <bool MASK, bool CONJ>
__device__ __forceinline__ void stage_in(const DftPlan& pl, const cf* src, int cnt, cf* lds, const float* csi, int* row_nz) {
    const bool wide = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    auto put = [&](int e, cf z) {
        const RowRef at = row_of(e, pl.M);
        if constexpr (MASK) {
            bool ok = soft_finite(z.x) && soft_finite(z.y);
            if (csi) {
                const float a = csi[at.i];
                ok = ok && soft_finite(a) && a > 0.f;
            }
            if (!ok) z = cf{0.f, 0.f};
            if (z.x != 0.f || z.y != 0.f) row_nz[at.r] = 1;
        }
        if constexpr (CONJ) z.y = -z.y;
        lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)] = z;
    };
    for (int e = 2 * int(threadIdx.x); e < cnt; e += 2 * DFT_THREADS) {
        const bool two = e + 1 < cnt;
        if (wide && two) {
            const float4 v = load_stream16(reinterpret_cast<const float*>(src + e));
            put(e, cf{v.x, v.y});
            put(e + 1, cf{v.z, v.w});
        } else {
            const float2 v0 = load_stream8(reinterpret_cast<const float*>(src + e));
            put(e, cf{v0.x, v0.y});
            if (two) {
                const float2 v1 = load_stream8(reinterpret_cast<const float*>(src + e + 1));
                put(e + 1, cf{v1.x, v1.y});
            }
        }
    }
}

// the passes of the nrows rows in LDS; every lane of the workgroup calls this.  CAP >= pl.M (DFT_SMALL_M or DFT_MAX_M)
template <int CAP>
__device__ __forceinline__ void dft_rows_in_lds(const DftPlan& pl, const cf* tw, cf* lds, int nrows) {
    const int r = int(threadIdx.x) / pl.lanes, lane = int(threadIdx.x) - r * pl.lanes;
    const bool active = r < nrows;
    cf* row = lds + r * pl.row_elems;
    cf v[DFT_MAX_REGS];
    int s = 1;
    for (int p = 0; p < pl.n_pass; ++p) {
        const int R = pl.radix[p];
        if (active) dft_pass_load_rt<CAP>(pl, R, s, lane, row, tw, v);
        __syncthreads();
        if (active) dft_pass_store_rt<CAP>(pl, R, s, lane, row, v);
        __syncthreads();
        s *= R;
    }
}

__device__ __forceinline__ void store_sym_pair(cf* dst, int e, bool two, bool wide, cf u0, cf u1) {
    if (wide && two) {
        store_stream16(reinterpret_cast<float*>(dst + e), float4{u0.x, u0.y, u1.x, u1.y});
    } else {
        store_stream8(reinterpret_cast<float*>(dst + e), float2{u0.x, u0.y});
        if (two) store_stream8(reinterpret_cast<float*>(dst + e + 1), float2{u1.x, u1.y});
    }
}

// ---- rows that are not contiguous: an allocation of M entries inside rows of row_len (dft_alloc.hip)

// Pair j of a group of nrows rows of M entries: row r = j / ceil(M/2), entries i and i + 1 of that row.  A pair never straddles
// two rows (a row of odd M ends with a single).
struct PairRef {
    int r, i;
    bool two;
};
__device__ __forceinline__ PairRef pair_of(int j, int M) {
    const int P = (M + 1) >> 1;
    const int r = int(unsigned(j) / unsigned(P));
    const int i = 2 * (j - r * P);
    return PairRef{r, i, i + 1 < M};
}

// stage_in for rows that lie row_stride apart: local row r starts at src + r*row_stride.  The width is chosen PER ROW (16-byte
// non-temporal loads where that row's base is 16-byte aligned, 8-byte loads of the same values otherwise): with an odd start
// or an odd row_stride the alignment alternates from row to row.  csi: the channel powers of the row's entries (entry 0 first).
template <bool MASK, bool CONJ>
__device__ __forceinline__ void stage_in_strided(const DftPlan& pl, const cf* src, int64_t row_stride, int nrows, cf* lds,
                                                 const float* csi, int* row_nz) {
    auto put = [&](int r, int i, cf z) {
        if constexpr (MASK) {
            bool ok = soft_finite(z.x) && soft_finite(z.y);
            if (csi) {
                const float a = csi[i];
                ok = ok && soft_finite(a) && a > 0.f;
            }
            if (!ok) z = cf{0.f, 0.f};
            if (z.x != 0.f || z.y != 0.f) row_nz[r] = 1;
        }
        if constexpr (CONJ) z.y = -z.y;
        lds[r * pl.row_elems + dft_phys(i, pl.pad)] = z;
    };
    const int pairs = nrows * ((pl.M + 1) >> 1);
    for (int j = int(threadIdx.x); j < pairs; j += DFT_THREADS) {
        const PairRef at = pair_of(j, pl.M);
        const cf* row = src + at.r * row_stride;
        const bool wide = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
        if (wide && at.two) {
            const float4 v = load_stream16(reinterpret_cast<const float*>(row + at.i));
            put(at.r, at.i, cf{v.x, v.y});
            put(at.r, at.i + 1, cf{v.z, v.w});
        } else {
            const float2 v0 = load_stream8(reinterpret_cast<const float*>(row + at.i));
            put(at.r, at.i, cf{v0.x, v0.y});
            if (at.two) {
                const float2 v1 = load_stream8(reinterpret_cast<const float*>(row + at.i + 1));
                put(at.r, at.i + 1, cf{v1.x, v1.y});
            }
        }
    }
}

// ---- the despreading epilogue: unbias, symbol store, LLRs, hard bits.  Every float32 product is rounded on its own.

// One transformed element z out of LDS: scaled, conjugated back, times float(1/beta); 0 where the row or the result is not usable.
__device__ __forceinline__ cf unbias(const DftPlan& pl, cf z, float inv, bool usable) {
#pragma clang fp contract(off)
    cf x = z * pl.scale;
    x.y = -x.y;
    const cf v = x * inv;
    return (usable && soft_finite(v.x) && soft_finite(v.y)) ? v : cf{0.f, 0.f};
}

// The LLRs of the symbols u[0] and (two) u[1] with the weight wgt, to q: 16-byte stores where wide_l, scalar stores otherwise.
template <int MOD>
__device__ __forceinline__ void soft_pair(const cf (&u)[2], float wgt, bool two, bool wide_l, float* q) {
#pragma clang fp contract(off)
    float o[2][MOD];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float dr[MOD / 2], di[MOD / 2], mr, mi;
        soft_axis<MOD>(u[h].x, dr, mr);
        soft_axis<MOD>(u[h].y, di, mi);
        const bool nz = u[h].x != 0.f || u[h].y != 0.f;                     // a zero symbol is an erasure
#pragma unroll
        for (int j = 0; j < MOD / 2; ++j) {
            const float vr = wgt * dr[j], vi = wgt * di[j];
            o[h][2 * j] = (nz && soft_finite(vr) && vr != 0.f) ? vr : 0.f;    // a zero is +0
            o[h][2 * j + 1] = (nz && soft_finite(vi) && vi != 0.f) ? vi : 0.f;
        }
    }
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

// The hard bits of the cnt symbols that the epilogue left in LDS, to bits (the group's first bit or byte).  Every lane of the
// workgroup calls this: it starts with the barrier behind the symbols' LDS stores.
template <int MOD>
__device__ __forceinline__ void hard_bits_sweep(const DftPlan& pl, const cf* lds, int cnt, uint8_t* bits, int bits_mode) {
    __syncthreads();
    auto stored = [&](int e) {
        const RowRef at = row_of(e, pl.M);
        return lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)];
    };
    if (bits_mode == 2) {                                                // one bit per byte
        for (int e = threadIdx.x; e < cnt; e += DFT_THREADS) {
            const unsigned hb = hard_bits<MOD>(stored(e));
#pragma unroll
            for (int b = 0; b < MOD; ++b) bits[int64_t(e) * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
        }
    } else {                                                             // packed MSB-first: a row's bits fill bytes (host check)
        constexpr int U = MOD == 4 ? 2 : 4, NB = U * MOD / 8;              // symbols and bytes of a unit
        for (int g = threadIdx.x; g * U < cnt; g += DFT_THREADS) {
            unsigned w = 0;
#pragma unroll
            for (int h = 0; h < U; ++h) w = (w << MOD) | hard_bits<MOD>(stored(g * U + h));
#pragma unroll
            for (int b = 0; b < NB; ++b) bits[int64_t(g) * NB + b] = uint8_t(w >> (8 * (NB - 1 - b)));
        }
    }
}

// The epilogue as a sweep over the group's cnt = nrows*M transformed elements in LDS (despread_rows_kernel, despread_alloc_rows_kernel):
// t = {float(1/beta), weight, beta, usable} of the segment; osym, llr, bits point at the group's first symbol in the dense
// outputs (null: not wanted; bits at its first bit or byte).  Every lane of the workgroup calls this.
template <int MOD, bool MORE>
__device__ __forceinline__ void despread_epilogue(const DftPlan& pl, cf* lds, const int* row_nz, int cnt, float4 t, cf* osym, float* llr,
                                                  uint8_t* bits, int bits_mode) {
    const bool wide_s = (reinterpret_cast<uintptr_t>(osym) & 15) == 0, wide_l = (reinterpret_cast<uintptr_t>(llr) & 15) == 0;
    for (int e = 2 * int(threadIdx.x); e < cnt; e += 2 * DFT_THREADS) {
        const bool two = e + 1 < cnt;
        cf u[2] = {cf{0.f, 0.f}, cf{0.f, 0.f}};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 0 || two) {
                const RowRef at = row_of(e + h, pl.M);
                cf* p = &lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)];
                u[h] = unbias(pl, *p, t.x, t.w != 0.f && row_nz[at.r] != 0);
                if (MORE) *p = u[h];                                    // the hard bits read the stored symbol
            }
        }
        if (osym) store_sym_pair(osym, e, two, wide_s, u[0], u[1]);
        if constexpr (MORE) {
            if (llr) soft_pair<MOD>(u, t.y, two, wide_l, llr + int64_t(e) * MOD);
        }
    }
    if constexpr (MORE) {
        if (bits) hard_bits_sweep<MOD>(pl, lds, cnt, bits, bits_mode);
    }
}

// The epilogue by the rows' own lanes (mrc_despread_alloc_rows_kernel; mrc_despread_rows_kernel has it as text): lane l owns the pairs
// of entries 2l, 2l + 2 lanes, ...; inv = float(1/beta) (0: the row is not usable) and wgt are the lane's row's.  The pointers
// are those of despread_epilogue.  Every lane of the workgroup calls this.
template <int MOD, bool MORE>
__device__ __forceinline__ void despread_epilogue_rows(const DftPlan& pl, cf* lds, int nrows, float inv, float wgt, cf* osym, float* llr,
                                                       uint8_t* bits, int bits_mode) {
    const int M = pl.M, r = int(threadIdx.x) / pl.lanes, lane = int(threadIdx.x) - r * pl.lanes;
    if (r < nrows) {
        cf* row = lds + r * pl.row_elems;
        if (osym) osym += r * M;
        if (llr) llr += int64_t(r) * M * MOD;
        const bool wide_s = (reinterpret_cast<uintptr_t>(osym) & 15) == 0, wide_l = (reinterpret_cast<uintptr_t>(llr) & 15) == 0;
        for (int i = 2 * lane; i < M; i += 2 * pl.lanes) {
            const bool two = i + 1 < M;
            cf u[2] = {cf{0.f, 0.f}, cf{0.f, 0.f}};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 0 || two) {
                    cf* p = &row[dft_phys(i + h, pl.pad)];
                    u[h] = unbias(pl, *p, inv, inv != 0.f);
                    if (MORE) *p = u[h];                                // the hard bits read the stored symbol
                }
            }
            if (osym) store_sym_pair(osym, i, two, wide_s, u[0], u[1]);
            if constexpr (MORE) {
                if (llr) soft_pair<MOD>(u, wgt, two, wide_l, llr + int64_t(i) * MOD);
            }
        }
    }
    if constexpr (MORE) {
        if (bits) hard_bits_sweep<MOD>(pl, lds, nrows * M, bits, bits_mode);
    }
}

// ---- the per-segment weights of the despreading stage (despread_table_kernel, despread_alloc_table_kernel): step 3 of the
// contract over the M channel powers at csi, {float(1/beta), weight, beta, usable}.  A workgroup of 256: a lane adds the entries
// k = lane, lane + 256, ... in that order, block_sum adds the lanes in a fixed order, all in double.
__device__ __forceinline__ float4 segment_weights(const float* csi, int M, double rho, double sigma2, double (&sh0)[4], double (&sh1)[4]) {
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
    // the flag is "float(1/beta) is not 0", as the rows kernels test it: with rho >= 0 beta <= 1 and it is 1 for every usable segment
    return usable ? float4{inv_f, w_f, b_f, inv_f != 0.f ? 1.f : 0.f} : float4{0.f, 0.f, 0.f, 0.f};
}

// ---- the branch combiner of receive diversity: comb_add, comb_finish for both MRC kernels, the stages for mrc_despread_alloc_rows_kernel

// Steps 2 and 3 of the combiner for one branch, as mrc_add of rx_mrc.hip (a different stage: it keeps its own): t = {c, t} of
// the entry (c = 0: not usable).  Returns whether the branch takes part; one that does not leaves the sums.
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

// Branches whose loads a lane issues before any arithmetic: MRC_ROUND of rx_mrc.hip and its reasons.
constexpr int COMB_ROUND = 2;

// What a lane has added up over its entries of its row (step 6): b = A/(A+1), e = 1/(A+1), and whether a v is not 0+0j.
struct CombSums {
    double sb, se;
    int nz;
};

// The lane's share of one row: B branches M entries at p0, p0 + zb, ... with their {c, t} at tab, tab + tb, ... combined per entry
// (16-byte non-temporal loads where that branch's row is 16-byte aligned, 8-byte loads of the same values otherwise), v
// conjugated into the row's place in LDS and, where wanted, as it is to comb.  Lane l owns the pairs of entries 2l, 2l + 2 lanes,
// ..., so what it adds up, and in which order, depends on M alone.  Called by the lanes of the group's rows.
__device__ __forceinline__ CombSums combine_row(const DftPlan& pl, const cf* p0, int64_t zb, const float2* tab, int64_t tb, int B, cf* row,
                                                cf* comb) {
#pragma clang fp contract(off)
    const int M = pl.M, lane = int(threadIdx.x) % pl.lanes;
    CombSums t{0.0, 0.0, 0};
    unsigned wide_in = 0;                                                // bit b: the row is 16-byte aligned in branch b
    for (int b = 0; b < B; ++b) wide_in |= unsigned((reinterpret_cast<uintptr_t>(p0 + b * zb) & 15) == 0) << b;
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
                z0[k] = z1[k] = cf{0.f, 0.f};                            // a slot past the last branch does not take part
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
        const double A0 = m0 ? double(s0.a) : 0.0, den0 = A0 + 1.0;       // not combined: b = 0, e = 1
        t.sb += A0 / den0;
        t.se += 1.0 / den0;
        t.nz |= int(v0.x != 0.f || v0.y != 0.f);
        row[dft_phys(i, pl.pad)] = cf{v0.x, -v0.y};
        if (two) {
            const double A1 = m1 ? double(s1.a) : 0.0, den1 = A1 + 1.0;
            t.sb += A1 / den1;
            t.se += 1.0 / den1;
            t.nz |= int(v1.x != 0.f || v1.y != 0.f);
            row[dft_phys(i + 1, pl.pad)] = cf{v1.x, -v1.y};
        }
        if (comb) store_sym_pair(comb, i, two, wide_c, v0, v1);
    }
    return t;
}

// float(1/beta) (0: the row is not usable), the weight and float(beta) of the lane's row
struct RowWeights {
    float inv, wgt, beta;
};

// From the lanes' sums to their row's weights (steps 6 and 7).  The row's lanes add their sums in a butterfly inside the wave (a + b
// and b + a are the same bits, so every lane of the row ends with the same totals); a row of 128 or 256 lanes then adds its waves'
// totals in wave order: the order depends on M alone.  Every lane of the workgroup calls this, those of rows past the group's last
// with sums of zero: its barrier is also the one behind the rows of v that combine_row put into LDS.
__device__ __forceinline__ RowWeights row_weights(const DftPlan& pl, CombSums t) {
    __shared__ double part_b[DFT_THREADS / 64], part_e[DFT_THREADS / 64];   // per wave, for rows of more than 64 lanes
    __shared__ int part_nz[DFT_THREADS / 64];
    for (int off = min(pl.lanes, 64) >> 1; off > 0; off >>= 1) {
        t.sb += __shfl_xor(t.sb, off);
        t.se += __shfl_xor(t.se, off);
        t.nz |= __shfl_xor(t.nz, off);
    }
    if (pl.lanes > 64 && (threadIdx.x & 63) == 0) {
        part_b[threadIdx.x >> 6] = t.sb;
        part_e[threadIdx.x >> 6] = t.se;
        part_nz[threadIdx.x >> 6] = t.nz;
    }
    __syncthreads();
    if (pl.lanes > 64) {
        const int w0 = (int(threadIdx.x) / pl.lanes) * (pl.lanes >> 6);
        t = CombSums{part_b[w0], part_e[w0], part_nz[w0]};
        for (int k = 1; k < (pl.lanes >> 6); ++k) {
            t.sb += part_b[w0 + k];
            t.se += part_e[w0 + k];
            t.nz |= part_nz[w0 + k];
        }
    }
    const double beta = t.sb / double(pl.M), eps = t.se / double(pl.M);
    const double w = beta / eps;
    auto good = [](double x) { return fabs(x) < __builtin_inf() && x > 0.0; };
    const float inv_f = float(1.0 / beta), w_f = float(w), b_f = float(beta);
    const bool usable = t.nz != 0 && good(beta) && good(eps) && good(w) && soft_finite(inv_f) && soft_finite(w_f);
    return usable ? RowWeights{inv_f, w_f, b_f} : RowWeights{0.f, 0.f, 0.f};   // beta <= 1: a usable row has float(1/beta) >= 1
}

}  // namespace

}  // namespace ofdm
