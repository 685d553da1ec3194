// dft_rows_device.hpp -- what the row kernels of DFT-spread OFDM share on the device (gfx950): a group of rows staged into LDS,
// the passes of dft_mixed.hpp over them, and the paired symbol store.  Used by dft_spread.hip and
// mrc_despread.hip (9.2.16); dft_alloc.hip (9.2.17) adds the strided staging and the despreading epilogue as a function.
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

// The epilogue of the despreading stage over the cnt = nrows*M transformed elements in LDS, exactly the arithmetic and the
// stores of despread_rows_kernel (dft_spread.hip): t = {float(1/beta), weight, beta, usable} of the segment; osym, llr, bits
// point at the group's first symbol in the dense outputs (null: not wanted).  Every lane of the workgroup calls this.
template <int MOD, bool MORE>
__device__ __forceinline__ void despread_epilogue(const DftPlan& pl, cf* lds, const int* row_nz, int cnt, float4 t, cf* osym, float* llr,
                                                  uint8_t* bits, int bits_mode) {
#pragma clang fp contract(off)
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
        if (bits) {
            __syncthreads();
            auto stored = [&](int e) {
                const RowRef at = row_of(e, pl.M);
                return lds[at.r * pl.row_elems + dft_phys(at.i, pl.pad)];
            };
            if (bits_mode == 2) {                                        // one bit per byte
                for (int e = threadIdx.x; e < cnt; e += DFT_THREADS) {
                    const unsigned hb = hard_bits<MOD>(stored(e));
#pragma unroll
                    for (int b = 0; b < MOD; ++b) bits[int64_t(e) * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
                }
            } else {                                                     // packed MSB-first: a row's bits fill bytes (host check)
                constexpr int U = MOD == 4 ? 2 : 4, NB = U * MOD / 8;      // symbols and bytes of a unit
                for (int g = threadIdx.x; g * U < cnt; g += DFT_THREADS) {
                    unsigned w = 0;
#pragma unroll
                    for (int h = 0; h < U; ++h) w = (w << MOD) | hard_bits<MOD>(stored(g * U + h));
#pragma unroll
                    for (int b = 0; b < NB; ++b) bits[int64_t(g) * NB + b] = uint8_t(w >> (8 * (NB - 1 - b)));
                }
            }
        }
    }
}

}  // namespace

}  // namespace ofdm
