// dft_rows_device.hpp -- what the row kernels of DFT-spread OFDM share on the device (gfx950): a group of rows staged into LDS,
// the passes of dft_mixed.hpp over them, and the paired symbol store.  Used by dft_spread.hip and
// mrc_despread.hip (9.2.16).
#pragma once
#include "ofdm_launch.hpp"
#include "dft_mixed.hpp"
#include "soft_device.hpp"

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

}  // namespace

}  // namespace ofdm
