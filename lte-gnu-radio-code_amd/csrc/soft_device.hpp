// soft_device.hpp -- device helpers the soft-output stages share (gfx950): rx_demap.hip (segmented soft de-mapper), rx_csi.hip
// (channel-state-weighted LLRs) and rx_mrc.hip (receive-diversity combining).  Every helper is inlined into its caller.  There is
// NO file-scope fp-contract pragma here: the flat de-mappers of rx_demap.hip are compiled with contraction allowed, so each
// arithmetic helper switches it off inside its own body.
#pragma once
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

__device__ __forceinline__ bool soft_finite(float x) { return fabsf(x) < __builtin_inff(); }

// 16-byte / 8-byte non-temporal load of data a kernel reads once, store of data it writes once and does not read again
__device__ __forceinline__ float4 load_stream16(const float* p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p));
    return float4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void store_stream16(float* p, float4 v) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(f4{v.x, v.y, v.z, v.w}, reinterpret_cast<f4*>(p));
}
__device__ __forceinline__ float2 load_stream8(const float* p) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = __builtin_nontemporal_load(reinterpret_cast<const f2*>(p));
    return float2{v.x, v.y};
}
__device__ __forceinline__ void store_stream8(float* p, float2 v) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(f2{v.x, v.y}, reinterpret_cast<f2*>(p));
}

// row position after a step: j < 2 * rl on entry
__device__ __forceinline__ int row_wrap(int j, int rl) { return j >= rl ? j - rl : j; }

// One axis of the max-log rule on squared distances (channel-state-weighted LLRs and the combiner behind them):
// d[j] = min over the levels with axis bit j = 1 of (x-l)^2 minus the same over bit j = 0, and m = the smallest (x-l)^2 of all.
// Levels and labels are those of rx_demap.hip: +-0.70710678 for QPSK (bit 0 <-> the positive level), else
// l_q = float(2q - (M-1)) * u with the TS 36.211 7.1 labels of Pam<BPS>.  Every product and difference is rounded on its own.
template <int MOD>
__device__ __forceinline__ void soft_axis(float x, float (&d)[MOD / 2], float& m) {
#pragma clang fp contract(off)
    if constexpr (MOD == 2) {
        constexpr float c = 0.70710678118654752f;
        const float p = (x - c) * (x - c), n = (x - (-c)) * (x - (-c));
        d[0] = n - p;
        m = fminf(p, n);
    } else {
        constexpr int M = MOD == 4 ? 4 : 8, NB = MOD / 2;
        const float u = MOD == 4 ? 0.31622776601683794f : 0.15430334996209191f;
        float m0[NB], m1[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) m0[j] = m1[j] = __builtin_inff();
#pragma unroll
        for (int q = 0; q < M; ++q) {
            const int lv = 2 * q - (M - 1), am = lv < 0 ? -lv : lv;
            const float l = float(lv) * u;
            const float e = (x - l) * (x - l);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const bool one = j == 0 ? lv < 0 : (MOD == 4 ? am == 3 : (j == 1 ? am > 4 : (am == 1 || am == 7)));
                if (one)
                    m1[j] = fminf(m1[j], e);
                else
                    m0[j] = fminf(m0[j], e);
            }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) d[j] = m1[j] - m0[j];
        m = fminf(m0[0], m1[0]);
    }
}

// Sums over the workgroup (256 lanes) in a fixed order: butterfly per wave, then the four wave sums; every lane gets the totals.
// The caller puts a barrier between two uses of the same arrays.
__device__ __forceinline__ double block_sum(double v, double (&sh)[4]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ void block_sum(double& v, long long& n, double (&sh)[4], long long (&shn)[4]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        v += __shfl_xor(v, m, 64);
        n += __shfl_xor(n, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6] = v;
        shn[threadIdx.x >> 6] = n;
    }
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    n = (shn[0] + shn[1]) + (shn[2] + shn[3]);
}

// 64-QAM tile store: tile t of a slice's output array `out` is 128 symbols = 768 floats, of which lane (0..63) holds the 6 of
// symbol 2*lane (x) and the 6 of symbol 2*lane + 1 (y).  They go through the wave's 3 KB of LDS `st` in symbol order -- 12 floats
// per lane in -- and out as 3 x 16 B per lane, piece k*64 + lane per store instruction: each writes 1 KB contiguous, once,
// non-temporal.  `st` is private to the wave and LDS is in order per wave: two counter waits, no barrier.
__device__ __forceinline__ void store_tile64(float* out, int t, int lane, float* st, const float (&x)[6], const float (&y)[6]) {
    float4* wr = reinterpret_cast<float4*>(st + lane * 12);
    wr[0] = float4{x[0], x[1], x[2], x[3]};
    wr[1] = float4{x[4], x[5], y[0], y[1]};
    wr[2] = float4{y[2], y[3], y[4], y[5]};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                    // wave-local exchange: in order per wave
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int piece = k * 64 + lane;
        store_stream16(out + int64_t(t) * 768 + 4 * piece, *reinterpret_cast<const float4*>(st + 4 * piece));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                    // reads done before the stage is rewritten
}

}  // namespace

}  // namespace ofdm
