// tb.hip -- the transport-block layer around the turbo code on the frame-batched path: CRC24A over the transport block
// (TS 36.212 5.1.1), segmentation into code blocks with a CRC24B each (5.1.2), concatenation of the rate-matched blocks (5.1.5)
// and the way back.  The definition the kernels implement is the contract in include/ofdm_mi355x.h; the
// reference has no bit-level processing, so there is nothing in it to cite.  The CRCs of blocks of up to 2^20 bits go through the
// chunk-and-combine routine of crc_device.hpp: a lane takes a run of bytes through the byte table in LDS, multiplies its
// remainder by x^(8 bytes behind the run) mod g, and the terms are XORed by shuffles -- no atomics, and the same value for
// every chunking.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "crc_device.hpp"
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

constexpr uint32_t POLY_A = crc_poly(0), POLY_B = crc_poly(1);
constexpr int TB_WAVES = TB_THREADS / 64;

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= uint32_t(__shfl_xor(int(v), m, 64));
    return v;
}

// the XOR of every thread's value; red is TB_WAVES words of LDS that no other use overlaps
__device__ __forceinline__ uint32_t workgroup_xor(uint32_t v, uint32_t* red) {
    v = wave_xor(v);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0u;
#pragma unroll
    for (int w = 0; w < TB_WAVES; ++w) r ^= red[w];
    __syncthreads();
    return r;
}

// code block r of transport block t inside the workspace
__device__ __forceinline__ uint8_t* tb_block(const TbSegArgs& a, int64_t t, int r) {
    int g = 0;
    if (a.n_ranges > 1 && r >= a.range[1].first) g = 1;
    if (a.n_ranges > 2 && r >= a.range[2].first) g = 2;
    const TbRange& x = a.range[g];
    return a.ws + x.base + (t * x.count + (r - x.first)) * int64_t(x.kbytes);
}
__device__ __forceinline__ int tb_block_bytes(const TbSeg& g, int r) { return r < g.Cm ? g.Km8 : g.Kp8; }
// bytes of the filler-prefixed sequence (F8 zeros, then the B-bit sequence) in front of block r
__device__ __forceinline__ int tb_block_start(const TbSeg& g, int r) {
    return r <= g.Cm ? r * (g.Km8 - g.L8) : g.Cm * (g.Km8 - g.L8) + (r - g.Cm) * (g.Kp8 - g.L8);
}
// byte p of the filler-prefixed sequence sits in block r at byte off
__device__ __forceinline__ void tb_locate(const TbSeg& g, int p, int& r, int& off) {
    const int nm = g.Cm * (g.Km8 - g.L8);
    if (p < nm) {
        r = p / (g.Km8 - g.L8);
        off = p - r * (g.Km8 - g.L8);
    } else {
        const int q = (p - nm) / (g.Kp8 - g.L8);
        r = g.Cm + q;
        off = (p - nm) - q * (g.Kp8 - g.L8);
    }
}

// One workgroup per transport block.  CRC24A over the payload (256 runs), then every byte of every code block that is not a
// CRC24B -- filler, payload, CRC24A -- by the thread that owns it, then one wave per code block for its CRC24B (64 runs over
// the same source bytes, filler zeros included).
__global__ void __launch_bounds__(TB_THREADS) tb_segment_kernel(TbSegArgs a) {
    __shared__ uint32_t tab_a[256], tab_b[256], red[TB_WAVES];
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    tab_a[tid] = crc_table_entry(POLY_A, 24, uint32_t(tid));
    tab_b[tid] = crc_table_entry(POLY_B, 24, uint32_t(tid));
    __syncthreads();
    const TbSeg g = a.g;
    const int64_t t = blockIdx.x;
    const bool packed = a.payload_mode == 1;
    const uint8_t* src = a.payload_in + t * (packed ? int64_t(g.A8) : 8 * int64_t(g.A8));
    const bool wide = (reinterpret_cast<uintptr_t>(src) & 7u) == 0;
    const uint32_t crc_a = workgroup_xor(crc_chunk_term(POLY_A, 24, uint32_t(g.A8), uint32_t(TB_THREADS), uint32_t(tid),
                                                        [&](uint32_t k) { return crc_load_byte(src, packed, wide, int(k)); },
                                                        [&](uint32_t i) { return tab_a[i]; }), red);
    // byte p of the filler-prefixed sequence: filler, payload, then the three bytes of CRC24A
    auto seq = [&](int p) -> uint32_t {
        const int s = p - g.F8;
        if (s < 0) return 0u;
        return s < g.A8 ? crc_load_byte(src, packed, wide, s) : (crc_a >> (16 - 8 * (s - g.A8))) & 0xffu;
    };
    const int bytes_m = g.Cm * g.Km8, total = bytes_m + (g.C - g.Cm) * g.Kp8;
    for (int o = tid; o < total; o += TB_THREADS) {
        int r, off, kb;
        if (o < bytes_m) {
            kb = g.Km8;
            r = o / kb;
            off = o - r * kb;
        } else {
            kb = g.Kp8;
            const int q = (o - bytes_m) / kb;
            r = g.Cm + q;
            off = (o - bytes_m) - q * kb;
        }
        if (off < kb - g.L8) tb_block(a, t, r)[off] = uint8_t(seq(tb_block_start(g, r) + off));
    }
    if (g.L8) {
        for (int r = wave; r < g.C; r += TB_WAVES) {
            const int n = tb_block_bytes(g, r) - 3, p0 = tb_block_start(g, r);
            const uint32_t crc_b = wave_xor(crc_chunk_term(POLY_B, 24, uint32_t(n), 64u, uint32_t(lane),
                                                           [&](uint32_t k) { return seq(p0 + int(k)); }, [&](uint32_t i) { return tab_b[i]; }));
            if (lane < 3) tb_block(a, t, r)[n + lane] = uint8_t(crc_b >> (16 - 8 * lane));
        }
    }
}

// One workgroup per transport block, over the decoder's packed bits: one wave per code block for its CRC24B, the payload bytes
// each by the thread that owns them, then CRC24A over the re-joined sequence (256 runs).
__global__ void __launch_bounds__(TB_THREADS) tb_desegment_kernel(TbSegArgs a) {
    __shared__ uint32_t tab_a[256], tab_b[256], red[TB_WAVES];
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    tab_a[tid] = crc_table_entry(POLY_A, 24, uint32_t(tid));
    tab_b[tid] = crc_table_entry(POLY_B, 24, uint32_t(tid));
    __syncthreads();
    const TbSeg g = a.g;
    const int64_t t = blockIdx.x;
    if (a.cb_ok) {
        if (g.L8) {
            for (int r = wave; r < g.C; r += TB_WAVES) {
                const uint8_t* blk = tb_block(a, t, r);
                const int n = tb_block_bytes(g, r) - 3;
                const uint32_t crc_b = wave_xor(crc_chunk_term(POLY_B, 24, uint32_t(n), 64u, uint32_t(lane),
                                                               [&](uint32_t k) { return uint32_t(blk[k]); }, [&](uint32_t i) { return tab_b[i]; }));
                const uint32_t parity = (uint32_t(blk[n]) << 16) | (uint32_t(blk[n + 1]) << 8) | uint32_t(blk[n + 2]);
                if (lane == 0) a.cb_ok[t * g.C + r] = crc_b == parity ? 1 : 0;
            }
        } else if (tid == 0) {
            a.cb_ok[t] = 1;
        }
    }
    // byte s of the re-joined B-bit sequence
    auto joined = [&](uint32_t s) -> uint32_t {
        int r, off;
        tb_locate(g, int(s) + g.F8, r, off);
        return tb_block(a, t, r)[off];
    };
    if (a.payload_out) {
        const bool packed = a.payload_mode == 1;
        uint8_t* dst = a.payload_out + t * (packed ? int64_t(g.A8) : 8 * int64_t(g.A8));
        const bool wide = (reinterpret_cast<uintptr_t>(dst) & 7u) == 0;
        for (int s = tid; s < g.A8; s += TB_THREADS) crc_store_byte(dst, packed, wide, s, joined(uint32_t(s)));
    }
    if (a.tb_ok || a.syndrome) {
        const uint32_t crc_a = workgroup_xor(crc_chunk_term(POLY_A, 24, uint32_t(g.A8), uint32_t(TB_THREADS), uint32_t(tid), joined,
                                                            [&](uint32_t i) { return tab_a[i]; }), red);
        if (tid == 0) {
            const uint32_t parity = (joined(uint32_t(g.A8)) << 16) | (joined(uint32_t(g.A8) + 1u) << 8) | joined(uint32_t(g.A8) + 2u);
            const uint32_t syn = crc_a ^ parity;
            if (a.syndrome) a.syndrome[t] = syn;
            if (a.tb_ok) a.tb_ok[t] = syn == 0u ? 1 : 0;
        }
    }
}

// One thread per output byte of the codeword: a bit (one bit per byte) or eight bits (packed), each gathered from its group's
// encoder output; zeros from bit G on.
__global__ void __launch_bounds__(256) tb_concat_kernel(TbConcatArgs a) {
    const bool packed = a.cw_mode == 1;
    const int64_t row = packed ? a.cw_bits >> 3 : a.cw_bits;
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= row) return;
    auto bit = [&](int64_t t, int64_t n) -> uint32_t {
        if (n >= a.G) return 0u;
        int g = 0;
        if (a.n_groups > 1 && n >= a.off[1]) g = 1;
        if (a.n_groups > 2 && n >= a.off[2]) g = 2;
        return a.ws[a.base[g] + t * a.bits[g] + (n - a.off[g])] & 1u;
    };
    for (int64_t t = blockIdx.y; t < a.n_tb; t += gridDim.y) {
        uint32_t v;
        if (packed) {
            v = 0u;
#pragma unroll
            for (int x = 0; x < 8; ++x) v |= bit(t, 8 * i + x) << (7 - x);
        } else {
            v = bit(t, i);
        }
        a.cw[t * row + i] = uint8_t(v);
    }
}

}  // namespace

uint32_t crc_long_host(int kind, const uint8_t* bits_packed, int64_t n_bytes) {
    const uint32_t poly = crc_poly(kind);
    const int L = crc_len(kind);
    uint32_t table[256], crc = 0u;
    for (uint32_t v = 0; v < 256u; ++v) table[v] = crc_table_entry(poly, L, v);
    for (uint32_t i = 0; i < uint32_t(TB_THREADS); ++i)
        crc ^= crc_chunk_term(poly, L, uint32_t(n_bytes), uint32_t(TB_THREADS), i, [&](uint32_t k) { return uint32_t(bits_packed[k]); },
                              [&](uint32_t v) { return table[v]; });
    return crc;
}

hipError_t launch_tb_segment(const TbSegArgs& a, hipStream_t s) {
    if (a.n_tb <= 0) return hipSuccess;
    hipLaunchKernelGGL(tb_segment_kernel, dim3(unsigned(a.n_tb)), dim3(TB_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tb_desegment(const TbSegArgs& a, hipStream_t s) {
    if (a.n_tb <= 0) return hipSuccess;
    hipLaunchKernelGGL(tb_desegment_kernel, dim3(unsigned(a.n_tb)), dim3(TB_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tb_concat(const TbConcatArgs& a, hipStream_t s) {
    const int64_t row = a.cw_mode == 1 ? a.cw_bits >> 3 : a.cw_bits;
    if (a.n_tb <= 0 || row <= 0) return hipSuccess;
    const dim3 grid(unsigned((row + 255) / 256), unsigned(std::min<int64_t>(a.n_tb, 65535)));
    hipLaunchKernelGGL(tb_concat_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t tb_prepare() { return load_kernels(tb_segment_kernel, tb_desegment_kernel, tb_concat_kernel); }

}  // namespace ofdm
