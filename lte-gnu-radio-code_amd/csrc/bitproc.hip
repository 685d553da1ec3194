// bitproc.hip -- the bit-level stages around the channel code on the frame-batched path: CRC attach / check (TS 36.212 5.1.1,
// the generators gCRC24A, gCRC24B, gCRC16, gCRC8) and the scrambling with the length-31 Gold sequence of TS 36.211 7.2, on bits
// (transmit side) and on the sign bits of LLRs (receive side).  The definition the kernels implement is the contract in
// include/ofdm_mi355x.h; the reference has no bit-level processing, so there is nothing in it to cite.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "crc_device.hpp"
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

// ------------------------------------------------------------------------------------------ Gold sequence: the jump tables
// An LFSR state is one 31-bit word, bit i = x(n + i).  A step is linear over GF(2), so state(n) = M^n state(0); a power of M is
// kept as its 31 columns (column i = the image of the state with only bit i set) and a product with a state is the XOR of the
// columns the state's bits select.  One table set serves the kernels (as __constant__ memory) and ofdm_gold_bits (on the host).
template <int WHICH>                                         // bit k = x(n + 31 + k) for the k with every tap inside y
__host__ __device__ constexpr uint32_t gold_feedback(uint32_t y) {
    return WHICH == 1 ? y ^ (y >> 3) : y ^ (y >> 1) ^ (y >> 2) ^ (y >> 3);
}
template <int WHICH>
constexpr uint32_t gold_step(uint32_t s) { return (s >> 1) | ((gold_feedback<WHICH>(s) & 1u) << 30); }
__host__ __device__ constexpr uint32_t gold_apply(const uint32_t* col, uint32_t s) {
    uint32_t r = 0u;
    for (int i = 0; i < 31; ++i) r ^= (0u - ((s >> i) & 1u)) & col[i];
    return r;
}

struct GoldTables {
    uint32_t j1[GOLD_LEVELS][31];        // M1^(GOLD_CH * 2^k)
    uint32_t j2[GOLD_LEVELS][31];        // M2^(GOLD_CH * 2^k)
    uint32_t a2[31];                     // M2^1600: c_init -> the x2 state at n = 0 of c
    uint32_t x1_start;                   // M1^1600 applied to x1(0) = 1
};

constexpr void gold_square(const uint32_t* in, uint32_t* out) {
    for (int i = 0; i < 31; ++i) out[i] = gold_apply(in, in[i]);
}
template <int WHICH>
constexpr void gold_fill(uint32_t (*jump)[31], uint32_t* at1600) {
    uint32_t p[31] = {}, q[31] = {}, acc[31] = {};
    for (int i = 0; i < 31; ++i) {
        p[i] = gold_step<WHICH>(1u << i);                    // M
        acc[i] = 1u << i;                                    // identity
    }
    int log_ch = 0;
    while ((1 << log_ch) < GOLD_CH) ++log_ch;
    for (int bit = 0; bit < log_ch + GOLD_LEVELS; ++bit) {   // p = M^(2^bit)
        if ((1600 >> bit) & 1) {
            for (int i = 0; i < 31; ++i) q[i] = gold_apply(p, acc[i]);
            for (int i = 0; i < 31; ++i) acc[i] = q[i];
        }
        if (bit >= log_ch)
            for (int i = 0; i < 31; ++i) jump[bit - log_ch][i] = p[i];
        gold_square(p, q);
        for (int i = 0; i < 31; ++i) p[i] = q[i];
    }
    for (int i = 0; i < 31; ++i) at1600[i] = acc[i];
}
constexpr GoldTables gold_make_tables() {
    GoldTables t{};
    uint32_t m1[31] = {};
    gold_fill<1>(t.j1, m1);
    gold_fill<2>(t.j2, t.a2);
    t.x1_start = m1[0];
    return t;
}
static_assert((GOLD_CH & (GOLD_CH - 1)) == 0 && GOLD_CH % 32 == 0, "a lane's share is a power of two of whole words");
static_assert((int64_t(GOLD_CH) << GOLD_LEVELS) >= (int64_t(1) << 31), "the tables reach the top of the index range");

constexpr GoldTables GOLD_HOST = gold_make_tables();
__constant__ GoldTables gold_dev = gold_make_tables();

// c(n .. n+31), bit i = c(n + i), from the two states at n; both advance by 32.  28 new bits come from one shifted XOR of the
// state, the next 5 from the same expression on what is then known (x(n + 28 ..)).
template <int WHICH>
__host__ __device__ __forceinline__ uint32_t gold_next32(uint32_t& s) {
    uint64_t x = uint64_t(s) | (uint64_t(gold_feedback<WHICH>(s) & 0x0fffffffu) << 31);      // x(n .. n+58)
    x |= uint64_t(gold_feedback<WHICH>(uint32_t(x >> 28)) & 0x1fu) << 59;                     // x(n+59 .. n+63)
    s = uint32_t(x >> 32) & 0x7fffffffu;
    return uint32_t(x);
}
__host__ __device__ __forceinline__ uint32_t gold_word(uint32_t& s1, uint32_t& s2) { return gold_next32<1>(s1) ^ gold_next32<2>(s2); }

// advances both states by GOLD_CH * (the bits first_level .. last_level - 1 of chunk)
__host__ __device__ __forceinline__ void gold_jump(const GoldTables& t, uint32_t chunk, int first_level, int last_level, uint32_t& s1,
                                                   uint32_t& s2) {
#pragma unroll 1
    for (int k = first_level; k < last_level; ++k)
        if ((chunk >> k) & 1u) {
            s1 = gold_apply(t.j1[k], s1);
            s2 = gold_apply(t.j2[k], s2);
        }
}

// ------------------------------------------------------------------------------------------ scrambling kernels
// One wave per workgroup; the wave owns GOLD_SPAN = 64 * GOLD_CH consecutive bits of one segment.  Phase 1: lane l jumps to bit
// l * GOLD_CH of the span (the span's part of the jump is wave-uniform and runs on the scalar unit, the lane's part is
// log2(64) levels) and writes its GOLD_CH sequence bits as words into LDS.  Phase 2: the wave streams the span's elements with
// consecutive lanes on consecutive vectors of four (float4 / one word of four bit-bytes) or on consecutive words of 32 packed
// bits; a vector's four sequence bits are one nibble of an LDS word that eight neighbouring lanes share (a broadcast read).
enum : int { GOLD_MODE_LLR = 0, GOLD_MODE_BYTES = 1, GOLD_MODE_PACKED = 2 };

// 32 sequence bits as four packed bytes in memory order (the first bit is the MSB of the first byte)
__device__ __forceinline__ uint32_t gold_packed_word(uint32_t w) { return __builtin_bswap32(__brev(w)); }

template <int MODE>
__global__ void __launch_bounds__(64) gold_apply_kernel(GoldArgs a) {
    __shared__ uint32_t seq[GOLD_SPAN / 32];
    const int lane = int(threadIdx.x);
    const int64_t span0 = int64_t(blockIdx.x) * GOLD_SPAN;               // first bit of this span inside its segment
    const int n = int(std::min<int64_t>(GOLD_SPAN, a.seg_bits - span0)); // > 0: the grid's x is ceil(seg_bits / GOLD_SPAN)
    for (int64_t seg = blockIdx.y; seg < a.n_seg; seg += gridDim.y) {
        // ---- phase 1
        uint32_t s1 = gold_dev.x1_start, s2 = gold_apply(gold_dev.a2, a.cinit[seg] & 0x7fffffffu);
        gold_jump(gold_dev, uint32_t(blockIdx.x) << 6, 6, GOLD_LEVELS, s1, s2);         // wave-uniform: the span's first chunk
        if (lane * GOLD_CH < n) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if ((lane >> k) & 1) {
                    s1 = gold_apply(gold_dev.j1[k], s1);
                    s2 = gold_apply(gold_dev.j2[k], s2);
                }
            const int words = std::min(GOLD_CH / 32, (n - lane * GOLD_CH + 31) >> 5);
            for (int r = 0; r < words; ++r) seq[lane * (GOLD_CH / 32) + r] = gold_word(s1, s2);
        }
        __syncthreads();
        // ---- phase 2
        if constexpr (MODE == GOLD_MODE_LLR) {
            const uint32_t* in = reinterpret_cast<const uint32_t*>(a.in) + seg * a.in_stride + span0;
            uint32_t* out = reinterpret_cast<uint32_t*>(a.out) + seg * a.out_stride + span0;
            if (((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0) {
                const int nvec = n >> 2;
#pragma unroll 4
                for (int v = lane; v < nvec; v += 64) {
                    uint4 x = reinterpret_cast<const uint4*>(in)[v];
                    const uint32_t nib = seq[v >> 3] >> ((v & 7) << 2);
                    x.x ^= nib << 31;
                    x.y ^= (nib >> 1) << 31;
                    x.z ^= (nib >> 2) << 31;
                    x.w ^= (nib >> 3) << 31;
                    reinterpret_cast<uint4*>(out)[v] = x;
                }
                const int e = (nvec << 2) + lane;                        // the tail behind the last whole vector
                if (lane < (n & 3)) out[e] = in[e] ^ ((seq[e >> 5] >> (e & 31)) << 31);
            } else {
                for (int e = lane; e < n; e += 64) out[e] = in[e] ^ ((seq[e >> 5] >> (e & 31)) << 31);
            }
        } else if constexpr (MODE == GOLD_MODE_BYTES) {
            const uint8_t* in = static_cast<const uint8_t*>(a.in) + seg * a.in_stride + span0;
            uint8_t* out = static_cast<uint8_t*>(a.out) + seg * a.out_stride + span0;
            if (((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0) {
                const int nvec = n >> 2;
#pragma unroll 4
                for (int v = lane; v < nvec; v += 64) {
                    const uint32_t x = reinterpret_cast<const uint32_t*>(in)[v] & 0x01010101u;
                    reinterpret_cast<uint32_t*>(out)[v] = x ^ gold_spread4((seq[v >> 3] >> ((v & 7) << 2)) & 0xfu);
                }
                const int e = (nvec << 2) + lane;
                if (lane < (n & 3)) out[e] = uint8_t((in[e] ^ (seq[e >> 5] >> (e & 31))) & 1u);
            } else {
                for (int e = lane; e < n; e += 64) out[e] = uint8_t((in[e] ^ (seq[e >> 5] >> (e & 31))) & 1u);
            }
        } else {
            const int nbytes = n >> 3;                                   // seg_bits % 8 == 0
            const uint8_t* in = static_cast<const uint8_t*>(a.in) + seg * a.in_stride + (span0 >> 3);
            uint8_t* out = static_cast<uint8_t*>(a.out) + seg * a.out_stride + (span0 >> 3);
            if (((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0) {
                const int nvec = nbytes >> 2;
                for (int v = lane; v < nvec; v += 64)
                    reinterpret_cast<uint32_t*>(out)[v] = reinterpret_cast<const uint32_t*>(in)[v] ^ gold_packed_word(seq[v]);
                const int e = (nvec << 2) + lane;
                if (lane < (nbytes & 3)) out[e] = uint8_t(in[e] ^ (gold_packed_word(seq[e >> 2]) >> ((e & 3) << 3)));
            } else {
                for (int e = lane; e < nbytes; e += 64) out[e] = uint8_t(in[e] ^ (gold_packed_word(seq[e >> 2]) >> ((e & 3) << 3)));
            }
        }
        __syncthreads();                                                 // the next segment overwrites seq
    }
}

// ------------------------------------------------------------------------------------------ CRC
// generators, table step and the byte load / store of both layouts: crc_device.hpp (shared with tb.hip and the host calls)

// One lane per block: the remainder of the first A bits through the byte-wise table of the call's generator, which the
// workgroup builds in LDS (256 threads, one entry each).  ATTACH: copies the payload into the block (either layout to either
// layout) and appends parity ^ mask.  Otherwise: syndrome = remainder ^ received parity, ok = (syndrome == mask), and the
// payload compacted -- each of the three only where its pointer is given.
template <bool ATTACH>
__global__ void __launch_bounds__(256) crc_kernel(CrcArgs a) {
    __shared__ uint32_t table[256];
    const int L = crc_len(a.kind);
    table[threadIdx.x] = crc_table_entry(crc_poly(a.kind), L, threadIdx.x);
    __syncthreads();
    const int64_t b = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (b >= a.n_blocks) return;
    const int nA = a.A >> 3, nL = L >> 3, K = a.A + L;
    const bool info_packed = a.info_mode == 1, pay_packed = a.payload_mode == 1;
    const uint32_t lmask = (1u << L) - 1u;
    const uint32_t mask = (a.mask_dev ? a.mask_dev[b] : a.mask) & lmask;
    if constexpr (ATTACH) {
        const uint8_t* src = a.payload_in + b * (pay_packed ? nA : a.A);
        uint8_t* dst = a.info_out + b * (info_packed ? K >> 3 : K);
        const bool src_wide = (reinterpret_cast<uintptr_t>(src) & 7u) == 0, dst_wide = (reinterpret_cast<uintptr_t>(dst) & 7u) == 0;
        uint32_t reg = 0u;
        for (int i = 0; i < nA; ++i) {
            const uint32_t v = crc_load_byte(src, pay_packed, src_wide, i);
            reg = crc_byte(reg, table[crc_index(reg, v, L)], L);
            crc_store_byte(dst, info_packed, dst_wide, i, v);
        }
        reg ^= mask;
        for (int i = 0; i < nL; ++i) crc_store_byte(dst, info_packed, dst_wide, nA + i, (reg >> (L - 8 - 8 * i)) & 0xffu);
    } else {
        const uint8_t* src = a.info_in + b * (info_packed ? K >> 3 : K);
        uint8_t* dst = a.payload_out ? a.payload_out + b * (pay_packed ? nA : a.A) : nullptr;
        const bool src_wide = (reinterpret_cast<uintptr_t>(src) & 7u) == 0, dst_wide = (reinterpret_cast<uintptr_t>(dst) & 7u) == 0;
        uint32_t reg = 0u;
        for (int i = 0; i < nA; ++i) {
            const uint32_t v = crc_load_byte(src, info_packed, src_wide, i);
            reg = crc_byte(reg, table[crc_index(reg, v, L)], L);
            if (dst) crc_store_byte(dst, pay_packed, dst_wide, i, v);
        }
        uint32_t parity = 0u;
        for (int i = 0; i < nL; ++i) parity = (parity << 8) | crc_load_byte(src, info_packed, src_wide, nA + i);
        const uint32_t syn = reg ^ parity;
        if (a.syndrome) a.syndrome[b] = syn;
        if (a.ok) a.ok[b] = syn == mask ? 1 : 0;
    }
}

template <int MODE>
hipError_t gold_launch(const GoldArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.seg_bits <= 0) return hipSuccess;
    const dim3 grid(unsigned((a.seg_bits + GOLD_SPAN - 1) / GOLD_SPAN), unsigned(std::min<int64_t>(a.n_seg, 65535)));
    hipLaunchKernelGGL(gold_apply_kernel<MODE>, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace

int crc_bits(int kind) { return kind >= 0 && kind < 4 ? crc_len(kind) : 0; }

uint32_t crc_host(int kind, const uint8_t* bits_packed, int A) {
    const int L = crc_len(kind);
    uint32_t reg = 0u;
    for (int i = 0; i < (A >> 3); ++i) {
        const uint32_t v = bits_packed[i];
        reg = crc_byte(reg, crc_table_entry(crc_poly(kind), L, crc_index(reg, v, L)), L);
    }
    return reg;
}

void gold_bits_host(uint32_t c_init, int64_t first, int64_t n, uint8_t* out) {
    uint32_t s1 = GOLD_HOST.x1_start, s2 = gold_apply(GOLD_HOST.a2, c_init & 0x7fffffffu);
    gold_jump(GOLD_HOST, uint32_t(first / GOLD_CH), 0, GOLD_LEVELS, s1, s2);
    int64_t skip = first % GOLD_CH, done = 0;
    while (done < n) {
        const uint32_t w = gold_word(s1, s2);
        for (int i = 0; i < 32 && done < n; ++i) {
            if (skip > 0)
                --skip;
            else
                out[done++] = uint8_t((w >> i) & 1u);
        }
    }
}

hipError_t launch_gold_llr(const GoldArgs& a, hipStream_t s) { return gold_launch<GOLD_MODE_LLR>(a, s); }
hipError_t launch_gold_bits(const GoldArgs& a, int packed, hipStream_t s) {
    return packed ? gold_launch<GOLD_MODE_PACKED>(a, s) : gold_launch<GOLD_MODE_BYTES>(a, s);
}

hipError_t launch_crc(const CrcArgs& a, hipStream_t s) {
    if (a.n_blocks <= 0) return hipSuccess;
    const dim3 grid(unsigned((a.n_blocks + 255) / 256));
    if (a.info_out)
        hipLaunchKernelGGL(crc_kernel<true>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(crc_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t bitproc_prepare() {
    return load_kernels(gold_apply_kernel<GOLD_MODE_LLR>, gold_apply_kernel<GOLD_MODE_BYTES>, gold_apply_kernel<GOLD_MODE_PACKED>,
                        crc_kernel<true>, crc_kernel<false>);
}

}  // namespace ofdm
