// crc_device.hpp -- the CRC arithmetic that bitproc.hip (one lane per short block), tb.hip (a workgroup or a wave per long
// block) and the host calls ofdm_crc_compute / ofdm_crc_compute_long share: the generators of TS 36.212 5.1.1, the byte-wise
// table step, the byte load / store of both bit layouts, and the chunk-and-combine construction for blocks that are too long for
// one lane.  Contract: include/ofdm_mi355x.h ("CRC and scrambling", "transport block"); DESIGN.md 9.2.5 and 9.2.8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ofdm {

__host__ __device__ constexpr uint32_t crc_poly(int kind) { return kind == 0 ? 0x1864CFBu : kind == 1 ? 0x1800063u : kind == 2 ? 0x11021u : 0x19Bu; }
__host__ __device__ constexpr int crc_len(int kind) { return kind <= 1 ? 24 : kind == 2 ? 16 : 8; }

// remainder of v * D^L, v one byte: the entry of the byte-wise table
__host__ __device__ constexpr uint32_t crc_table_entry(uint32_t poly, int L, uint32_t v) {
    uint32_t reg = v << (L - 8);
    for (int i = 0; i < 8; ++i) {
        const uint32_t top = (reg >> (L - 1)) & 1u;
        reg = (reg << 1) ^ (top ? poly : 0u);
    }
    return reg & ((1u << L) - 1u);
}
// one byte further: reg' = (reg << 8 mod D^L) ^ table[crc_index(reg, byte)]
__host__ __device__ __forceinline__ uint32_t crc_byte(uint32_t reg, uint32_t entry, int L) { return ((reg << 8) & ((1u << L) - 1u)) ^ entry; }
__host__ __device__ __forceinline__ uint32_t crc_index(uint32_t reg, uint32_t byte, int L) { return ((reg >> (L - 8)) ^ byte) & 0xffu; }

// ---- chunk and combine.  The register starts at zero and nothing is XORed at the end, so the CRC is linear over GF(2):
// crc(M1 || M2) = crc(M1) x^|M2| mod g  ^  crc(M2).  A message of n bytes is cut into `parts` runs; run i is bytes
// [i per, min((i+1) per, n)) with per = ceil(n / parts), and its term is (remainder of the run alone) x^(8 bytes behind it) mod g.
// The CRC is the XOR of the terms, whatever `parts` is.
// a b mod g for a, b below 2^L: b's bits from the top, one shift-and-reduce of the sum and one conditional add each
__host__ __device__ constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b, uint32_t poly, int L) {
    uint32_t r = 0u;
    for (int i = L - 1; i >= 0; --i) {
        r = ((r << 1) ^ (((r >> (L - 1)) & 1u) ? poly : 0u)) & ((1u << L) - 1u);
        r ^= (0u - ((b >> i) & 1u)) & a;
    }
    return r;
}
// x^(8 nbytes) mod g by square-and-multiply over the bits of nbytes
__host__ __device__ constexpr uint32_t crc_xpow_bytes(uint32_t poly, int L, uint32_t nbytes) {
    uint32_t sq = 1u;                                        // x^8 mod g: eight shift-and-reduce steps of 1
    for (int i = 0; i < 8; ++i) sq = ((sq << 1) ^ (((sq >> (L - 1)) & 1u) ? poly : 0u)) & ((1u << L) - 1u);
    uint32_t r = 1u;
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) r = crc_mulmod(r, sq, poly, L);
        sq = crc_mulmod(sq, sq, poly, L);
    }
    return r;
}
// term i of `parts` of a message of n bytes: byte k is src(k), a table entry is entry(index).  0 for a run that is empty.
template <class Src, class Entry>
__host__ __device__ __forceinline__ uint32_t crc_chunk_term(uint32_t poly, int L, uint32_t n, uint32_t parts, uint32_t i, Src src, Entry entry) {
    const uint32_t per = (n + parts - 1u) / parts;
    const uint32_t begin = i * per;                          // i < parts and per <= n: no overflow for n below 2^31
    if (per == 0u || begin >= n) return 0u;
    const uint32_t end = begin + per < n ? begin + per : n;
    uint32_t reg = 0u;
    for (uint32_t k = begin; k < end; ++k) reg = crc_byte(reg, entry(crc_index(reg, src(k), L)), L);
    return end == n ? reg : crc_mulmod(reg, crc_xpow_bytes(poly, L, n - end), poly, L);
}

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t gold_spread4(uint32_t nib) {         // bit y -> byte y
    return (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
}
// byte i of a block (8 bits, the first one on top) in either layout; `wide`: the block starts on a word boundary
__device__ __forceinline__ uint32_t crc_load_byte(const uint8_t* blk, bool packed, bool wide, int i) {
    if (packed) return blk[i];
    if (wide) {
        const uint2 w = reinterpret_cast<const uint2*>(blk)[i];
        return ((((w.x & 0x01010101u) * 0x08040201u) >> 20) & 0xf0u) | ((((w.y & 0x01010101u) * 0x08040201u) >> 24) & 0x0fu);
    }
    uint32_t v = 0u;
#pragma unroll
    for (int x = 0; x < 8; ++x) v |= (uint32_t(blk[8 * i + x]) & 1u) << (7 - x);
    return v;
}
__device__ __forceinline__ void crc_store_byte(uint8_t* blk, bool packed, bool wide, int i, uint32_t v) {
    if (packed) {
        blk[i] = uint8_t(v);
    } else if (wide) {
        reinterpret_cast<uint2*>(blk)[i] = make_uint2(gold_spread4(__brev(v >> 4) >> 28), gold_spread4(__brev(v & 0xfu) >> 28));
    } else {
#pragma unroll
        for (int x = 0; x < 8; ++x) blk[8 * i + x] = uint8_t((v >> (7 - x)) & 1u);
    }
}
#endif

}  // namespace ofdm
