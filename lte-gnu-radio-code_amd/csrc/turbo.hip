// turbo.hip -- LTE turbo code (TS 36.212 5.1.3.2: two 8-state constituent encoders 1 + D^2 + D^3 / 1 + D + D^3 around a QPP
// interleaver, rate 1/3, trellis termination) on the frame-batched path: encoder in front of ofdm_tx_modulate_frames, iterative
// max-log-MAP decoder behind the per-frame LLRs.  The definition the kernels implement is the contract in
// include/ofdm_mi355x.h; the reference has no channel code, so there is nothing in it to cite.
//
// Arithmetic: the contract fixes every float32 operation and its order, and -inf is a value of the forward recursion.  HIP
// device code is compiled with -ffp-contract=fast by default, which would fuse a product into the add behind it (one rounding
// instead of two); the pragma below turns that off for this whole translation unit, and the build has no fast-math flag (no
// finite-math assumption).  The only fused operations left are the explicit fmaf calls, each of whose products is +-1 times a
// value -- exact -- so that the fma rounds once, exactly like the product followed by the add.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ofdm_launch.hpp"
#include "turbo_device.hpp"

#pragma clang fp contract(off)

#include "turbo_siso.hpp"

namespace ofdm {

namespace {

// ------------------------------------------------------------------------------------------ encoder
// One wave per PAIR of consecutive blocks of a segment, 32 lanes per block: 2 (3K + 12) coded bits are a whole number of bytes,
// so that a wave's packed output starts and ends on a byte of its own although a single block (3K + 12 = 4 mod 8) does not.
//   A  every lane runs both constituent encoders over its chunk of ceil(K / 32) steps from state 0 (the zero-state response);
//   -  the recursion is linear over GF(2), so the state behind a chunk is free^len(entry) ^ response: a walk over the 32 lanes
//      gives every lane its two entry states and the wave the two final states, hence the 12 tail bits;
//   B  every lane runs its chunk again from its entry states and leaves z[k] | z'[k] << 1 in LDS, one byte per step;
//   C  the TBCC encoder's store shape: one lane per 4 output bytes of the pair's part of the segment, a whole-word store where
//      the address allows it; the filler behind a segment's last block is written by its last wave (a segment without blocks
//      has one wave that writes nothing else).
__global__ void __launch_bounds__(64) turbo_encode_kernel(TurboEncArgs a) {
    extern __shared__ uint8_t sm_enc[];                      // [8] two tail words, then [2][K] parity bytes
    uint32_t* sm_tail = reinterpret_cast<uint32_t*>(sm_enc);
    uint8_t* sm_z = sm_enc + 8;
    const int lane = int(threadIdx.x), half = lane >> 5, hl = lane & 31;
    const int K = a.q.K, bps = a.blocks_per_seg;
    const int info_packed = a.info_mode == 1, coded_packed = a.coded_mode == 1;
    const int64_t units_per_seg = std::max<int64_t>(1, (int64_t(bps) + 1) >> 1);
    const int64_t seg = int64_t(blockIdx.x) / units_per_seg;
    const int64_t u = int64_t(blockIdx.x) - seg * units_per_seg;
    const int64_t b = 2 * u + half;
    const bool has = b < bps;
    const int blk_bytes = info_packed ? K >> 3 : K;
    const uint8_t* pair_info = a.info + (seg * bps + 2 * u) * blk_bytes;
    const uint8_t* info = pair_info + int64_t(half) * blk_bytes;

    const int chunk = (K + 31) >> 5;
    const int k_begin = std::min(K, hl * chunk), k_end = std::min(K, k_begin + chunk);
    const unsigned uK = unsigned(K);
    const unsigned p_begin = turbo_qpp_at(a.q, unsigned(k_begin));
    // pi(i + 1) - pi(i) = f1 + f2 (2 i + 1)
    const unsigned g_begin = (unsigned(a.q.f1) + unsigned(a.q.f2) + (unsigned(a.q.g2) * unsigned(k_begin)) % uK) % uK;

    unsigned s1 = 0u, s2 = 0u, z;
    if (has) {
        unsigned p = p_begin, g = g_begin;
        for (int k = k_begin; k < k_end; ++k) {
            s1 = turbo_rsc_step(s1, info_bit(info, info_packed, unsigned(k)), z);
            s2 = turbo_rsc_step(s2, info_bit(info, info_packed, p), z);
            p = turbo_mod_add(p, g, uK);
            g = turbo_mod_add(g, unsigned(a.q.g2), uK);
        }
    }
    const int len7 = (k_end - k_begin) % 7;
    unsigned e1 = 0u, e2 = 0u, in1 = 0u, in2 = 0u;
    for (int l = 0; l < 32; ++l) {
        if (hl == l) {
            in1 = e1;
            in2 = e2;
        }
        const int src = (half << 5) + l;
        const int n = __shfl(len7, src, 64);
        e1 = turbo_rsc_free(e1, n) ^ unsigned(__shfl(int(s1), src, 64));
        e2 = turbo_rsc_free(e2, n) ^ unsigned(__shfl(int(s2), src, 64));
    }
    if (hl == 0) sm_tail[half] = (turbo_rsc_tail(e1) << 6) | turbo_rsc_tail(e2);      // bit 11 - t = coded bit 3K + t
    if (has) {
        unsigned p = p_begin, g = g_begin, z1, z2;
        s1 = in1;
        s2 = in2;
        for (int k = k_begin; k < k_end; ++k) {
            s1 = turbo_rsc_step(s1, info_bit(info, info_packed, unsigned(k)), z1);
            s2 = turbo_rsc_step(s2, info_bit(info, info_packed, p), z2);
            sm_z[half * K + k] = uint8_t(z1 | (z2 << 1));
            p = turbo_mod_add(p, g, uK);
            g = turbo_mod_add(g, unsigned(a.q.g2), uK);
        }
    }
    __syncthreads();

    const int64_t blk_bits = 3 * int64_t(K) + 12;
    const int64_t q_begin = 2 * u * blk_bits;
    const int64_t q_coded = q_begin + std::min<int64_t>(2, std::max<int64_t>(0, bps - 2 * u)) * blk_bits;
    const int shift = coded_packed ? 3 : 0;                  // bits per byte of the coded buffer: 8 or 1
    const int64_t byte_begin = q_begin >> shift;
    const int64_t byte_end = u == units_per_seg - 1 ? a.seg_bytes : q_coded >> shift;
    auto coded_bit = [&](int64_t q) -> unsigned {
        if (q >= q_coded) return 0u;
        int64_t r = q - q_begin;
        const int lb = r >= blk_bits ? 1 : 0;
        r -= lb * blk_bits;
        if (r >= 3 * K) return (sm_tail[lb] >> (11 - int(r - 3 * K))) & 1u;
        const int k = int(r) / 3, j = int(r) - 3 * k;
        if (j == 0) return info_bit(pair_info + int64_t(lb) * blk_bytes, info_packed, unsigned(k));
        return (unsigned(sm_z[lb * K + k]) >> (j - 1)) & 1u;
    };
    uint8_t* seg_out = a.coded + seg * a.seg_bytes;
    for (int64_t byte0 = byte_begin + 4 * int64_t(lane); byte0 < byte_end; byte0 += 256) {
        const int nbytes = int(std::min<int64_t>(4, byte_end - byte0));
        uint32_t word = 0u;
        for (int y = 0; y < nbytes; ++y) {
            unsigned v;
            if (coded_packed) {
                v = 0u;
                for (int x = 0; x < 8; ++x) v |= coded_bit(((byte0 + y) << 3) + x) << (7 - x);
            } else {
                v = coded_bit(byte0 + y);
            }
            word |= v << (8 * y);
        }
        uint8_t* dst = seg_out + byte0;
        if (nbytes == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(dst) = word;
        } else {
            for (int y = 0; y < nbytes; ++y) dst[y] = uint8_t(word >> (8 * y));
        }
    }
}

// ------------------------------------------------------------------------------------------ decoder
// One wave per 8 code blocks, lane = (block, state): group = lane >> 3 is the block, lane & 7 the trellis state, one state metric
// per VGPR.  A step's exchange of metrics stays inside the 8-lane group: ds_bpermute with lane-constant addresses for the two
// predecessors (forward) or successors (backward), xor-shuffles for the two maxima over the states.  A wave is full whatever K
// is, and a batch needs only 8 blocks per wave.
//
// Steps run in tiles of TURBO_CKPT.  The lanes of a group load a tile's inputs -- x = ls + la and lp, through pi for the second
// decoder -- one step per lane and 8 steps apart, and leave them in LDS with the index the step's output goes to; every step then
// reads its pair back with one ds_read_b64 (8 addresses per wave, the rows padded by one entry so that they fall on different
// banks).  The forward metrics are not kept for all k (32 B per step and block): a first forward pass stores A at every tile
// start in the workspace (a checkpoint: 64 floats per wave and tile, written and read back by the same lane), and the backward
// pass runs each tile forward again from its checkpoint into LDS (sm_a, one column per lane) before it walks the tile backwards.
// The second run does the same operations on the same values, so it is exact.  The grid of the normalisation (every 8 steps)
// divides the tile length, so a checkpoint is a normalised A.
//
// The extrinsic values live in the workspace, K floats per block, in the first decoder's order: decoder 1 reads la1[k] and
// writes e1[k] over it, decoder 2 reads e1[pi(i)] and writes e2[i] over it as la1[pi(i)].  A tile's values are read (by the tile
// load) before the tile's steps overwrite them and pi is a permutation, so one array serves both.  The last half-iteration writes
// post in place of the extrinsic value, which leaves llr[k] in natural order for the output pass.
//
// The half-iteration itself -- lane constants, tile load, forward tile, tail, backward tile -- is turbo_half_iteration of
// turbo_siso.hpp, which turbo_decode_es_kernel (turbo_es.hip) instantiates too.
__global__ void __launch_bounds__(64) turbo_decode_kernel(TurboDecArgs a) {
    __shared__ float sm_a[TURBO_CKPT * 64];                  // [step of the tile][lane] forward metrics
    __shared__ float2 sm_x[8 * TURBO_ROW];                   // [group][step] {x, lp}
    __shared__ int sm_i[8 * TURBO_ROW];                      // [group][step] index of the step's output in the block's K floats
    const int lane = int(threadIdx.x), grp = lane >> 3, st = lane & 7;
    const int K = a.q.K;
    const int64_t blk = int64_t(blockIdx.x) * TURBO_GROUP + grp;
    const bool active = blk < a.n_blocks;
    const int64_t seg = active ? blk / a.blocks_per_seg : 0;
    const int64_t b = active ? blk - seg * a.blocks_per_seg : 0;
    const float* llr = a.llr + seg * a.seg_stride + b * (3 * int64_t(K) + 12);
    float* ext = a.ext + blk * K;                            // touched by active groups only
    const int n_tiles = (K + TURBO_CKPT - 1) / TURBO_CKPT;
    float* ckpt = a.ckpt + int64_t(blockIdx.x) * n_tiles * 64 + lane;
    float2* my_x = sm_x + grp * TURBO_ROW;
    int* my_i = sm_i + grp * TURBO_ROW;

    const TurboLane c = turbo_lane(grp, st);

    for (int it = 0; it < a.n_iter; ++it) {
        for (int half = 0; half < 2; ++half) {
            const bool first = it == 0 && half == 0;         // la1 = 0
            const bool last = it == a.n_iter - 1 && half == 1;
            turbo_half_iteration<false>(a.q, llr, ext, nullptr, ckpt, active, active, half, first, last, c, sm_a, my_x, my_i, lane, st);
        }
    }

    if (!active) return;
    if (a.llr_out) {
        float* out = a.llr_out + blk * K;
        for (int k = st; k < K; k += 8) out[k] = ext[k];
    }
    if (a.bits) {
        if (a.bits_mode == 1) {                              // packed MSB-first, K / 8 bytes per block
            uint8_t* out = a.bits + blk * (K >> 3);
            for (int j = st; j < (K >> 3); j += 8) {
                unsigned byte = 0u;
#pragma unroll
                for (int x = 0; x < 8; ++x) byte |= (ext[8 * j + x] < 0.f ? 1u : 0u) << (7 - x);
                out[j] = uint8_t(byte);
            }
        } else {
            uint8_t* out = a.bits + blk * K;
            for (int k = st; k < K; k += 8) out[k] = ext[k] < 0.f ? 1 : 0;
        }
    }
}

}  // namespace

bool turbo_qpp_valid(int64_t K, int64_t f1, int64_t f2) {
    if (!turbo_valid_k(K) || f1 < 0 || f1 >= K || f2 < 0 || f2 >= K) return false;
    uint64_t seen[(TURBO_K_MAX + 63) / 64] = {};
    int64_t p = 0, g = (f1 + f2) % K;                        // pi(0), pi(1) - pi(0)
    for (int64_t i = 0; i < K; ++i) {
        if (seen[p >> 6] >> (p & 63) & 1u) return false;
        seen[p >> 6] |= uint64_t(1) << (p & 63);
        p = (p + g) % K;
        g = (g + 2 * f2) % K;
    }
    return true;
}

TurboQpp turbo_qpp(int K, int f1, int f2) {
    TurboQpp q{};
    q.K = K;
    q.f1 = f1;
    q.f2 = f2;
    q.g2 = int((2 * int64_t(f2)) % K);
    q.c8 = int((8 * int64_t(f1) + 64 * int64_t(f2)) % K);
    q.c16 = int((16 * int64_t(f2)) % K);
    q.c128 = int((128 * int64_t(f2)) % K);
    return q;
}

int64_t turbo_ws_floats(int64_t n_blocks, int K) {
    const int64_t waves = (n_blocks + TURBO_GROUP - 1) / TURBO_GROUP;
    return n_blocks * K + waves * ((K + TURBO_CKPT - 1) / TURBO_CKPT) * 64;
}

hipError_t launch_turbo_encode(const TurboEncArgs& a, hipStream_t s) {
    const int64_t units = a.n_seg * std::max<int64_t>(1, (int64_t(a.blocks_per_seg) + 1) >> 1);
    if (units <= 0 || a.seg_bytes <= 0) return hipSuccess;
    hipLaunchKernelGGL(turbo_encode_kernel, dim3(unsigned(units)), dim3(64), size_t(8 + 2 * a.q.K), s, a);
    return hipGetLastError();
}

hipError_t launch_turbo_decode(const TurboDecArgs& a, hipStream_t s) {
    if (a.n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(turbo_decode_kernel, dim3(unsigned((a.n_blocks + TURBO_GROUP - 1) / TURBO_GROUP)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t turbo_decode_prepare() { return load_kernels(turbo_decode_kernel); }

}  // namespace ofdm
