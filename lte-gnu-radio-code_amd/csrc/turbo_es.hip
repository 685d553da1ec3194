// turbo_es.hip -- the turbo decoder of turbo.hip with early termination by CRC: after every full iteration from min_iter on, the
// CRC of each block's hard decisions is checked, a block whose remainder is zero is frozen, and a wave ends as soon as all of
// its blocks are.  The definition is the contract in include/ofdm_mi355x.h: a block that stops after n
// iterations has exactly the outputs of turbo_decode_kernel at n_iter = n.  The half-iteration is the one of turbo_siso.hpp,
// shared with turbo.hip, so the float32 operations and their order are the same by construction.
//
// Arithmetic: as in turbo.hip, no contraction anywhere in this translation unit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "crc_device.hpp"
#include "ofdm_launch.hpp"
#include "turbo_device.hpp"

#pragma clang fp contract(off)

#include "turbo_siso.hpp"

namespace ofdm {

namespace {

// The mapping of turbo_decode_kernel: one wave per 8 code blocks, lane = (block, state), tiles of TURBO_CKPT, checkpointed
// forward pass, one ext array for both decoders.  What differs:
//   post   In the second half of every iteration with it + 1 >= min_iter a live group stores e to ext as always and post, at
//          the same natural-order index, to a second K-float array of its block.  The CRC pass and the output pass read it.
//   CRC    Behind the barrier that ends that half-iteration the group's 8 lanes each take a contiguous run of the block's K / 8
//          bytes (a byte = the signs of eight post values, the first on top) through the byte table of the kind in use (LDS),
//          weight the remainder by x^(8 bytes behind the run) mod g and XOR the 8 terms with shuffles: the chunk-and-combine
//          construction of crc_device.hpp, no atomics, the same value for every chunking.
//   freeze `done` is uniform over a group.  A group that is done (or has no block) stores nothing more -- not ext, not post,
//          not a checkpoint -- so its post array holds the post of its stopping iteration.  Its lanes keep executing, because
//          ds_bpermute, the shuffles and the barriers need the whole wave; what they compute from then on is discarded.
//   exit   The iteration loop leaves when every group is done or empty, or at max_iter.
__global__ void __launch_bounds__(64) turbo_decode_es_kernel(TurboDecEsArgs a) {
    __shared__ float sm_a[TURBO_CKPT * 64];                  // [step of the tile][lane] forward metrics
    __shared__ float2 sm_x[8 * TURBO_ROW];                   // [group][step] {x, lp}
    __shared__ int sm_i[8 * TURBO_ROW];                      // [group][step] index of the step's output in the block's K floats
    __shared__ uint32_t sm_tab[256];                         // byte table of the CRC kind in use
    const int lane = int(threadIdx.x), grp = lane >> 3, st = lane & 7;
    const int K = a.q.K;
    const int64_t blk = int64_t(blockIdx.x) * TURBO_GROUP + grp;
    const bool active = blk < a.n_blocks;
    const int64_t seg = active ? blk / a.blocks_per_seg : 0;
    const int64_t b = active ? blk - seg * a.blocks_per_seg : 0;
    const float* llr = a.llr + seg * a.seg_stride + b * (3 * int64_t(K) + 12);
    float* ext = a.ext + blk * K;                            // touched by active groups only
    float* post = a.post + blk * K;                          // likewise
    const int n_tiles = (K + TURBO_CKPT - 1) / TURBO_CKPT;
    float* ckpt = a.ckpt + int64_t(blockIdx.x) * n_tiles * 64 + lane;
    float2* my_x = sm_x + grp * TURBO_ROW;
    int* my_i = sm_i + grp * TURBO_ROW;
    const TurboLane c = turbo_lane(grp, st);

    const uint32_t poly = crc_poly(a.crc_kind);
    const int L = crc_len(a.crc_kind);
#pragma unroll
    for (int j = 0; j < 4; ++j) sm_tab[lane + 64 * j] = crc_table_entry(poly, L, uint32_t(lane + 64 * j));
    // this lane's run of the block's bytes and the weight of its remainder; a run may be empty (K = 40: 5 bytes over 8 lanes)
    const int n_bytes = K >> 3, per = (n_bytes + 7) >> 3;
    const int run_begin = std::min(n_bytes, st * per), run_end = std::min(n_bytes, run_begin + per);
    const uint32_t weight = crc_xpow_bytes(poly, L, uint32_t(n_bytes - run_end));

    bool done = !active;
    int iters = a.max_iter;
    uint32_t ok = 0u;
    for (int it = 0; it < a.max_iter; ++it) {
        const bool eligible = it + 1 >= a.min_iter;
        const bool store = !done;
        turbo_half_iteration<true>(a.q, llr, ext, post, ckpt, active, store, 0, it == 0, false, c, sm_a, my_x, my_i, lane, st);
        turbo_half_iteration<true>(a.q, llr, ext, post, ckpt, active, store, 1, false, eligible, c, sm_a, my_x, my_i, lane, st);
        if (eligible) {
            uint32_t reg = 0u;
            if (active) {
                for (int k = run_begin; k < run_end; ++k) {
                    const float4 p0 = *reinterpret_cast<const float4*>(post + 8 * k);
                    const float4 p1 = *reinterpret_cast<const float4*>(post + 8 * k + 4);
                    const uint32_t byte = (p0.x < 0.f ? 0x80u : 0u) | (p0.y < 0.f ? 0x40u : 0u) | (p0.z < 0.f ? 0x20u : 0u) |
                                          (p0.w < 0.f ? 0x10u : 0u) | (p1.x < 0.f ? 0x08u : 0u) | (p1.y < 0.f ? 0x04u : 0u) |
                                          (p1.z < 0.f ? 0x02u : 0u) | (p1.w < 0.f ? 0x01u : 0u);
                    reg = crc_byte(reg, sm_tab[crc_index(reg, byte, L)], L);
                }
                reg = crc_mulmod(reg, weight, poly, L);
            }
            reg ^= uint32_t(__shfl_xor(int(reg), 1, 64));
            reg ^= uint32_t(__shfl_xor(int(reg), 2, 64));
            reg ^= uint32_t(__shfl_xor(int(reg), 4, 64));
            if (!done && reg == 0u) {
                done = true;
                iters = it + 1;
                ok = 1u;
            }
        }
        if (__all(done)) break;
    }

    if (!active) return;
    if (a.llr_out) {
        float* out = a.llr_out + blk * K;
        for (int k = st; k < K; k += 8) out[k] = post[k];
    }
    if (a.bits) {
        if (a.bits_mode == 1) {                              // packed MSB-first, K / 8 bytes per block
            uint8_t* out = a.bits + blk * (K >> 3);
            for (int j = st; j < (K >> 3); j += 8) {
                unsigned byte = 0u;
#pragma unroll
                for (int x = 0; x < 8; ++x) byte |= (post[8 * j + x] < 0.f ? 1u : 0u) << (7 - x);
                out[j] = uint8_t(byte);
            }
        } else {
            uint8_t* out = a.bits + blk * K;
            for (int k = st; k < K; k += 8) out[k] = post[k] < 0.f ? 1 : 0;
        }
    }
    if (st == 0) {
        const int64_t at = seg * a.stat_stride + b;
        if (a.iters) a.iters[at] = uint8_t(iters);
        if (a.crc_ok) a.crc_ok[at] = uint8_t(ok);
    }
}

}  // namespace

int64_t turbo_es_ws_floats(int64_t n_blocks, int K) {
    return n_blocks * K + turbo_ws_floats(n_blocks, K);
}

hipError_t launch_turbo_decode_es(const TurboDecEsArgs& a, hipStream_t s) {
    if (a.n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(turbo_decode_es_kernel, dim3(unsigned((a.n_blocks + TURBO_GROUP - 1) / TURBO_GROUP)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t turbo_decode_es_prepare() { return load_kernels(turbo_decode_es_kernel); }

}  // namespace ofdm
