// tbcc.hip -- LTE tail-biting convolutional code (TS 36.212 5.1.3.1: constraint length 7, rate 1/3, generators 133 / 171 / 165)
// on the frame-batched path: encoder in front of ofdm_tx_modulate_frames, wrap-around Viterbi decoder behind the per-frame LLRs.
// Around it the sub-block interleaver and circular-buffer rate matching of 5.1.4.2: an encoder of its own, a de-matching kernel
// and the decoder's RM instantiation, which de-matches in its tile load.  The definition the kernels implement is the contract
// in include/ofdm_mi355x.h; the reference has no channel code, so there is nothing in it to cite.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <type_traits>
#include "codec_device.hpp"
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

constexpr unsigned TBCC_G0 = 0133, TBCC_G1 = 0171, TBCC_G2 = 0165;   // bit 6 = current input, bit 6-i = delay i

// ------------------------------------------------------------------------------------------ encoder
// dj[k] of the block at blk: the parity of generator j over the 7-bit window that ends at k
__device__ __forceinline__ unsigned tbcc_stream_bit(const uint8_t* blk, int info_packed, int K, int k, int j) {
    unsigned reg = 0u;                                   // bit 6-i = c[(k - i) mod K]
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        int idx = k - i;
        if (idx < 0) idx += K;
        reg |= info_bit(blk, info_packed, idx) << (6 - i);
    }
    const unsigned g = j == 0 ? TBCC_G0 : j == 1 ? TBCC_G1 : TBCC_G2;
    return unsigned(__popc(reg & g)) & 1u;
}

// coded bit q of a segment (0 past the last block: filler)
__device__ __forceinline__ unsigned tbcc_coded_bit(const uint8_t* seg_info, int info_packed, int K, int64_t coded_per_seg, int64_t q) {
    if (q >= coded_per_seg) return 0u;
    const int b = int(q / (3 * K));
    const int r = int(q - int64_t(b) * 3 * K);
    const int k = r / 3, j = r - 3 * k;
    return tbcc_stream_bit(seg_info + int64_t(b) * (info_packed ? K >> 3 : K), info_packed, K, k, j);
}

// One thread per 4 output bytes of a segment (4 coded bits one per byte, or 32 packed MSB-first), stored as one word where the
// address allows it; the filler behind the last block is written as zeros by the same threads.
__global__ void __launch_bounds__(256) tbcc_encode_kernel(TbccEncArgs a) {
    const int64_t words_per_seg = (a.seg_bytes + 3) >> 2;
    const int64_t total = a.n_seg * words_per_seg;
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int64_t seg = g / words_per_seg, w = g - seg * words_per_seg;
    const int info_packed = a.info_mode == 1, coded_packed = a.coded_mode == 1;
    const uint8_t* seg_info = a.info + seg * int64_t(a.blocks_per_seg) * (info_packed ? a.K >> 3 : a.K);
    const int64_t coded_per_seg = int64_t(a.blocks_per_seg) * 3 * a.K;
    const int64_t byte0 = w << 2;
    const int nbytes = int(std::min<int64_t>(4, a.seg_bytes - byte0));
    uint32_t word = 0u;
    for (int y = 0; y < nbytes; ++y) {
        unsigned v;
        if (coded_packed) {
            v = 0u;
            for (int x = 0; x < 8; ++x) v |= tbcc_coded_bit(seg_info, info_packed, a.K, coded_per_seg, ((byte0 + y) << 3) + x) << (7 - x);
        } else {
            v = tbcc_coded_bit(seg_info, info_packed, a.K, coded_per_seg, byte0 + y);
        }
        word |= v << (8 * y);
    }
    uint8_t* dst = a.coded + seg * a.seg_bytes + byte0;
    if (nbytes == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(dst) = word;
    } else {
        for (int y = 0; y < nbytes; ++y) dst[y] = uint8_t(word >> (8 * y));
    }
}

// ------------------------------------------------------------------------------------------ rate matching
// The sub-block interleaver in closed form (include/ofdm_mi355x.h): P[c] is the 5-bit reversal of c ^ 16, so neither P nor its
// inverse is a table, and the NULLs in front of a column are a popcount of the 32-bit mask of the columns that start with one.
__device__ __forceinline__ int tbcc_rm_perm(int c) { return int(__brev(unsigned(c) ^ 16u) >> 27); }        // P[c]
__device__ __forceinline__ int tbcc_rm_perm_inv(int x) { return int(__brev(unsigned(x)) >> 27) ^ 16; }     // P^-1[x]
// rank of d0[i] among the 3K coded bits of the circular buffer; dj[i] sits j*K behind it
__device__ __forceinline__ int tbcc_rm_rank0(const TbccRmGeom& g, int i) {
    const int y = g.ND + i, c = tbcc_rm_perm_inv(y & 31);
    return c * g.R + (y >> 5) - __popc(g.nullmask & ((2u << c) - 1u));
}
// coded bits in front of column c of one stream
__device__ __forceinline__ int tbcc_rm_cum(const TbccRmGeom& g, int c) { return c * g.R - __popc(g.nullmask & ((1u << c) - 1u)); }
// rank r inside a stream (0 <= r < K) -> i: the largest column with cum(c) <= r (cum does not decrease: five halvings), then the row
__device__ __forceinline__ int tbcc_rm_index(const TbccRmGeom& g, int r) {
    int c = 0;
#pragma unroll
    for (int bit = 16; bit; bit >>= 1)
        if (tbcc_rm_cum(g, c | bit) <= r) c |= bit;
    const int p = tbcc_rm_perm(c);
    return 32 * (r - tbcc_rm_cum(g, c) + (p < g.ND ? 1 : 0)) + p - g.ND;
}

// The plain encoder's shape: one thread per 4 output bytes, a whole-word store where the address allows it, the filler written by
// the same threads.  A thread divides once for its first bit and steps (block, bit of the block, rank) from there; every
// output bit is a gather from the information bits: rank -> (j, i) -> the window parity, no d streams in between.
__global__ void __launch_bounds__(256) tbcc_encode_rm_kernel(TbccEncRmArgs a) {
    const int64_t words_per_seg = (a.seg_bytes + 3) >> 2;
    const int64_t total = a.n_seg * words_per_seg;
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int64_t seg = g / words_per_seg, w = g - seg * words_per_seg;
    const int info_packed = a.info_mode == 1, coded_packed = a.coded_mode == 1;
    const int K = a.K, E = a.g.E, blk_bytes = info_packed ? K >> 3 : K;
    const uint8_t* seg_info = a.info + seg * int64_t(a.blocks_per_seg) * blk_bytes;
    const int64_t coded_per_seg = int64_t(a.blocks_per_seg) * E;
    const int64_t byte0 = w << 2;
    const int nbytes = int(std::min<int64_t>(4, a.seg_bytes - byte0));
    const int nbits = coded_packed ? nbytes << 3 : nbytes;
    const int64_t q0 = coded_packed ? byte0 << 3 : byte0;
    int64_t b = q0 / E;
    int k = int(q0 - b * E);
    int rank = k % (3 * K);
    uint32_t word = 0u;
    for (int x = 0; x < nbits; ++x) {
        if (q0 + x < coded_per_seg) {
            const int j = rank >= 2 * K ? 2 : rank >= K ? 1 : 0;
            const unsigned v = tbcc_stream_bit(seg_info + b * blk_bytes, info_packed, K, tbcc_rm_index(a.g, rank - j * K), j);
            word |= v << (coded_packed ? (x & ~7) + 7 - (x & 7) : 8 * x);
        }
        if (++rank == 3 * K) rank = 0;
        if (++k == E) {
            k = 0;
            rank = 0;
            ++b;
        }
    }
    uint8_t* dst = a.coded + seg * a.seg_bytes + byte0;
    if (nbytes == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(dst) = word;
    } else {
        for (int y = 0; y < nbytes; ++y) dst[y] = uint8_t(word >> (8 * y));
    }
}

// De-matching of one coded bit: l = the block's E LLRs, q = the bit's rank, n3 = 3K.  The copies are added in increasing index,
// one float32 addition each; a punctured bit is +0.  No product: nothing here for the compiler to contract.
__device__ __forceinline__ float tbcc_rm_combine(const float* l, int E, int n3, int q) {
    float L = 0.f;
    if (q < E) {
        L = finite_or_zero(l[q]);
        for (int idx = q + n3; idx < E; idx += n3) L = L + finite_or_zero(l[idx]);
    }
    return L;
}

// Stand-alone de-matching: one thread per output LLR (segment, block, 3i + j), the grid is exactly the work.  The stores are
// coalesced; the <= 16 reads per thread are scattered over the block's own E floats.
__global__ void __launch_bounds__(256) tbcc_dematch_kernel(TbccDematchArgs a) {
    const int n3 = 3 * a.K;
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= a.n_blocks * n3) return;
    const int64_t blk = g / n3;
    const int x = int(g - blk * n3);
    const int64_t seg = blk / a.blocks_per_seg;
    const int b = int(blk - seg * a.blocks_per_seg);
    const int i = x / 3, j = x - 3 * i;
    const float* l = a.llr + seg * a.seg_stride + int64_t(b) * a.g.E;
    a.out[seg * a.out_stride + int64_t(b) * n3 + x] = tbcc_rm_combine(l, a.g.E, n3, tbcc_rm_rank0(a.g, i) + j * a.K);
}

// ------------------------------------------------------------------------------------------ decoder
// One wave per code block, lane = trellis state s'.  The path metric lives in one VGPR; the metrics of the two predecessors
// p0 = (s' << 1) & 63 and p0 | 1 come over ds_bpermute with lane-constant addresses.  The LLRs of 64 consecutive steps are loaded
// once per tile, one step per lane (coalesced), and a step's three values are read back with v_readlane (wave-uniform, SGPR
// operands of the branch metric).  Survivors: every lane shifts ITS decision bit of 32 consecutive steps into one register and
// the wave stores 256 B per 32 steps -- sm[t >> 5][s'] bit (t & 31) = decision[t][s'] -- so no ballot has to travel from the
// scalar to the vector side.  The traceback is scalar: per 32 steps every lane re-reads its word, the walk picks the word of
// the current state with v_readlane and runs on the SALU.
//
// Arithmetic (the contract fixes fp32 and the order): sigma_j is +-1, so sigma_j * l_j is exact and
// fma(sigma_1, l_1, sigma_0 * l_0) rounds once, exactly like (sigma_0 l_0 + sigma_1 l_1); the same holds for the third term.
// The fma calls below are therefore the written order, and there is no other product in the metric path to contract.
// RM = false is the plain decoder.  RM = true de-matches in the tile load: the lane that owns step t takes its three LLRs
// straight from the block's E rate-matched floats (tbcc_rm_combine, and a sum that is not finite counts as 0 like any other
// input), so a rate-matched block is decoded in one launch with no 3K-float intermediate.  Everything behind the tile load is
// shared.
template <bool RM>
__global__ void __launch_bounds__(64) tbcc_viterbi_kernel(std::conditional_t<RM, TbccDecRmArgs, TbccDecArgs> a) {
    extern __shared__ uint32_t sm[];                         // [ceil(T / 32)][64]
    const int lane = int(threadIdx.x);
    const int K = a.K, W = TBCC_W, T = K + 2 * TBCC_W;
    const int64_t blk = int64_t(blockIdx.x);
    const int64_t seg = blk / a.blocks_per_seg;
    const int b = int(blk - seg * a.blocks_per_seg);
    const float* llr;
    if constexpr (RM) {
        llr = a.llr + seg * a.seg_stride + int64_t(b) * a.g.E;
    } else {
        llr = a.llr + seg * a.seg_stride + int64_t(b) * 3 * K;
    }

    const int p0 = (lane << 1) & 63;
    const unsigned tr = (unsigned(lane >> 5) << 6) | unsigned(p0);      // transition p0 -> s' with the input bit on top
    const float sg0 = (__popc(tr & TBCC_G0) & 1) ? -1.f : 1.f;
    const float sg1 = (__popc(tr & TBCC_G1) & 1) ? -1.f : 1.f;
    const float sg2 = (__popc(tr & TBCC_G2) & 1) ? -1.f : 1.f;
    const int addr0 = p0 << 2, addr1 = addr0 + 4;

    float pm = 0.f;
    for (int base = 0; base < T; base += 64) {
        float l0 = 0.f, l1 = 0.f, l2 = 0.f;
        if (base + lane < T) {
            const int i = (base + lane + 4 * K - W) % K;     // (t - W) mod K; 4K >= W for every K >= 24
            if constexpr (RM) {
                const int q = tbcc_rm_rank0(a.g, i);
                l0 = finite_or_zero(tbcc_rm_combine(llr, a.g.E, 3 * K, q));
                l1 = finite_or_zero(tbcc_rm_combine(llr, a.g.E, 3 * K, q + K));
                l2 = finite_or_zero(tbcc_rm_combine(llr, a.g.E, 3 * K, q + 2 * K));
            } else {
                l0 = finite_or_zero(llr[3 * i]);
                l1 = finite_or_zero(llr[3 * i + 1]);
                l2 = finite_or_zero(llr[3 * i + 2]);
            }
        }
        for (int h = 0; h < 2; ++h) {
            const int n = std::min(32, T - base - 32 * h);   // a multiple of 8: K % 8 == 0
            if (n <= 0) break;
            uint32_t dec = 0u;
            for (int u = 0; u < n; u += 8) {
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const int src = 32 * h + u + v;
                    const float bm = __builtin_fmaf(sg2, readlane(l2, src),
                                                    __builtin_fmaf(sg1, readlane(l1, src), sg0 * readlane(l0, src)));
                    const float c0 = bperm(addr0, pm) + bm;
                    const float c1 = bperm(addr1, pm) - bm;
                    const bool d = c1 > c0;
                    pm = d ? c1 : c0;
                    dec |= (d ? 1u : 0u) << (u + v);
                }
            }
            sm[(((base >> 5) + h) << 6) + lane] = dec;
        }
    }

    // end state: largest metric, lowest index on a tie
    float best = pm;
    int best_s = lane;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int os = __shfl_xor(best_s, off, 64);
        if (ov > best || (ov == best && os < best_s)) {
            best = ov;
            best_s = os;
        }
    }
    __syncthreads();

    // traceback: bit[t] = s_{t+1} >> 5, s_t = ((s_{t+1} << 1) & 63) | decision[t][s_{t+1}]
    int s = __builtin_amdgcn_readfirstlane(best_s);
    int s_end = 0, s_begin = 0;                              // s_{W+K}, s_W
    for (int g = (T - 1) >> 5; g >= 0; --g) {
        const int mine = int(sm[(g << 6) + lane]);
        uint32_t acc = 0u;                                   // bit (t & 31) = bit[t]
        for (int t = std::min(T - 1, 32 * g + 31); t >= 32 * g; --t) {
            if (t + 1 == W + K) s_end = s;
            acc |= uint32_t(s >> 5) << (t & 31);
            const unsigned word = unsigned(__builtin_amdgcn_readlane(mine, s));
            s = ((s << 1) & 63) | int((word >> (t & 31)) & 1u);
            if (t == W) s_begin = s;
        }
        if (lane == 0) sm[g << 6] = acc;                     // every lane holds this group's words in `mine` already
    }
    __syncthreads();

    if (a.bits) {
        if (a.bits_mode == 1) {                              // packed MSB-first, K / 8 bytes per block
            uint8_t* out = a.bits + blk * (K >> 3);
            for (int j = lane; j < (K >> 3); j += 64) {
                const int t = W + 8 * j;                     // W % 32 == 0: the byte's 8 steps sit in one word
                const uint32_t byte = (sm[(t >> 5) << 6] >> (t & 31)) & 0xffu;
                out[j] = uint8_t(__brev(byte) >> 24);
            }
        } else {
            uint8_t* out = a.bits + blk * K;
            const bool aligned = (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
            for (int i = 4 * lane; i < K; i += 256) {        // K % 4 == 0
                const int t = W + i;
                const uint32_t nib = (sm[(t >> 5) << 6] >> (t & 31)) & 0xfu;
                const uint32_t word = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
                if (aligned) {
                    *reinterpret_cast<uint32_t*>(out + i) = word;
                } else {
                    for (int y = 0; y < 4; ++y) out[i + y] = uint8_t(word >> (8 * y));
                }
            }
        }
    }
    if (lane == 0) {
        if (a.metric) a.metric[blk] = best;
        if (a.tb_ok) a.tb_ok[blk] = s_begin == s_end ? 1 : 0;
    }
}

}  // namespace

size_t tbcc_lds_bytes(int K) { return size_t((K + 2 * TBCC_W + 31) / 32) * 64 * sizeof(uint32_t); }

hipError_t launch_tbcc_encode(const TbccEncArgs& a, hipStream_t s) {
    const int64_t total = a.n_seg * ((a.seg_bytes + 3) >> 2);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(tbcc_encode_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tbcc_decode(const TbccDecArgs& a, hipStream_t s) {
    if (a.n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(tbcc_viterbi_kernel<false>, dim3(unsigned(a.n_blocks)), dim3(64), tbcc_lds_bytes(a.K), s, a);
    return hipGetLastError();
}

TbccRmGeom tbcc_rm_geom(int K, int E) {
    TbccRmGeom g{};
    g.E = E;
    g.R = (K + 31) / 32;
    g.ND = 32 * g.R - K;
    for (unsigned c = 0; c < 32; ++c) {
        unsigned x = c ^ 16u, p = 0u;                        // P[c]: the 5-bit reversal of c ^ 16
        for (int bit = 0; bit < 5; ++bit) p |= ((x >> bit) & 1u) << (4 - bit);
        if (int(p) < g.ND) g.nullmask |= 1u << c;
    }
    return g;
}

hipError_t launch_tbcc_encode_rm(const TbccEncRmArgs& a, hipStream_t s) {
    const int64_t total = a.n_seg * ((a.seg_bytes + 3) >> 2);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(tbcc_encode_rm_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tbcc_dematch(const TbccDematchArgs& a, hipStream_t s) {
    const int64_t total = a.n_blocks * 3 * a.K;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(tbcc_dematch_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tbcc_decode_rm(const TbccDecRmArgs& a, hipStream_t s) {
    if (a.n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(tbcc_viterbi_kernel<true>, dim3(unsigned(a.n_blocks)), dim3(64), tbcc_lds_bytes(a.K), s, a);
    return hipGetLastError();
}

hipError_t tbcc_decode_prepare() { return load_kernels(tbcc_viterbi_kernel<false>, tbcc_viterbi_kernel<true>); }

}  // namespace ofdm
