// turbo_rm.hip -- rate matching of the LTE turbo code (TS 36.212 5.1.4.1: three sub-block interleavers, the third with its own
// permutation, a circular buffer with v1 and v2 interlaced, a buffer limit Ncb and a redundancy-version start k0) around the
// codec of turbo.hip: an encoder of its own in front of ofdm_tx_modulate_frames and a de-matching kernel that can add a
// retransmission into an existing soft buffer (HARQ).  The definition the kernels implement is the contract in
// include/ofdm_mi355x.h; the reference has no channel code, so there is nothing in it to cite.
//
// Closed form.  P[c] is the 5-bit reversal of c and its own inverse, so neither is a table.  With y = ND + i the place of d0[i]
// and d1[i] in its stream is column P[y & 31], row y >> 5; d2[i] sits where pi2 = y, which is the same with y - 1.  The NULLs
// are row 0 of the columns with P[c] < ND (v0, v1) or P[c] < ND - 1 (v2), and v2's very last entry (pi2 = 0); the non-NULL
// entries in front of a place are therefore a popcount of a 32-bit mask (turbo_rm_stream_count, shared with the host), and the
// rank of a coded bit in the circular buffer follows from the interlacing: v0 first, then v1[k] in front of v2[k].  Its first
// transmission is n0 = (rank - rank(k0)) mod Navail, its copies follow every Navail bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ofdm_launch.hpp"
#include "turbo_device.hpp"

namespace ofdm {

namespace {

__device__ __forceinline__ int turbo_rm_rank0(const TurboRmGeom& g, int rv) {
    return rv == 0 ? g.rank0[0] : rv == 1 ? g.rank0[1] : rv == 2 ? g.rank0[2] : g.rank0[3];
}
__device__ __forceinline__ int turbo_rm_rv(int rv, const int32_t* rv_dev, int64_t seg) { return rv_dev ? int(rv_dev[seg]) & 3 : rv; }

// n0 of dj[i]: the index of its first transmission in e for a start of rank rank0, or -1 if its place in w is at or behind Ncb
__device__ __forceinline__ int turbo_rm_first(const TurboRmGeom& g, int rank0, int i, int j) {
    const int y = g.ND + i - (j == 2 ? 1 : 0);               // >= ND - 1 >= 3
    const int c = int(__brev(unsigned(y & 31)) >> 27), r = y >> 5;
    const int kv = c * g.R + r;
    const int pos = j == 0 ? kv : g.Kpi + 2 * kv + (j - 1);
    if (pos >= g.Ncb) return -1;
    int rank = turbo_rm_stream_count(g.mask01, g.R, c, r);
    if (j) rank += g.D + turbo_rm_stream_count(g.mask2, g.R, c, r);
    if (j == 2 && !(r == 0 && ((g.mask01 >> c) & 1u))) ++rank;          // v1[kv] in front of v2[kv], unless it is a NULL
    const int d = rank - rank0;
    return d < 0 ? d + g.navail : d;
}

// ------------------------------------------------------------------------------------------ encoder
// One wave per group of turbo_rm_group() consecutive blocks of a segment -- 8 / gcd(E, 8) with packed output, so that the
// group's bits are a whole number of bytes and no two workgroups share one; 1 with a bit per byte -- taken one block at a time:
//   A  every lane runs both constituent encoders over its chunk of ceil(K / 64) steps from state 0; the walk over the lanes
//      gives each its two entry states and the wave the two final states, hence the 12 tail bits (turbo.hip's scheme, 64 lanes);
//   B  every lane runs its chunk again from its entry states and leaves c[k], z[k], z'[k] in LDS AT THEIR RANK in the circular
//      buffer, one byte each (sm_w[rank] for the Navail entries of w[0 .. Ncb) that are not NULL); lanes 0 .. 11 add the tail;
//   C  output bit n of the block is sm_w[(rank0 + n) mod Navail]: one lane per 4 whole output bytes, a whole-word store where
//      the address allows it.  A block that starts or ends inside a byte (packed, E % 8 != 0) hands the byte's leading bits to
//      the next block of the group through sm_carry (two slots, so that the reader and the writer of one pass do not meet).
// The last group of a segment completes a byte left open with zeros and writes the filler (a segment without blocks has one
// group that writes nothing else).
__global__ void __launch_bounds__(64) turbo_encode_rm_kernel(TurboEncRmArgs a, int group) {
    extern __shared__ uint8_t sm_rm[];                       // [8] the two carry bytes, then [Navail] the buffer
    uint8_t* sm_carry = sm_rm;
    uint8_t* sm_w = sm_rm + 8;
    const int lane = int(threadIdx.x);
    const int K = a.q.K, bps = a.blocks_per_seg, E = a.g.E, navail = a.g.navail;
    const int info_packed = a.info_mode == 1, coded_packed = a.coded_mode == 1;
    const int64_t units_per_seg = std::max<int64_t>(1, (int64_t(bps) + group - 1) / group);
    const int64_t seg = int64_t(blockIdx.x) / units_per_seg;
    const int64_t u = int64_t(blockIdx.x) - seg * units_per_seg;
    const int64_t b_begin = u * group;
    const int n_here = int(std::min<int64_t>(group, std::max<int64_t>(0, bps - b_begin)));
    const int blk_bytes = info_packed ? K >> 3 : K;
    const int rank0 = turbo_rm_rank0(a.g, turbo_rm_rv(a.rv, a.rv_dev, seg));
    const int shift = coded_packed ? 3 : 0;                  // bits per byte of the coded buffer: 8 or 1
    uint8_t* seg_out = a.coded + seg * a.seg_bytes;

    const int chunk = (K + 63) >> 6;
    const int k_begin = std::min(K, lane * chunk), k_end = std::min(K, k_begin + chunk);
    const unsigned uK = unsigned(K);
    const unsigned p_begin = turbo_qpp_at(a.q, unsigned(k_begin));
    // pi(i + 1) - pi(i) = f1 + f2 (2 i + 1)
    const unsigned g_begin = (unsigned(a.q.f1) + unsigned(a.q.f2) + (unsigned(a.q.g2) * unsigned(k_begin)) % uK) % uK;
    const int len7 = (k_end - k_begin) % 7;
    if (lane < 2) sm_carry[lane] = 0;

    for (int t = 0; t < n_here; ++t) {
        const uint8_t* info = a.info + (seg * bps + b_begin + t) * blk_bytes;
        unsigned s1 = 0u, s2 = 0u, z;
        {
            unsigned p = p_begin, g = g_begin;
            for (int k = k_begin; k < k_end; ++k) {
                s1 = turbo_rsc_step(s1, info_bit(info, info_packed, unsigned(k)), z);
                s2 = turbo_rsc_step(s2, info_bit(info, info_packed, p), z);
                p = turbo_mod_add(p, g, uK);
                g = turbo_mod_add(g, unsigned(a.q.g2), uK);
            }
        }
        unsigned e1 = 0u, e2 = 0u, in1 = 0u, in2 = 0u;
        for (int l = 0; l < 64; ++l) {
            if (lane == l) {
                in1 = e1;
                in2 = e2;
            }
            const int n = __shfl(len7, l, 64);
            e1 = turbo_rsc_free(e1, n) ^ unsigned(__shfl(int(s1), l, 64));
            e2 = turbo_rsc_free(e2, n) ^ unsigned(__shfl(int(s2), l, 64));
        }
        {
            unsigned p = p_begin, g = g_begin, z1, z2;
            s1 = in1;
            s2 = in2;
            for (int k = k_begin; k < k_end; ++k) {
                const unsigned c = info_bit(info, info_packed, unsigned(k));
                s1 = turbo_rsc_step(s1, c, z1);
                s2 = turbo_rsc_step(s2, info_bit(info, info_packed, p), z2);
                const int n0 = turbo_rm_first(a.g, 0, k, 0), n1 = turbo_rm_first(a.g, 0, k, 1), n2 = turbo_rm_first(a.g, 0, k, 2);
                if (n0 >= 0) sm_w[n0] = uint8_t(c);
                if (n1 >= 0) sm_w[n1] = uint8_t(z1);
                if (n2 >= 0) sm_w[n2] = uint8_t(z2);
                p = turbo_mod_add(p, g, uK);
                g = turbo_mod_add(g, unsigned(a.q.g2), uK);
            }
        }
        if (lane < 12) {                                     // coded bit 3K + lane = d_{lane % 3}[K + lane / 3] = bit 11 - lane
            const unsigned tail = (turbo_rsc_tail(e1) << 6) | turbo_rsc_tail(e2);
            const int n = turbo_rm_first(a.g, 0, K + lane / 3, lane % 3);
            if (n >= 0) sm_w[n] = uint8_t((tail >> (11 - lane)) & 1u);
        }
        __syncthreads();

        const int64_t q0 = (b_begin + t) * int64_t(E), q1 = q0 + E;      // the block's bits of the segment
        const int64_t full0 = (q0 + (coded_packed ? 7 : 0)) >> shift, full1 = q1 >> shift;       // its whole bytes
        // bits q .. q + n - 1 of the segment (inside the block), the first on top of an n-bit value
        auto bits_at = [&](int64_t q, int n) -> unsigned {
            int idx = (rank0 + int(q - q0)) % navail;
            unsigned v = 0u;
            for (int x = 0; x < n; ++x) {
                v = (v << 1) | sm_w[idx];
                if (++idx == navail) idx = 0;
            }
            return v;
        };
        for (int64_t byte0 = full0 + 4 * int64_t(lane); byte0 < full1; byte0 += 256) {
            const int nbytes = int(std::min<int64_t>(4, full1 - byte0));
            uint32_t word = 0u;
            if (coded_packed) {
                const unsigned v = bits_at(byte0 << 3, 8 * nbytes);      // byte y = bits 8 (nbytes - 1 - y) .. of v
                for (int y = 0; y < nbytes; ++y) word |= ((v >> (8 * (nbytes - 1 - y))) & 0xffu) << (8 * y);
            } else {
                const unsigned v = bits_at(byte0, nbytes);
                for (int y = 0; y < nbytes; ++y) word |= ((v >> (nbytes - 1 - y)) & 1u) << (8 * y);
            }
            uint8_t* dst = seg_out + byte0;
            if (nbytes == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
                *reinterpret_cast<uint32_t*>(dst) = word;
            } else {
                for (int y = 0; y < nbytes; ++y) dst[y] = uint8_t(word >> (8 * y));
            }
        }
        if (coded_packed && lane == 0 && (q0 & 7)) {         // the byte the block starts in: the carry, then the block's bits
            const int n = int(std::min<int64_t>(q1, full0 << 3) - q0);
            const unsigned v = unsigned(sm_carry[t & 1]) | (bits_at(q0, n) << (8 - int(q0 & 7) - n));
            if (q1 >= (full0 << 3)) seg_out[full0 - 1] = uint8_t(v);
            else sm_carry[(t + 1) & 1] = uint8_t(v);         // the block ends inside the same byte
        }
        if (coded_packed && lane == 1 && (q1 & 7) && full1 >= full0) {      // the byte the block ends in: left to the next block
            const int n = int(q1 & 7);
            sm_carry[(t + 1) & 1] = uint8_t(bits_at(full1 << 3, n) << (8 - n));
        }
        __syncthreads();
    }

    if (u != units_per_seg - 1) return;
    __syncthreads();
    const int64_t q_end = int64_t(bps) * E;
    int64_t fill0 = (q_end + (coded_packed ? 7 : 0)) >> shift;
    if (coded_packed && lane == 0 && (q_end & 7)) seg_out[fill0 - 1] = sm_carry[n_here & 1];    // zeros complete the byte
    for (int64_t byte0 = fill0 + 4 * int64_t(lane); byte0 < a.seg_bytes; byte0 += 256) {
        const int nbytes = int(std::min<int64_t>(4, a.seg_bytes - byte0));
        uint8_t* dst = seg_out + byte0;
        if (nbytes == 4 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(dst) = 0u;
        } else {
            for (int y = 0; y < nbytes; ++y) dst[y] = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------ de-matching
// tbcc_dematch_kernel's shape: one thread per output LLR (segment, block, 3i + j), the grid is exactly the work.  The stores are
// coalesced; the <= 16 reads per thread are scattered over the block's own E floats.  The copies are added in increasing index,
// one float32 addition each, a bit that is never sent is +0; with accumulate the float already there is added last.  No
// product: nothing here for the compiler to contract.
__global__ void __launch_bounds__(256) turbo_dematch_kernel(TurboDematchArgs a) {
    const int per = 3 * a.K + 12;
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= a.n_blocks * per) return;
    const int64_t blk = g / per;
    const int x = int(g - blk * per);
    const int64_t seg = blk / a.blocks_per_seg;
    const int b = int(blk - seg * a.blocks_per_seg);
    const int i = x / 3, j = x - 3 * i;
    const float* l = a.llr + seg * a.seg_stride + int64_t(b) * a.g.E;
    const int n0 = turbo_rm_first(a.g, turbo_rm_rank0(a.g, turbo_rm_rv(a.rv, a.rv_dev, seg)), i, j);
    float L = 0.f;
    if (n0 >= 0 && n0 < a.g.E) {
        L = finite_or_zero(l[n0]);
        for (int idx = n0 + a.g.navail; idx < a.g.E; idx += a.g.navail) L = L + finite_or_zero(l[idx]);
    }
    float* out = a.out + seg * a.out_stride + int64_t(b) * per + x;
    *out = a.accumulate ? *out + L : L;
}

}  // namespace

TurboRmGeom turbo_rm_geom(int K, int E, int Ncb) {
    TurboRmGeom g{};
    g.E = E;
    g.D = K + 4;
    g.Kpi = turbo_rm_kpi(K);
    g.R = g.Kpi / 32;
    g.ND = g.Kpi - g.D;
    g.Ncb = Ncb ? Ncb : 3 * g.Kpi;
    for (unsigned c = 0; c < 32; ++c) {
        unsigned p = 0u;                                     // P[c]: the 5-bit reversal of c
        for (int bit = 0; bit < 5; ++bit) p |= ((c >> bit) & 1u) << (4 - bit);
        if (int(p) < g.ND) g.mask01 |= 1u << c;
        if (int(p) < g.ND - 1) g.mask2 |= 1u << c;
    }
    g.navail = turbo_rm_count(g, g.Ncb);
    for (int rv = 0; rv < 4; ++rv) g.rank0[rv] = turbo_rm_count(g, turbo_rm_k0(K, g.Ncb, rv));
    return g;
}

int turbo_rm_group(int E, int coded_mode) {
    if (coded_mode != 1) return 1;
    int g = 8;
    while (g > 1 && (E * (g >> 1)) % 8 == 0) g >>= 1;        // 8 / gcd(E, 8)
    return g;
}

hipError_t launch_turbo_encode_rm(const TurboEncRmArgs& a, hipStream_t s) {
    const int group = turbo_rm_group(a.g.E, a.coded_mode);
    const int64_t units = a.n_seg * std::max<int64_t>(1, (int64_t(a.blocks_per_seg) + group - 1) / group);
    if (units <= 0 || a.seg_bytes <= 0) return hipSuccess;
    hipLaunchKernelGGL(turbo_encode_rm_kernel, dim3(unsigned(units)), dim3(64), size_t(8 + a.g.navail), s, a, group);
    return hipGetLastError();
}

hipError_t launch_turbo_dematch(const TurboDematchArgs& a, hipStream_t s) {
    const int64_t total = a.n_blocks * (3 * int64_t(a.K) + 12);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(turbo_dematch_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t turbo_rm_prepare() { return load_kernels(turbo_encode_rm_kernel, turbo_dematch_kernel); }

}  // namespace ofdm
