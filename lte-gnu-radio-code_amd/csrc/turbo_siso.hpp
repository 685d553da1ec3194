// turbo_siso.hpp -- one half-iteration (one SISO run over a block's K steps) of the turbo decoders' wave mapping, shared by
// turbo_decode_kernel (turbo.hip) and turbo_decode_es_kernel (turbo_es.hip): the lane constants, the tile load, the forward
// tile, the tail and the backward tile.  The mapping itself is described in front of turbo_decode_kernel.
//
// Arithmetic: the contract fixes every float32 operation and its order, so nothing here may be contracted.  The pragma below
// holds from here to the end of the translation unit; both files that include this header set it themselves as well, and no
// other file may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "ofdm_launch.hpp"
#include "turbo_device.hpp"

#pragma clang fp contract(off)

namespace ofdm {

namespace {

__device__ __forceinline__ float turbo_group_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    return fmaxf(v, __shfl_xor(v, 4, 64));
}

constexpr int TURBO_ROW = TURBO_CKPT + 1;                    // padded row of the per-group tile arrays

struct TurboLane {
    // forward, lane = s': its predecessors are p0 = 2 (s' & 3) (r3 = 0) and p0 + 1 (r3 = 1); with a = s' >> 2, r1 = (s' >> 1) & 1,
    // r2 = s' & 1 the p0 branch carries u = a ^ r2, z = a ^ r1, and the other branch has both flipped: its gamma is exactly -gamma.
    float f_su, f_sz;
    int addr_s0, addr_p0, addr_p1;
    // backward, lane = s = 4 r1 + 2 r2 + r3: input 0 gives a = r2 ^ r3, z = r1 ^ r2 and next = 4 a + (s >> 1); input 1 flips a and z
    float b_sz;
    int addr_n0, addr_n1;
    // tail, lane = s: the terminating path s, s >> 1, s >> 2 with the signs of (r2 ^ r3, r1 ^ r3) at each of its states
    float t_s0, t_s1, t_s2, t_s3, t_s4;
};

__device__ __forceinline__ TurboLane turbo_lane(int grp, int st) {
    TurboLane c;
    const int f_a = st >> 2, f_r1 = (st >> 1) & 1, f_r2 = st & 1;
    c.f_su = (f_a ^ f_r2) ? -1.f : 1.f, c.f_sz = (f_a ^ f_r1) ? -1.f : 1.f;
    c.addr_s0 = (grp << 3) << 2;
    c.addr_p0 = c.addr_s0 + ((2 * (st & 3)) << 2), c.addr_p1 = c.addr_p0 + 4;
    const int b_r1 = st >> 2, b_r2 = (st >> 1) & 1, b_r3 = st & 1;
    c.b_sz = (b_r1 ^ b_r2) ? -1.f : 1.f;
    const int n0 = ((b_r2 ^ b_r3) << 2) | (st >> 1);
    c.addr_n0 = c.addr_s0 + (n0 << 2), c.addr_n1 = c.addr_s0 + ((n0 ^ 4) << 2);
    c.t_s0 = (b_r2 ^ b_r3) ? -1.f : 1.f, c.t_s1 = (b_r1 ^ b_r3) ? -1.f : 1.f;
    c.t_s2 = (b_r1 ^ b_r2) ? -1.f : 1.f, c.t_s3 = b_r2 ? -1.f : 1.f;
    c.t_s4 = b_r1 ? -1.f : 1.f;
    return c;
}

// Half-iteration `half` (0: decoder 1 in natural order, 1: decoder 2 through pi) of the wave's 8 blocks.  llr, ext and post are
// the group's own block, ckpt the lane's own column; sm_a is [TURBO_CKPT][64], my_x and my_i the group's padded rows.  `first`:
// la1 = 0.  Ends with the barrier that puts the stores in front of the next loads.  Every lane of the wave has to be here.
template <bool ES>
__device__ __forceinline__ void turbo_half_iteration(const TurboQpp& q, const float* llr, float* ext, float* post_arr, float* ckpt,
                                                     bool active, bool store, int half, bool first, bool want_post, const TurboLane& c,
                                                     float* sm_a, float2* my_x, int* my_i, int lane, int st) {
    const int K = q.K;
    const unsigned uK = unsigned(K);
    const int n_tiles = (K + TURBO_CKPT - 1) / TURBO_CKPT;

    // lane st of a group loads steps k0 + st, k0 + st + 8, ..: pi steps by 8 with pi(i + 8) - pi(i) = 8 f1 + f2 (16 i + 64)
    auto load_tile = [&](int k0, int n) {
        __syncthreads();
        unsigned i = unsigned(k0 + st);
        unsigned p = 0u, g = 0u;
        if (half) {
            p = turbo_qpp_at(q, i);
            g = (unsigned(q.c8) + (unsigned(q.c16) * i) % uK) % uK;
        }
        for (int j = st; j < n; j += 8, i += 8) {
            float x = 0.f, lp = 0.f;
            const unsigned idx = half ? p : i;
            if (active) {
                const float la = first ? 0.f : ext[idx];
                x = finite_or_zero(llr[3 * idx]) + la;
                lp = finite_or_zero(llr[3 * i + 1 + half]);
            }
            my_x[j] = make_float2(x, lp);
            my_i[j] = int(idx);
            p = turbo_mod_add(p, g, uK);
            g = turbo_mod_add(g, unsigned(q.c128), uK);
        }
        __syncthreads();
    };
    // A_k -> A_{k+n} over the loaded tile; n is a multiple of 8 and so is the tile's first step
    auto forward_tile = [&](float A, int n, bool keep) -> float {
        for (int j8 = 0; j8 < n; j8 += 8) {
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const float2 xl = my_x[j8 + v];
                if (keep) sm_a[((j8 + v) << 6) + lane] = A;
                const float gm = __builtin_fmaf(c.f_sz, xl.y, c.f_su * xl.x);
                const float c0 = bperm(c.addr_p0, A) + gm;
                const float c1 = bperm(c.addr_p1, A) - gm;
                A = fmaxf(c0, c1);
                if (v == 7) A = A - bperm(c.addr_s0, A);
            }
        }
        return A;
    };

    float A = st == 0 ? 0.f : -INFINITY;
    for (int t = 0; t < n_tiles; ++t) {
        const int k0 = t * TURBO_CKPT, n = std::min(TURBO_CKPT, K - k0);
        load_tile(k0, n);
        if (!ES || store) ckpt[int64_t(t) << 6] = A;
        A = forward_tile(A, n, false);
    }

    float B;
    {
        float t[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) t[j] = active ? finite_or_zero(llr[3 * K + 6 * half + j]) : 0.f;
        const float g0 = __builtin_fmaf(c.t_s1, t[1], c.t_s0 * t[0]);
        const float g1 = __builtin_fmaf(c.t_s3, t[3], c.t_s2 * t[2]);
        const float g2 = __builtin_fmaf(c.t_s4, t[5], c.t_s4 * t[4]);
        const float bs = (g0 + g1) + g2;
        B = bs - bperm(c.addr_s0, bs);
    }

    for (int t = n_tiles - 1; t >= 0; --t) {
        const int k0 = t * TURBO_CKPT, n = std::min(TURBO_CKPT, K - k0);
        load_tile(k0, n);
        forward_tile(ckpt[int64_t(t) << 6], n, true);
        for (int j8 = n - 8; j8 >= 0; j8 -= 8) {
            float mine = 0.f, mine_post = 0.f;
#pragma unroll
            for (int v = 7; v >= 0; --v) {
                const float2 xl = my_x[j8 + v];
                const float Ak = sm_a[((j8 + v) << 6) + lane];
                const float gm = __builtin_fmaf(c.b_sz, xl.y, xl.x);                 // gamma of input 0; input 1 has -gamma
                const float b0 = bperm(c.addr_n0, B), b1 = bperm(c.addr_n1, B);
                const float m0 = turbo_group_max((Ak + gm) + b0);
                const float m1 = turbo_group_max((Ak - gm) + b1);
                const float post = 0.5f * (m0 - m1);
                const float e = 0.75f * (post - xl.x);
                if (v == st) {
                    if (ES) {
                        mine = e;
                        mine_post = post;
                    } else {
                        mine = want_post ? post : e;
                    }
                }
                float nb = fmaxf(gm + b0, b1 - gm);
                if (v == 0) nb = nb - bperm(c.addr_s0, nb);
                B = nb;
            }
            if (store) {
                const int at = my_i[j8 + st];
                ext[at] = mine;
                if (ES && want_post) post_arr[at] = mine_post;
            }
        }
    }
    __syncthreads();                                         // the half-iteration's stores, before the next one's loads
}

}  // namespace

}  // namespace ofdm
