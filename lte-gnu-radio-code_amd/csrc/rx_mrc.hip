// rx_mrc.hip -- maximum-ratio combining of B receive branches behind the batch receiver, with max-log LLRs of the combined symbol
// (gfx950): ofdm_combine_csi_frames.  Definition: include/ofdm_mi355x.h, "receive-diversity combining"; DESIGN.md 9.2.11.  No
// reference code: the reference receiver has one antenna.
//
// Launches of one call (one stream, nothing added atomically):
//   mrc_table_kernel   tab[g][j] = {c, t} = {(a + rho) / w_den, a / w_den} per (unit g = b*n_seg + s, entry j), c = 0 where the
//                      entry is not usable: every division that depends on (g, j) alone, once; the variances used -> sigma2_out
//   mrc_llr_kernel     per output symbol: the B matched-filter terms added in branch order, two divisions, the axis rule of the
//                      channel-state-weighted LLRs, stores as csi_llr_kernel's
// Every float32 product, sum and quotient below is rounded on its own (contraction off), so the outputs are those of the NumPy
// restatement in tests/mrc_ref.py bit for bit and do not depend on the path a symbol takes.  The finite test, the streaming loads
// and stores, the row wrap and the axis rule are those of soft_device.hpp, shared with rx_csi.hip and rx_demap.hip; the 64-QAM
// tile store is this kernel's own copy of that header's store_tile64 (see there).
#include "ofdm_launch.hpp"
#include "soft_device.hpp"

namespace ofdm {

namespace {

// The sums of one output symbol: N = sum p, A = sum t over the branches that take part, from +0 in branch order.
struct MrcAcc {
    float nr, ni, a;
};

// steps 2 and 3 for one branch: t = {c, t} of its entry (c = 0: not usable).  A branch that does not take part leaves the sums.
__device__ __forceinline__ void mrc_add(MrcAcc& s, cf z, float2 t) {
#pragma clang fp contract(off)
    const float pr = z.x * t.x, pi = z.y * t.x;
    const bool in = t.x != 0.f && soft_finite(z.x) && soft_finite(z.y) && (z.x != 0.f || z.y != 0.f) && soft_finite(pr) && soft_finite(pi);
    const float nr = s.nr + pr, ni = s.ni + pi, a = s.a + t.y;
    s.nr = in ? nr : s.nr;
    s.ni = in ? ni : s.ni;
    s.a = in ? a : s.a;
}

// steps 4 to 7: u = N / A, the usable test (A > 0 holds exactly when a branch took part: every t is > 0), d[] in ofdm_demap's
// bit order, llr = A * d where finite.  Returns u and A for the other two outputs (0 where not usable).
template <int MOD>
__device__ __forceinline__ void mrc_finish(MrcAcc s, float (&o)[MOD], cf& u, float& w) {
#pragma clang fp contract(off)
    const float ur = s.nr / s.a, ui = s.ni / s.a;
    const bool ok = soft_finite(s.a) && s.a > 0.f && soft_finite(ur) && soft_finite(ui);
    float dr[MOD / 2], di[MOD / 2], unused;                                               // the smallest distance is not needed here
    soft_axis<MOD>(ur, dr, unused);
    soft_axis<MOD>(ui, di, unused);
#pragma unroll
    for (int j = 0; j < MOD / 2; ++j) {
        const float vr = s.a * dr[j], vi = s.a * di[j];
        o[2 * j] = (ok && soft_finite(vr)) ? vr : 0.f;
        o[2 * j + 1] = (ok && soft_finite(vi)) ? vi : 0.f;
    }
    u = ok ? cf{ur, ui} : cf{0.f, 0.f};
    w = ok ? s.a : 0.f;
}

// The branch loop is a runtime loop in rounds of MRC_ROUND branches: a lane issues the symbol loads and the table entries of a
// whole round before any arithmetic (B <= 2: all of them), which bounds the registers the loads hold whatever B is.  Rounds of 4
// cost 26 to 40 VGPRs more and were slower at B = 2 and B = 4 alike.  A slot past the last branch holds
// z = 0 and c = 0: it does not take part.
constexpr int MRC_ROUND = 2;

}  // namespace

// tab[g][j], g = b*n_seg + s: c = (a + rho) / w_den, t = a / w_den; the entry is usable iff a and w_den are finite and > 0, c is
// finite, t is finite and > 0 (then c >= t > 0: c = 0 can mark the others).  The lane of entry 0 writes the unit's variance.
__global__ void __launch_bounds__(256) mrc_table_kernel(MrcArgs a) {
#pragma clang fp contract(off)
    const int64_t units = int64_t(a.n_branch) * a.n_seg;
    const int64_t n = units * a.row_len;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
        const int64_t g = i / a.row_len;
        const int j = int(i - g * a.row_len);
        const double var = a.sigma2 ? a.sigma2[g] : a.noise_var[g / a.n_seg];
        const float w_den = float(var);
        const float av = a.csi[g * a.csi_stride + j];
        const float c = (av + a.rho) / w_den, t = av / w_den;
        const bool ok = soft_finite(av) && av > 0.f && soft_finite(w_den) && w_den > 0.f && soft_finite(c) && soft_finite(t) && t > 0.f;
        a.tab[i] = ok ? float2{c, t} : float2{0.f, 0.f};
        if (j == 0 && a.sigma2_out) a.sigma2_out[g] = var;
    }
}

// One (output segment, slice of SEG_SLICE symbols) per workgroup pass; work split, alignment rule and store patterns of
// csi_llr_kernel: QPSK two symbols per lane (16 B loads, 16 B llr store), 16-QAM one symbol per lane (8 B loads, 16 B store),
// 64-QAM a wave's tile of 128 symbols through its 3 KB of LDS so that every llr store instruction writes 1 KB contiguous.
// Slices where a branch's input or a wanted output is not 16-byte aligned, and the symbols past the last full pair / tile, take
// per-float stores of the same values.  MORE: sym or weight may be wanted (each skipped by a wave-uniform branch where it is
// not); the llr-only kernel does without their pointers, which is what keeps it free of SGPR spills.  Lane offsets are unsigned
// 32-bit numbers against wave-uniform bases, so the loads take their base from scalar registers.
template <int MOD, bool MORE>
__global__ void __launch_bounds__(256) mrc_llr_kernel(MrcArgs a) {
#pragma clang fp contract(off)
    constexpr int TILE = 128;
    __shared__ __attribute__((aligned(16))) float stage[MOD == 6 ? 4 : 1][MOD == 6 ? TILE * MOD : 4];
    const int64_t n_items = a.n_seg * a.n_slices;
    const int rl = a.row_len, step256 = 256 % rl, step512 = 512 % rl;
    const int B = a.n_branch;
    const int64_t zb = a.n_seg * a.seg_stride;                                            // branch to branch, complex items
    const int64_t tb = a.n_seg * int64_t(rl);                                             //                   table entries
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int64_t s = w / a.n_slices, first = (w - s * a.n_slices) * SEG_SLICE;
        const int len = int(min(int64_t(SEG_SLICE), a.seg_len - first));
        const cf* p = a.sym + s * a.seg_stride + first;                                   // branch 0
        const float2* tab = a.tab + s * rl;
        const int64_t o0 = s * a.seg_len + first;
        float* ql = a.llr ? a.llr + o0 * MOD : nullptr;
        cf* qs = MORE && a.osym ? a.osym + o0 : nullptr;
        float* qw = MORE && a.weight ? a.weight + o0 : nullptr;
        const unsigned j0 = unsigned(first % rl);
        // 16 B for the llr stores and the inputs; two symbols per lane: 16 B for sym, 8 B for weight (one: theirs by type)
        uintptr_t bits = reinterpret_cast<uintptr_t>(ql);
        if constexpr (MOD != 4) bits |= reinterpret_cast<uintptr_t>(qs) | (reinterpret_cast<uintptr_t>(qw) << 1);
        for (int b = 0; b < B; ++b) bits |= reinterpret_cast<uintptr_t>(p + b * zb);
        const bool wide = (bits & 15) == 0;
        int done = 0;                                                                     // symbols handled by the wide path
        if constexpr (MOD == 2) {
            if (wide) {
                done = len & ~1;
                int j = int((j0 + 2u * threadIdx.x) % unsigned(rl));
                for (int g = threadIdx.x; 2 * g < done; g += 256) {
                    const int j1 = row_wrap(j + 1, rl);
                    MrcAcc s0{0.f, 0.f, 0.f}, s1{0.f, 0.f, 0.f};
                    for (int b0 = 0; b0 < B; b0 += MRC_ROUND) {
                        float4 v[MRC_ROUND];
                        float2 t0[MRC_ROUND], t1[MRC_ROUND];
#pragma unroll
                        for (int k = 0; k < MRC_ROUND; ++k) {
                            v[k] = float4{0.f, 0.f, 0.f, 0.f};
                            t0[k] = t1[k] = float2{0.f, 0.f};
                            if (b0 + k < B) {
                                v[k] = load_stream16(reinterpret_cast<const float*>(p + (b0 + k) * zb) + 4u * unsigned(g));
                                t0[k] = (tab + (b0 + k) * tb)[unsigned(j)];
                                t1[k] = (tab + (b0 + k) * tb)[unsigned(j1)];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < MRC_ROUND; ++k) {
                            mrc_add(s0, cf{v[k].x, v[k].y}, t0[k]);
                            mrc_add(s1, cf{v[k].z, v[k].w}, t1[k]);
                        }
                    }
                    float x[2], y[2], w0, w1;
                    cf u0, u1;
                    mrc_finish<2>(s0, x, u0, w0);
                    mrc_finish<2>(s1, y, u1, w1);
                    if (ql) store_stream16(ql + 4 * g, float4{x[0], x[1], y[0], y[1]});
                    if (qs) store_stream16(reinterpret_cast<float*>(qs + 2 * g), float4{u0.x, u0.y, u1.x, u1.y});
                    if (qw) store_stream8(qw + 2 * g, float2{w0, w1});
                    j = row_wrap(j + step512, rl);
                }
            }
        } else if constexpr (MOD == 4) {
            if (wide) {
                done = len;
                int j = int((j0 + threadIdx.x) % unsigned(rl));
                for (int i = threadIdx.x; i < len; i += 256) {
                    MrcAcc s0{0.f, 0.f, 0.f};
                    for (int b0 = 0; b0 < B; b0 += MRC_ROUND) {
                        float2 v[MRC_ROUND], t0[MRC_ROUND];
#pragma unroll
                        for (int k = 0; k < MRC_ROUND; ++k) {
                            v[k] = t0[k] = float2{0.f, 0.f};
                            if (b0 + k < B) {
                                v[k] = load_stream8(reinterpret_cast<const float*>(p + (b0 + k) * zb) + 2u * unsigned(i));
                                t0[k] = (tab + (b0 + k) * tb)[unsigned(j)];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < MRC_ROUND; ++k) mrc_add(s0, cf{v[k].x, v[k].y}, t0[k]);
                    }
                    float o[4], w0;
                    cf u0;
                    mrc_finish<4>(s0, o, u0, w0);
                    if (ql) store_stream16(ql + 4 * i, float4{o[0], o[1], o[2], o[3]});
                    if (qs) store_stream8(reinterpret_cast<float*>(qs + i), float2{u0.x, u0.y});
                    if (qw) __builtin_nontemporal_store(w0, qw + i);
                    j = row_wrap(j + step256, rl);
                }
            }
        } else {
            if (wide) {
                const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
                const int n_tiles = len / TILE;
                done = n_tiles * TILE;
                float* st = stage[wave];
                int j = int((j0 + unsigned(wave * TILE + 2 * lane)) % unsigned(rl));
                for (int t = wave; t < n_tiles; t += 4) {
                    const int j1 = row_wrap(j + 1, rl), i0 = t * TILE + 2 * lane;
                    MrcAcc s0{0.f, 0.f, 0.f}, s1{0.f, 0.f, 0.f};
                    for (int b0 = 0; b0 < B; b0 += MRC_ROUND) {
                        float4 v[MRC_ROUND];
                        float2 t0[MRC_ROUND], t1[MRC_ROUND];
#pragma unroll
                        for (int k = 0; k < MRC_ROUND; ++k) {
                            v[k] = float4{0.f, 0.f, 0.f, 0.f};
                            t0[k] = t1[k] = float2{0.f, 0.f};
                            if (b0 + k < B) {
                                v[k] = load_stream16(reinterpret_cast<const float*>(p + (b0 + k) * zb) + 2u * unsigned(i0));
                                t0[k] = (tab + (b0 + k) * tb)[unsigned(j)];
                                t1[k] = (tab + (b0 + k) * tb)[unsigned(j1)];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < MRC_ROUND; ++k) {
                            mrc_add(s0, cf{v[k].x, v[k].y}, t0[k]);
                            mrc_add(s1, cf{v[k].z, v[k].w}, t1[k]);
                        }
                    }
                    float x[6], y[6], w0, w1;
                    cf u0, u1;
                    mrc_finish<6>(s0, x, u0, w0);                                         // symbol 2*lane of the tile
                    mrc_finish<6>(s1, y, u1, w1);                                         // symbol 2*lane + 1
                    if (qs) store_stream16(reinterpret_cast<float*>(qs + i0), float4{u0.x, u0.y, u1.x, u1.y});
                    if (qw) store_stream8(qw + i0, float2{w0, w1});
                    if (ql) {
                        // store_tile64 of soft_device.hpp written out: through it this kernel's prologue came out in another order,
                        // and the timing against the parent's library did not hold its bound (profiles/soft_stage_header_ab.txt).
                        // Through the wave's 3 KB: 12 floats per lane in, 3 x 16 B per lane out.
                        float4* wr = reinterpret_cast<float4*>(st + lane * 12);
                        wr[0] = float4{x[0], x[1], x[2], x[3]};
                        wr[1] = float4{x[4], x[5], y[0], y[1]};
                        wr[2] = float4{y[2], y[3], y[4], y[5]};
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // wave-local exchange: in order per wave
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const int piece = k * 64 + lane;
                            store_stream16(ql + int64_t(t) * (TILE * 6) + 4 * piece, *reinterpret_cast<const float4*>(st + 4 * piece));
                        }
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                // reads done before the stage is rewritten
                    }
                    j = row_wrap(j + step512, rl);
                }
            }
        }
        {
            int j = int((j0 + unsigned(done) + threadIdx.x) % unsigned(rl));
            for (int i = done + int(threadIdx.x); i < len; i += 256) {
                MrcAcc s0{0.f, 0.f, 0.f};
                for (int b0 = 0; b0 < B; b0 += MRC_ROUND) {
                    cf v[MRC_ROUND];
                    float2 t0[MRC_ROUND];
#pragma unroll
                    for (int k = 0; k < MRC_ROUND; ++k) {
                        v[k] = cf{0.f, 0.f};
                        t0[k] = float2{0.f, 0.f};
                        if (b0 + k < B) {
                            v[k] = p[(b0 + k) * zb + i];
                            t0[k] = (tab + (b0 + k) * tb)[unsigned(j)];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < MRC_ROUND; ++k) mrc_add(s0, v[k], t0[k]);
                }
                float o[MOD], w0;
                cf u0;
                mrc_finish<MOD>(s0, o, u0, w0);
                if (ql) {
#pragma unroll
                    for (int b = 0; b < MOD; ++b) ql[int64_t(i) * MOD + b] = o[b];
                }
                if (qs) {
                    reinterpret_cast<float*>(qs + i)[0] = u0.x;
                    reinterpret_cast<float*>(qs + i)[1] = u0.y;
                }
                if (qw) qw[i] = w0;
                j = row_wrap(j + step256, rl);
            }
        }
    }
}

// Grid caps as rx_csi.hip's: the kernels loop with the grid as stride.
constexpr int64_t MRC_GRID_CAP = 262144;

template <int MOD>
static void launch_mrc_llr(const MrcArgs& a, bool more, unsigned grid, hipStream_t s) {
    if (more)
        hipLaunchKernelGGL((mrc_llr_kernel<MOD, true>), dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((mrc_llr_kernel<MOD, false>), dim3(grid), dim3(256), 0, s, a);
}

// The table alone, for the stage that despreads what it combines (mrc_despread.hip).  The caller has sized the table.
hipError_t launch_mrc_table(const MrcArgs& a, hipStream_t s) {
    const int64_t entries = int64_t(a.n_branch) * a.n_seg * a.row_len;
    if (entries <= 0) return hipSuccess;
    const unsigned gt = unsigned(std::min<int64_t>((entries + 255) / 256, MRC_GRID_CAP));
    hipLaunchKernelGGL(mrc_table_kernel, dim3(gt), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t mrc_table_prepare() { return load_kernels(mrc_table_kernel); }

// The caller has checked the arguments and sized the table.
hipError_t launch_combine_mrc(const MrcArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.seg_len <= 0 || a.n_branch <= 0) return hipSuccess;
    const bool want = a.llr || a.osym || a.weight;
    if (!want && !a.sigma2_out) return hipSuccess;
    const int64_t entries = int64_t(a.n_branch) * a.n_seg * a.row_len;
    const unsigned gt = unsigned(std::min<int64_t>((entries + 255) / 256, MRC_GRID_CAP));
    const unsigned gi = unsigned(std::min<int64_t>(a.n_seg * a.n_slices, MRC_GRID_CAP));
    if (a.mod != 2 && a.mod != 4 && a.mod != 6) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrc_table_kernel, dim3(gt), dim3(256), 0, s, a);
    if (want) {
        const bool more = a.osym || a.weight;
        switch (a.mod) {
            case 2: launch_mrc_llr<2>(a, more, gi, s); break;
            case 4: launch_mrc_llr<4>(a, more, gi, s); break;
            default: launch_mrc_llr<6>(a, more, gi, s); break;
        }
    }
    return hipGetLastError();
}

}  // namespace ofdm
