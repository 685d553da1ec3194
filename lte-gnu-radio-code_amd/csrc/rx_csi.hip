// rx_csi.hip -- channel-state-weighted max-log LLRs behind the batch receiver (gfx950): ofdm_demap_csi_frames and the |H|^2 rows
// of ofdm_rx_csi_frames.  Definition: include/ofdm_mi355x.h, "channel-state-weighted LLRs"; DESIGN.md 9.2.10.  No reference code:
// BitRecovery.py knows one sigma per buffer and a linear distance.
//
// Launches of one call (all on one stream, nothing added atomically):
//   csi_table_kernel   tab[s][j] = {s_j, a_j} (noise estimated) or {s_j, w_j} (noise given): the two divides, once per (segment, entry)
//   csi_noise_kernel   (estimated) one double and one count per (segment, slice of SEG_SLICE symbols)
//   csi_finish_kernel  a segment's partials added in a fixed order -> sigma2, n_used; (estimated) a_j -> w_j = a_j / float(sigma2)
//   csi_llr_kernel     the LLRs with the store patterns of demap_seg_soft_kernel; (given, n_used wanted) the usable counts
// Every float32 product, sum and quotient below is rounded on its own (contraction off), so the outputs are those of the NumPy
// restatement in tests/csi_ref.py bit for bit and do not depend on the path a symbol takes.
#include "ofdm_launch.hpp"
#include "soft_device.hpp"

namespace ofdm {

namespace {

// One symbol with its entry's s (0: the entry is an erasure): the usable test, d[] in ofdm_demap's bit order (b0 real axis, b1
// imaginary axis, b2 real axis, ...) and m = |u - nearest point|^2.
template <int MOD>
__device__ __forceinline__ bool csi_symbol(cf z, float s, float (&d)[MOD], float& m) {
#pragma clang fp contract(off)
    const float ur = z.x * s, ui = z.y * s;
    const bool ok = s != 0.f && soft_finite(z.x) && soft_finite(z.y) && (z.x != 0.f || z.y != 0.f) && soft_finite(ur) && soft_finite(ui);
    float dr[MOD / 2], di[MOD / 2], mr, mi;
    soft_axis<MOD>(ur, dr, mr);
    soft_axis<MOD>(ui, di, mi);
#pragma unroll
    for (int j = 0; j < MOD / 2; ++j) {
        d[2 * j] = dr[j];
        d[2 * j + 1] = di[j];
    }
    m = mr + mi;
    return ok;
}

// llr of one symbol: w * d where usable and finite, else +0
template <int MOD>
__device__ __forceinline__ bool csi_llr(cf z, float2 t, float (&o)[MOD]) {
#pragma clang fp contract(off)
    float d[MOD], m;
    const bool ok = csi_symbol<MOD>(z, t.x, d, m);
#pragma unroll
    for (int b = 0; b < MOD; ++b) {
        const float v = t.y * d[b];
        o[b] = (ok && soft_finite(v)) ? v : 0.f;
    }
    return ok;
}

}  // namespace

// tab[s][j]: s_j = (a + rho) / a where a is finite and > 0 and the quotient is finite, else 0 (an erasure).  The second word is
// a itself while the noise is still to be estimated, else w_j = a / w_den (NaN if w_den is not finite and > 0: every product
// with it fails the finite test, which makes the LLR +0).
__global__ void __launch_bounds__(256) csi_table_kernel(CsiArgs a) {
#pragma clang fp contract(off)
    const int64_t n = a.n_seg * a.row_len;
    const float w_den = float(a.noise_var);
    const bool w_ok = soft_finite(w_den) && w_den > 0.f;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
        const int64_t s = i / a.row_len;
        const int j = int(i - s * a.row_len);
        const float av = a.csi[s * a.csi_stride + j];
        const float sv = (av + a.rho) / av;
        const bool ok = soft_finite(av) && av > 0.f && soft_finite(sv);
        a.tab[i] = float2{ok ? sv : 0.f, a.est ? av : (w_ok ? av / w_den : __builtin_nanf(""))};
    }
}

// Noise terms of one (segment, slice): a lane takes symbols 2*(k*256 + lane) and the next one, k = 0..3 (one 16 B non-temporal
// load where the slice is 16-byte aligned, else two 8 B loads), and adds e = a * |u - nearest point|^2 to its running double
// ONE BY ONE in that order on both paths: the partial does not depend on the alignment of the segment.
template <int MOD>
__global__ void __launch_bounds__(256) csi_noise_kernel(CsiArgs a) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    __shared__ long long shn[4];
    const int64_t n_items = a.n_seg * a.n_slices;
    const int rl = a.row_len, step = 512 % rl;
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int64_t s = w / a.n_slices, first = (w - s * a.n_slices) * SEG_SLICE;
        const int len = int(min(int64_t(SEG_SLICE), a.seg_len - first));
        const cf* p = a.sym + s * a.seg_stride + first;
        const float2* tab = a.tab + s * rl;
        const bool wide = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
        int j = int((unsigned(first % rl) + 2u * threadIdx.x) % unsigned(rl));
        double acc = 0.0;
        long long cnt = 0;
        // all of the lane's loads first (four 16 B loads and eight table entries in flight), then the arithmetic in symbol order
        constexpr int STEPS = SEG_SLICE / 512;
        cf z[STEPS][2];
        float2 t[STEPS][2];
#pragma unroll
        for (int k = 0; k < STEPS; ++k) {
            const int i0 = 2 * (k * 256 + int(threadIdx.x));
            z[k][0] = z[k][1] = cf{0.f, 0.f};                                             // z = 0 is not usable: nothing is added
            if (wide && i0 + 1 < len) {
                const float4 v = load_stream16(reinterpret_cast<const float*>(p + i0));
                z[k][0] = cf{v.x, v.y};
                z[k][1] = cf{v.z, v.w};
            } else {
                if (i0 < len) z[k][0] = p[i0];
                if (i0 + 1 < len) z[k][1] = p[i0 + 1];
            }
            t[k][0] = tab[j];
            t[k][1] = tab[row_wrap(j + 1, rl)];
            j = row_wrap(j + step, rl);
        }
#pragma unroll
        for (int k = 0; k < STEPS; ++k) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                float d[MOD], m;
                const bool ok = csi_symbol<MOD>(z[k][e], t[k][e].x, d, m);
                const float en = t[k][e].y * m;
                if (ok && soft_finite(en)) {
                    acc += double(en);
                    cnt += 1;
                }
            }
        }
        block_sum(acc, cnt, sh, shn);
        if (threadIdx.x == 0) {
            a.part_e[w] = acc;
            a.part_n[w] = cnt;
        }
        __syncthreads();                                                                  // sh is reused by the next item
    }
}

// One workgroup per segment.  counts: part_n holds this call's counts (EST always; GIVEN when n_used is wanted).
__global__ void __launch_bounds__(256) csi_finish_kernel(CsiArgs a, int counts) {
#pragma clang fp contract(off)
    __shared__ double sh[4];
    __shared__ long long shn[4];
    for (int64_t s = blockIdx.x; s < a.n_seg; s += gridDim.x) {
        double acc = 0.0;
        long long cnt = 0;
        if (counts) {
            for (int64_t i = threadIdx.x; i < a.n_slices; i += 256) {
                if (a.est) acc += a.part_e[s * a.n_slices + i];
                cnt += a.part_n[s * a.n_slices + i];
            }
            block_sum(acc, cnt, sh, shn);
        }
        const double sigma2 = a.est ? (cnt > 0 ? acc / double(cnt) : 0.0) : a.noise_var;
        if (threadIdx.x == 0) {
            if (a.sigma2) a.sigma2[s] = sigma2;
            if (a.n_used && counts) a.n_used[s] = cnt;
        }
        if (a.est) {
            const float w_den = float(sigma2);
            const bool w_ok = soft_finite(w_den) && w_den > 0.f;
            float2* tab = a.tab + s * a.row_len;
            for (int j = threadIdx.x; j < a.row_len; j += 256) tab[j].y = w_ok ? tab[j].y / w_den : __builtin_nanf("");
        }
        __syncthreads();                                                                  // sh is reused by the next segment
    }
}

// The LLRs of one (segment, slice) per workgroup pass, stores as demap_seg_soft_kernel's llr array: QPSK two symbols per lane
// (16 B load, 16 B store), 16-QAM one symbol per lane (8 B load, 16 B store), 64-QAM a wave's tile of 128 symbols through its
// 3 KB of LDS so that every store instruction writes 1 KB contiguous.  Slices that are not 16-byte aligned in the input or the
// output, and the symbols past the last full pair / tile, take per-float stores of the same values.  A lane knows the row
// position j of its symbol: one 32-bit remainder per slice, then j advances by (lanes' stride) mod row_len.
// COUNT: the usable symbols of the slice go to part_n (noise given and n_used wanted); a.llr may then be null.
template <int MOD, bool COUNT>
__global__ void __launch_bounds__(256) csi_llr_kernel(CsiArgs a) {
#pragma clang fp contract(off)
    constexpr int TILE = 128;
    __shared__ double sh[COUNT ? 4 : 1];
    __shared__ long long shn[COUNT ? 4 : 1];
    __shared__ __attribute__((aligned(16))) float stage[MOD == 6 ? 4 : 1][MOD == 6 ? TILE * MOD : 4];
    const int64_t n_items = a.n_seg * a.n_slices;
    const int rl = a.row_len, step256 = 256 % rl, step512 = 512 % rl;
    const bool want = a.llr != nullptr;
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int64_t s = w / a.n_slices, first = (w - s * a.n_slices) * SEG_SLICE;
        const int len = int(min(int64_t(SEG_SLICE), a.seg_len - first));
        const cf* p = a.sym + s * a.seg_stride + first;
        const float2* tab = a.tab + s * rl;
        float* ql = want ? a.llr + (s * a.seg_len + first) * MOD : nullptr;
        const unsigned j0 = unsigned(first % rl);
        const bool wide = want && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(ql)) & 15) == 0;
        long long cnt = 0;
        int done = 0;                                                                     // symbols handled by the wide path
        if constexpr (MOD == 2) {
            if (wide) {
                done = len & ~1;
                int j = int((j0 + 2u * threadIdx.x) % unsigned(rl));
                for (int g = threadIdx.x; 2 * g < done; g += 256) {
                    const float4 v = load_stream16(reinterpret_cast<const float*>(p + 2 * g));
                    const float2 t0 = tab[j], t1 = tab[row_wrap(j + 1, rl)];
                    float o0[2], o1[2];
                    cnt += csi_llr<2>(cf{v.x, v.y}, t0, o0);
                    cnt += csi_llr<2>(cf{v.z, v.w}, t1, o1);
                    store_stream16(ql + 4 * g, float4{o0[0], o0[1], o1[0], o1[1]});
                    j = row_wrap(j + step512, rl);
                }
            }
        } else if constexpr (MOD == 4) {
            if (wide) {
                done = len;
                int j = int((j0 + threadIdx.x) % unsigned(rl));
                for (int i = threadIdx.x; i < len; i += 256) {
                    const float2 v = load_stream8(reinterpret_cast<const float*>(p + i));
                    float o[4];
                    cnt += csi_llr<4>(cf{v.x, v.y}, tab[j], o);
                    store_stream16(ql + 4 * i, float4{o[0], o[1], o[2], o[3]});
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
                    const float4 v = load_stream16(reinterpret_cast<const float*>(p + t * TILE + 2 * lane));
                    const float2 t0 = tab[j], t1 = tab[row_wrap(j + 1, rl)];
                    float x[6], y[6];
                    cnt += csi_llr<6>(cf{v.x, v.y}, t0, x);                                 // symbol 2*lane of the tile
                    cnt += csi_llr<6>(cf{v.z, v.w}, t1, y);                                 // symbol 2*lane + 1
                    store_tile64(ql, t, lane, st, x, y);
                    j = row_wrap(j + step512, rl);
                }
            }
        }
        {
            int j = int((j0 + unsigned(done) + threadIdx.x) % unsigned(rl));
            for (int i = done + int(threadIdx.x); i < len; i += 256) {
                float o[MOD];
                cnt += csi_llr<MOD>(p[i], tab[j], o);
                if (want) {
#pragma unroll
                    for (int b = 0; b < MOD; ++b) ql[int64_t(i) * MOD + b] = o[b];
                }
                j = row_wrap(j + step256, rl);
            }
        }
        if constexpr (COUNT) {
            double unused = 0.0;
            block_sum(unused, cnt, sh, shn);
            if (threadIdx.x == 0) a.part_n[w] = cnt;
            __syncthreads();                                                              // shn is reused by the next item
        }
    }
}

// Grid caps as rx_demap.hip's: these kernels loop with the grid as stride, and many short workgroups keep more loads in flight
// than a few long ones.
constexpr int64_t CSI_GRID_CAP = 262144;

template <int MOD>
static void launch_demap_csi_mod(const CsiArgs& a, hipStream_t s) {
    const int64_t items = a.n_seg * a.n_slices;
    const unsigned gi = unsigned(std::min<int64_t>(items, CSI_GRID_CAP));
    const unsigned gs = unsigned(std::min<int64_t>(a.n_seg, CSI_GRID_CAP));
    const unsigned gt = unsigned(std::min<int64_t>((a.n_seg * a.row_len + 255) / 256, CSI_GRID_CAP));
    hipLaunchKernelGGL(csi_table_kernel, dim3(gt), dim3(256), 0, s, a);
    if (a.est) {
        hipLaunchKernelGGL(csi_noise_kernel<MOD>, dim3(gi), dim3(256), 0, s, a);
        hipLaunchKernelGGL(csi_finish_kernel, dim3(gs), dim3(256), 0, s, a, 1);
        if (a.llr) hipLaunchKernelGGL((csi_llr_kernel<MOD, false>), dim3(gi), dim3(256), 0, s, a);
    } else {
        if (a.n_used)
            hipLaunchKernelGGL((csi_llr_kernel<MOD, true>), dim3(gi), dim3(256), 0, s, a);
        else if (a.llr)
            hipLaunchKernelGGL((csi_llr_kernel<MOD, false>), dim3(gi), dim3(256), 0, s, a);
        if (a.n_used || a.sigma2) hipLaunchKernelGGL(csi_finish_kernel, dim3(gs), dim3(256), 0, s, a, a.n_used ? 1 : 0);
    }
}

// The caller has checked the arguments and sized the workspace.
hipError_t launch_demap_csi(const CsiArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.seg_len <= 0) return hipSuccess;
    if (!a.llr && !a.sigma2 && !a.n_used) return hipSuccess;
    switch (a.mod) {
        case 2: launch_demap_csi_mod<2>(a, s); break;
        case 4: launch_demap_csi_mod<4>(a, s); break;
        case 6: launch_demap_csi_mod<6>(a, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) csi_frames_kernel(const cf* H, int N, int K, const uint16_t* src, int n_out, int64_t n_frames,
                                                         float* out, int64_t out_stride) {
#pragma clang fp contract(off)
    const int64_t n = n_frames * n_out;
    const int h = K >> 1;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
        const int64_t f = i / n_out;
        const int j = int(i - f * n_out);
        const int e = src ? int(src[j]) : j;
        const int k = e < h ? N - h + e : e - h + 1;                                       // binsP(K)
        const cf v = H[f * N + k];
        out[f * out_stride + j] = v.x * v.x + v.y * v.y;
    }
}

hipError_t launch_csi_frames(const cf* H, int nfft, int K, const uint16_t* src, int n_out, int64_t n_frames, float* out,
                             int64_t out_stride, hipStream_t s) {
    if (n_frames <= 0 || n_out <= 0) return hipSuccess;
    const unsigned g = unsigned(std::min<int64_t>((n_frames * n_out + 255) / 256, CSI_GRID_CAP));
    hipLaunchKernelGGL(csi_frames_kernel, dim3(g), dim3(256), 0, s, H, nfft, K, src, n_out, n_frames, out, out_stride);
    return hipGetLastError();
}

}  // namespace ofdm
