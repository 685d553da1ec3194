// rx_demap.hip -- stand-alone de-mappers (gfx950): BitRecovery hard / max-log soft outputs
// (reference: LEGACY/gr-ofdm-rx/python/BitRecovery.py:66-157), whole buffers and per-frame segments.
#include "ofdm_launch.hpp"
#include "demap_hard.hpp"
#include "soft_device.hpp"

namespace ofdm {

// ------------------------------------------------------------------------------------------ standalone de-mapper
// Hard bits, one per byte.  A thread takes FOUR consecutive symbols (two 16 B loads) and writes their 4*MOD bytes as whole
// words (byte-by-byte stores, one symbol per thread, ran at 0.36-0.64 of the HBM rate); the last n % 4 symbols and buffers that
// are not 16-byte aligned take the plain path.
template <int MOD>
__device__ __forceinline__ void demap_hard_words(const cf (&z)[4], uint32_t (&w)[MOD]) {
#pragma unroll
    for (int k = 0; k < MOD; ++k) w[k] = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned hb = hard_bits<MOD>(z[e]);
#pragma unroll
        for (int j = 0; j < MOD; ++j) {
            const int k = e * MOD + j;                                 // byte index in the group's 4*MOD bytes
            w[k >> 2] |= ((hb >> (MOD - 1 - j)) & 1u) << (8 * (k & 3));
        }
    }
}
__device__ __forceinline__ void qpsk_nearest(cf z, bool& re_pos, bool& im_pos, cf& e) {
    // quadrant tests in the reference's order ++, -+, --, +- (BitRecovery.py:106-125)
    re_pos = (z.x > 0.f) || (z.x == 0.f && z.y >= 0.f);
    im_pos = (z.y >= 0.f);
    constexpr float c = 0.70710678118654752f;
    e = cf{z.x - (re_pos ? c : -c), z.y - (im_pos ? c : -c)};                            // :93-98
}

// pass 2: llrp0 / llrp1 (BitRecovery.py:102-125)
__global__ void __launch_bounds__(256) demap_soft_kernel(DemapArgs a) {
    __shared__ double sh_tot;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < DEMAP_PARTIALS; ++i) s += a.partial[i];
        sh_tot = s;
    }
    __syncthreads();
    const double sigma = 0.7071067811865476 * (sh_tot / double(a.n));                    // :102
    const float hf = float(-0.5 / (sigma * sigma));                                      // -0.5*dfact :103
    constexpr float K = 1.414213562373095f;                                              // :57
    auto metrics = [&](cf z, float (&m0)[2], float (&m1)[2]) {
        bool rp, ip;
        cf e;
        qpsk_nearest(z, rp, ip, e);
        const float nr = hf * fabsf(e.x), fr = hf * (K - fabsf(e.x));
        const float ni = hf * fabsf(e.y), fi = hf * (K - fabsf(e.y));
        m0[0] = rp ? nr : fr;
        m0[1] = ip ? ni : fi;
        m1[0] = rp ? fr : nr;
        m1[1] = ip ? fi : ni;
    };
    // two symbols per thread: one 16 B load, one 16 B store per metric array (buffers 16-byte aligned; else one by one)
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    const bool wide = ((reinterpret_cast<uintptr_t>(a.sym) | reinterpret_cast<uintptr_t>(a.soft0) | reinterpret_cast<uintptr_t>(a.soft1)) & 15) == 0;
    const int64_t n2 = wide ? a.n >> 1 : 0;
    for (int64_t g = gid; g < n2; g += stride) {
        const float4 v = reinterpret_cast<const float4*>(a.sym)[g];
        float a0[2], a1[2], b0[2], b1[2];
        metrics(cf{v.x, v.y}, a0, a1);
        metrics(cf{v.z, v.w}, b0, b1);
        if (a.soft0) store_stream16(a.soft0 + 4 * g, float4{a0[0], a0[1], b0[0], b0[1]});
        if (a.soft1) store_stream16(a.soft1 + 4 * g, float4{a1[0], a1[1], b1[0], b1[1]});
    }
    for (int64_t i = n2 * 2 + gid; i < a.n; i += stride) {
        float m0[2], m1[2];
        metrics(a.sym[i], m0, m1);
        if (a.soft0) {
            a.soft0[2 * i] = m0[0];
            a.soft0[2 * i + 1] = m0[1];
        }
        if (a.soft1) {
            a.soft1[2 * i] = m1[0];
            a.soft1[2 * i + 1] = m1[1];
        }
    }
}

// ---- 16/64-QAM extension of the soft metric (no reference code: BitRecovery.py knows QPSK only).
// Same structure as BitRecovery.work: sigma = 0.7071 * mean distance to the nearest point over the buffer, per-bit
// metrics -0.5/sigma^2 * (linear distance), taken per axis to the nearest PAM level that carries bit value 0 / 1.
// Axis levels l_q = (2q - (M-1)) * u, q = 0..M-1, M = 4 (u = 1/sqrt(10)) or 8 (u = 1/sqrt(42)); TS 36.211 7.1 labels:
// bit 0 = (l < 0); 16-QAM bit 1 = (|m| == 3); 64-QAM bit 1 = (|m| > 4), bit 2 = (|m| == 1 or 7), m = 2q-(M-1).
template <int BPS>
struct Pam {
    static constexpr int M = BPS == 4 ? 4 : 8;
    static constexpr int NB = BPS / 2;
    static __device__ __forceinline__ float unit() { return BPS == 4 ? 0.31622776601683794f : 0.15430334996209191f; }
    static __device__ __forceinline__ bool label(int q, int j) {
        const int m = 2 * q - (M - 1), am = m < 0 ? -m : m;
        if (j == 0) return m < 0;
        if (BPS == 4) return am == 3;
        return j == 1 ? am > 4 : (am == 1 || am == 7);
    }
    // distances from coordinate x to the nearest level with axis bit j = 0 / 1, and to the nearest level overall
    static __device__ __forceinline__ void dist(float x, float (&d0)[NB], float (&d1)[NB], float& e) {
        const float u = unit();
        e = 3.0e38f;
#pragma unroll
        for (int j = 0; j < NB; ++j) d0[j] = d1[j] = 3.0e38f;
#pragma unroll
        for (int q = 0; q < M; ++q) {
            const float d = fabsf(x - float(2 * q - (M - 1)) * u);
            e = fminf(e, d);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (label(q, j))
                    d1[j] = fminf(d1[j], d);
                else
                    d0[j] = fminf(d0[j], d);
            }
        }
    }
};

// distance of one symbol to its nearest constellation point (BitRecovery.py:87-88; the QAM extension's own definition)
template <int MOD>
__device__ __forceinline__ float demap_dmin(cf z) {
    if constexpr (MOD == 2) {
        bool rp, ip;
        cf e;
        qpsk_nearest(z, rp, ip, e);
        return sqrtf(cnorm2(e));
    } else {
        float d0[Pam<MOD>::NB], d1[Pam<MOD>::NB], ex, ey;
        Pam<MOD>::dist(z.x, d0, d1, ex);
        Pam<MOD>::dist(z.y, d0, d1, ey);
        return sqrtf(ex * ex + ey * ey);
    }
}

// Pass 1 of the de-mapper, ONE read of the symbols: hard bits (one per byte; a thread takes FOUR consecutive symbols -- two 16 B
// loads -- and writes their 4*MOD bytes as whole words) and / or the partial sums of the nearest-point distances that sigma
// needs (BitRecovery.py:88,102: double partial sums, added atomically into DEMAP_PARTIALS slots zeroed by the launcher).
// Round 2 ran these as two kernels: hard + soft output read every symbol three times.
template <int MOD, bool HARD, bool DMIN>
__global__ void __launch_bounds__(256) demap_pass1_kernel(DemapArgs a) {
    const int64_t n = a.n, n4 = n >> 2;
    const bool wide = ((reinterpret_cast<uintptr_t>(a.sym) | (HARD ? reinterpret_cast<uintptr_t>(a.hard) : 0)) & 15) == 0;
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    double acc = 0.0;
    if (wide) {
        for (int64_t g = gid; g < n4; g += stride) {
            const float4 v0 = load_stream16(reinterpret_cast<const float*>(a.sym) + 8 * g),
                         v1 = load_stream16(reinterpret_cast<const float*>(a.sym) + 8 * g + 4);
            const cf z[4] = {cf{v0.x, v0.y}, cf{v0.z, v0.w}, cf{v1.x, v1.y}, cf{v1.z, v1.w}};
            if constexpr (DMIN) {
                // four float distances summed in float (exact enough: 4 terms), the running sum in double
                acc += double((demap_dmin<MOD>(z[0]) + demap_dmin<MOD>(z[1])) + (demap_dmin<MOD>(z[2]) + demap_dmin<MOD>(z[3])));
            }
            if constexpr (HARD) {
                uint32_t w[MOD];
                demap_hard_words<MOD>(z, w);
                uint32_t* o = reinterpret_cast<uint32_t*>(a.hard + g * 4 * MOD);
                if constexpr (MOD == 4) {
                    *reinterpret_cast<uint4*>(o) = uint4{w[0], w[1], w[2], w[3]};
                } else if constexpr (MOD == 1) {
                    o[0] = w[0];
                } else {                                                   // 8 or 24 bytes, 8-byte aligned
#pragma unroll
                    for (int k = 0; k < MOD; k += 2) *reinterpret_cast<uint2*>(o + k) = uint2{w[k], w[k + 1]};
                }
            }
        }
    }
    for (int64_t i = (wide ? n4 * 4 : 0) + gid; i < n; i += stride) {
        const cf z = a.sym[i];
        if constexpr (DMIN) acc += double(demap_dmin<MOD>(z));
        if constexpr (HARD) {
            const unsigned hb = hard_bits<MOD>(z);
#pragma unroll
            for (int b = 0; b < MOD; ++b) a.hard[i * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
        }
    }
    if constexpr (DMIN) {
        __shared__ double sh[256];
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
            __syncthreads();
        }
        // more workgroups than partial slots (256 of them cannot keep the memory system busy)
        if (threadIdx.x == 0) atomicAdd(a.partial + (blockIdx.x % DEMAP_PARTIALS), sh[0]);
    }
}

template <int BPS>
__global__ void __launch_bounds__(256) demap_soft_qam_kernel(DemapArgs a) {
    __shared__ double sh_tot;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < DEMAP_PARTIALS; ++i) s += a.partial[i];
        sh_tot = s;
    }
    __syncthreads();
    const double sigma = 0.7071067811865476 * (sh_tot / double(a.n));
    const float hf = float(-0.5 / (sigma * sigma));
    constexpr int NB = Pam<BPS>::NB;
    const bool wide = ((reinterpret_cast<uintptr_t>(a.soft0) | reinterpret_cast<uintptr_t>(a.soft1)) & 15) == 0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += int64_t(gridDim.x) * blockDim.x) {
        const cf z = a.sym[i];
        float r0[NB], r1[NB], i0[NB], i1[NB], e;
        Pam<BPS>::dist(z.x, r0, r1, e);
        Pam<BPS>::dist(z.y, i0, i1, e);
        float o0[BPS], o1[BPS];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            o0[2 * j] = hf * r0[j];
            o0[2 * j + 1] = hf * i0[j];
            o1[2 * j] = hf * r1[j];
            o1[2 * j + 1] = hf * i1[j];
        }
        // BPS floats per symbol = 16 B (16-QAM: one 16 B store where the buffer allows it) / 24 B (64-QAM: three 8 B stores)
        if (BPS == 4 && wide) {
            if (a.soft0) store_stream16(a.soft0 + i * BPS, float4{o0[0], o0[1], o0[2], o0[3]});
            if (a.soft1) store_stream16(a.soft1 + i * BPS, float4{o1[0], o1[1], o1[2], o1[3]});
        } else {
#pragma unroll
            for (int b = 0; b < BPS; b += 2) {
                if (a.soft0) *reinterpret_cast<float2*>(a.soft0 + i * BPS + b) = make_float2(o0[b], o0[b + 1]);
                if (a.soft1) *reinterpret_cast<float2*>(a.soft1 + i * BPS + b) = make_float2(o1[b], o1[b + 1]);
            }
        }
    }
}

// 64-QAM soft metrics with DENSE stores.  A symbol owns 6 floats per metric array, so a lane that keeps "its" symbols writes 24 B
// pieces at a 24 B stride: every store instruction of a wave touches 12+ lines partially (0.39 of the HBM rate with both arrays,
// round 2).  Here a wave takes a tile of 128 symbols (one 16 B load per lane = 2 symbols), parks each array's 768 floats in LDS
// in symbol order and writes them back as 192 pieces of 16 B, piece k*64 + lane per store instruction: 1 KB contiguous, written
// once, non-temporal.  The staging area is private to the wave (LDS is in order per wave: a counter wait, no barrier).
__global__ void __launch_bounds__(256) demap_soft_qam64_kernel(DemapArgs a) {
    constexpr int BPS = 6, NB = 3, TILE = 128;
    __shared__ __attribute__((aligned(16))) float stage[4][2][TILE * BPS];               // 4 waves x 2 arrays x 3 KB
    __shared__ double sh_tot;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < DEMAP_PARTIALS; ++i) s += a.partial[i];
        sh_tot = s;
    }
    __syncthreads();
    const double sigma = 0.7071067811865476 * (sh_tot / double(a.n));
    const float hf = float(-0.5 / (sigma * sigma));
    auto metrics = [&](cf z, float (&o0)[BPS], float (&o1)[BPS]) {
        float r0[NB], r1[NB], i0[NB], i1[NB], e;
        Pam<BPS>::dist(z.x, r0, r1, e);
        Pam<BPS>::dist(z.y, i0, i1, e);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            o0[2 * j] = hf * r0[j];
            o0[2 * j + 1] = hf * i0[j];
            o1[2 * j] = hf * r1[j];
            o1[2 * j + 1] = hf * i1[j];
        }
    };
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool wide = ((reinterpret_cast<uintptr_t>(a.sym) | reinterpret_cast<uintptr_t>(a.soft0) | reinterpret_cast<uintptr_t>(a.soft1)) & 15) == 0;
    const int64_t n_tiles = wide ? a.n / TILE : 0;
    float* st0 = stage[wave][0];
    float* st1 = stage[wave][1];
    for (int64_t tile = int64_t(blockIdx.x) * 4 + wave; tile < n_tiles; tile += int64_t(gridDim.x) * 4) {
        const float4 v = load_stream16(reinterpret_cast<const float*>(a.sym) + 4 * (tile * (TILE / 2) + lane));
        float p0[BPS], p1[BPS], q0[BPS], q1[BPS];
        metrics(cf{v.x, v.y}, p0, p1);                                                    // symbol 2*lane of the tile
        metrics(cf{v.z, v.w}, q0, q1);                                                    // symbol 2*lane + 1
        float4* w0 = reinterpret_cast<float4*>(st0 + lane * 2 * BPS);
        float4* w1 = reinterpret_cast<float4*>(st1 + lane * 2 * BPS);
        w0[0] = float4{p0[0], p0[1], p0[2], p0[3]};
        w0[1] = float4{p0[4], p0[5], q0[0], q0[1]};
        w0[2] = float4{q0[2], q0[3], q0[4], q0[5]};
        w1[0] = float4{p1[0], p1[1], p1[2], p1[3]};
        w1[1] = float4{p1[4], p1[5], q1[0], q1[1]};
        w1[2] = float4{q1[2], q1[3], q1[4], q1[5]};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                              // wave-local exchange: in order per wave
        const int64_t obase = tile * (TILE * BPS);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int piece = k * 64 + lane;
            if (a.soft0) store_stream16(a.soft0 + obase + 4 * piece, *reinterpret_cast<const float4*>(st0 + 4 * piece));
            if (a.soft1) store_stream16(a.soft1 + obase + 4 * piece, *reinterpret_cast<const float4*>(st1 + 4 * piece));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                              // reads done before the next tile overwrites
    }
    for (int64_t i = n_tiles * TILE + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += int64_t(gridDim.x) * blockDim.x) {
        float o0[BPS], o1[BPS];
        metrics(a.sym[i], o0, o1);
#pragma unroll
        for (int b = 0; b < BPS; ++b) {
            if (a.soft0) a.soft0[i * BPS + b] = o0[b];
            if (a.soft1) a.soft1[i * BPS + b] = o1[b];
        }
    }
}

// ---- segmented soft de-mapper (ofdm_demap_frames): the metrics above with one sigma per segment (one frame of the batch).
// Work item w = (segment w / n_slices, slice w % n_slices), workgroups loop over the items with the grid as stride.  Nothing is
// added atomically: pass 1 writes one double per item, pass 2 adds a segment's partials in a fixed order, so a segment's outputs
// are the same bits alone, in any batch and on every call (block_sum of soft_device.hpp).

// Pass 1: a thread takes groups of FOUR consecutive symbols (two 16 B non-temporal loads where the slice is 16-byte aligned,
// else four 8 B loads) and adds their distances to its running double sum ONE BY ONE, in the same order on both paths: the
// partial does not depend on the alignment of the segment.
template <int MOD>
__global__ void __launch_bounds__(256) demap_seg_dmin_kernel(SegDemapArgs a) {
    __shared__ double sh[4];
    const int64_t n_items = a.n_seg * a.n_slices;
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int64_t s = w / a.n_slices, first = (w - s * a.n_slices) * SEG_SLICE;
        const int len = int(min(int64_t(SEG_SLICE), a.seg_len - first));
        const cf* p = a.sym + s * a.seg_stride + first;
        const bool wide = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < SEG_SLICE / 1024; ++k) {
            const int i0 = 4 * (k * 256 + int(threadIdx.x));
            if (i0 >= len) break;
            cf z[4];
            if (wide && i0 + 4 <= len) {
                const float4 v0 = load_stream16(reinterpret_cast<const float*>(p + i0)),
                             v1 = load_stream16(reinterpret_cast<const float*>(p + i0) + 4);
                z[0] = cf{v0.x, v0.y};
                z[1] = cf{v0.z, v0.w};
                z[2] = cf{v1.x, v1.y};
                z[3] = cf{v1.z, v1.w};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = i0 + e < len ? p[i0 + e] : cf{0.f, 0.f};
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < len) acc += double(demap_dmin<MOD>(z[e]));
        }
        const double tot = block_sum(acc, sh);
        if (threadIdx.x == 0) a.partial[w] = tot;
        __syncthreads();
    }
}

// per-symbol metrics of the segmented pass 2: llrp0 / llrp1 exactly as demap_soft_kernel (QPSK) / demap_soft_qam_kernel
// (no products here are contracted, so that llr = llrp0 - llrp1 is the difference of the two stored values)
template <int MOD>
__device__ __forceinline__ void seg_metrics(cf z, float hf, float (&o0)[MOD], float (&o1)[MOD]) {
#pragma clang fp contract(off)
    if constexpr (MOD == 2) {
        constexpr float K = 1.414213562373095f;
        bool rp, ip;
        cf e;
        qpsk_nearest(z, rp, ip, e);
        const float nr = hf * fabsf(e.x), fr = hf * (K - fabsf(e.x));
        const float ni = hf * fabsf(e.y), fi = hf * (K - fabsf(e.y));
        o0[0] = rp ? nr : fr;
        o0[1] = ip ? ni : fi;
        o1[0] = rp ? fr : nr;
        o1[1] = ip ? fi : ni;
    } else {
        constexpr int NB = Pam<MOD>::NB;
        float r0[NB], r1[NB], i0[NB], i1[NB], e;
        Pam<MOD>::dist(z.x, r0, r1, e);
        Pam<MOD>::dist(z.y, i0, i1, e);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            o0[2 * j] = hf * r0[j];
            o0[2 * j + 1] = hf * i0[j];
            o1[2 * j] = hf * r1[j];
            o1[2 * j + 1] = hf * i1[j];
        }
    }
}

// Pass 2: sigma of the item's segment from its partials (each lane adds partials lane, lane+256, ... in order, then
// block_sum), hf = -0.5/sigma^2 as ofdm_demap, then the slice's requested arrays (OUTS = SEG_OUT_* bits; OUTS == 0: sigma
// only, one item per segment).  llr = llrp0 - llrp1 of the two rounded values: the pragma keeps the compiler from contracting
// hf*d0 - hf*d1 into an fma.  QPSK: two symbols per lane (16 B load, 16 B store per array); 16-QAM: one symbol per lane (8 B
// load, 16 B store per array); 64-QAM: a wave's tile of 128 symbols through LDS as demap_soft_qam64_kernel, one array after
// the other, so every store instruction writes 1 KB contiguous.  Slices that are not 16-byte aligned in the input or in a
// requested output, and the symbols past the last full pair / tile, take per-float stores of the same values.
template <int MOD, int OUTS>
__global__ void __launch_bounds__(256) demap_seg_soft_kernel(SegDemapArgs a) {
#pragma clang fp contract(off)
    constexpr int TILE = 128;
    constexpr bool S0 = (OUTS & SEG_OUT_SOFT0) != 0, S1 = (OUTS & SEG_OUT_SOFT1) != 0, LL = (OUTS & SEG_OUT_LLR) != 0;
    __shared__ double sh[4];
    __shared__ __attribute__((aligned(16))) float stage[MOD == 6 ? 4 : 1][MOD == 6 ? TILE * MOD : 4];
    const int64_t per_seg = OUTS ? a.n_slices : 1;
    const int64_t n_items = a.n_seg * per_seg;
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const int64_t s = w / per_seg, sl = w - s * per_seg;
        const double* part = a.partial + s * a.n_slices;
        double acc = 0.0;
        for (int64_t i = threadIdx.x; i < a.n_slices; i += 256) acc += part[i];
        const double sigma = 0.7071067811865476 * (block_sum(acc, sh) / double(a.seg_len));
        const float hf = float(-0.5 / (sigma * sigma));
        if (sl == 0 && threadIdx.x == 0 && a.sigma) a.sigma[s] = sigma;
        if constexpr (OUTS != 0) {
            const int64_t first = sl * SEG_SLICE;
            const int len = int(min(int64_t(SEG_SLICE), a.seg_len - first));
            const cf* p = a.sym + s * a.seg_stride + first;
            const int64_t obase = (s * a.seg_len + first) * MOD;                        // float index of the slice's outputs
            float* q0 = S0 ? a.soft0 + obase : nullptr;
            float* q1 = S1 ? a.soft1 + obase : nullptr;
            float* ql = LL ? a.llr + obase : nullptr;
            const bool wide = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q0) | reinterpret_cast<uintptr_t>(q1) |
                                reinterpret_cast<uintptr_t>(ql)) & 15) == 0;
            auto put1 = [&](int i, const float (&o0)[MOD], const float (&o1)[MOD]) {                  // symbol i, per float
#pragma unroll
                for (int b = 0; b < MOD; ++b) {
                    if constexpr (S0) q0[int64_t(i) * MOD + b] = o0[b];
                    if constexpr (S1) q1[int64_t(i) * MOD + b] = o1[b];
                    if constexpr (LL) ql[int64_t(i) * MOD + b] = o0[b] - o1[b];
                }
            };
            int done = 0;                                                                 // symbols handled by the wide path
            if constexpr (MOD == 2) {
                if (wide) {
                    done = len & ~1;
                    for (int g = threadIdx.x; 2 * g < done; g += 256) {
                        const float4 v = load_stream16(reinterpret_cast<const float*>(p + 2 * g));
                        float a0[2], a1[2], b0[2], b1[2];
                        seg_metrics<2>(cf{v.x, v.y}, hf, a0, a1);
                        seg_metrics<2>(cf{v.z, v.w}, hf, b0, b1);
                        if constexpr (S0) store_stream16(q0 + 4 * g, float4{a0[0], a0[1], b0[0], b0[1]});
                        if constexpr (S1) store_stream16(q1 + 4 * g, float4{a1[0], a1[1], b1[0], b1[1]});
                        if constexpr (LL) store_stream16(ql + 4 * g, float4{a0[0] - a1[0], a0[1] - a1[1], b0[0] - b1[0], b0[1] - b1[1]});
                    }
                }
            } else if constexpr (MOD == 4) {
                if (wide) {
                    done = len;
                    for (int i = threadIdx.x; i < len; i += 256) {
                        const float2 v = load_stream8(reinterpret_cast<const float*>(p + i));
                        float o0[4], o1[4];
                        seg_metrics<4>(cf{v.x, v.y}, hf, o0, o1);
                        if constexpr (S0) store_stream16(q0 + 4 * i, float4{o0[0], o0[1], o0[2], o0[3]});
                        if constexpr (S1) store_stream16(q1 + 4 * i, float4{o1[0], o1[1], o1[2], o1[3]});
                        if constexpr (LL) store_stream16(ql + 4 * i, float4{o0[0] - o1[0], o0[1] - o1[1], o0[2] - o1[2], o0[3] - o1[3]});
                    }
                }
            } else {
                if (wide) {
                    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
                    const int n_tiles = len / TILE;
                    done = n_tiles * TILE;
                    float* st = stage[wave];
                    for (int t = wave; t < n_tiles; t += 4) {
                        const float4 v = load_stream16(reinterpret_cast<const float*>(p + t * TILE + 2 * lane));
                        float p0[6], p1[6], r0[6], r1[6];
                        seg_metrics<6>(cf{v.x, v.y}, hf, p0, p1);                             // symbol 2*lane of the tile
                        seg_metrics<6>(cf{v.z, v.w}, hf, r0, r1);                             // symbol 2*lane + 1
                        // one array at a time through the wave's 3 KB: 12 floats per lane in, 3 x 16 B per lane out
                        if constexpr (S0) store_tile64(q0, t, lane, st, p0, r0);
                        if constexpr (S1) store_tile64(q1, t, lane, st, p1, r1);
                        if constexpr (LL) {
                            float dp[6], dr[6];
#pragma unroll
                            for (int b = 0; b < 6; ++b) {
                                dp[b] = p0[b] - p1[b];
                                dr[b] = r0[b] - r1[b];
                            }
                            store_tile64(ql, t, lane, st, dp, dr);
                        }
                    }
                }
            }
            for (int i = done + int(threadIdx.x); i < len; i += 256) {
                float o0[MOD], o1[MOD];
                seg_metrics<MOD>(p[i], hf, o0, o1);
                put1(i, o0, o1);
            }
        }
        __syncthreads();                                                                  // sh is reused by the next item
    }
}

// Grid caps of the two passes.  These kernels loop with the grid as stride; with the 4 096 workgroups (16 per CU) of rounds 1-2 they
// read 0.60-0.68 of the HBM rate, with up to 262 144 (the loop then runs once or twice) 0.68-0.82: the dispatcher keeps more loads in
// flight across many short workgroups than 16 long ones per CU do (profiles/r03_demap_grid_ab.txt).
#ifndef OFDM_DEMAP_CAP1
#define OFDM_DEMAP_CAP1 262144
#endif
#ifndef OFDM_DEMAP_CAP2
#define OFDM_DEMAP_CAP2 262144
#endif
hipError_t launch_demap(const DemapArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const bool soft = a.soft0 || a.soft1;
    if (soft && a.mod != 2 && a.mod != 4 && a.mod != 6) return hipErrorInvalidValue;
    if (a.mod != 1 && a.mod != 2 && a.mod != 4 && a.mod != 6) return hipErrorInvalidValue;
    if (soft) {
        hipError_t e = hipMemsetAsync(a.partial, 0, DEMAP_PARTIALS * sizeof(double), s);
        if (e != hipSuccess) return e;
    }
    // pass 1 (one read of the symbols): hard bits and / or the distance sums sigma needs
    if (a.hard || soft) {
        const unsigned g1 = unsigned(std::min<int64_t>((a.n / 4 + 255) / 256 + 1, OFDM_DEMAP_CAP1));
#define OFDM_P1(M)                                                                                             \
    do {                                                                                                       \
        if (a.hard && soft)                                                                                    \
            hipLaunchKernelGGL((demap_pass1_kernel<M, true, (M != 1)>), dim3(g1), dim3(256), 0, s, a);         \
        else if (a.hard)                                                                                       \
            hipLaunchKernelGGL((demap_pass1_kernel<M, true, false>), dim3(g1), dim3(256), 0, s, a);            \
        else                                                                                                   \
            hipLaunchKernelGGL((demap_pass1_kernel<M, false, (M != 1)>), dim3(g1), dim3(256), 0, s, a);        \
    } while (0)
        switch (a.mod) {
            case 1: OFDM_P1(1); break;
            case 2: OFDM_P1(2); break;
            case 4: OFDM_P1(4); break;
            default: OFDM_P1(6); break;
        }
#undef OFDM_P1
    }
    // pass 2 (second read): the two metric arrays
    if (soft) {
        const unsigned grid = unsigned(std::min<int64_t>((a.n + 255) / 256, OFDM_DEMAP_CAP2));
        if (a.mod == 2)
            hipLaunchKernelGGL(demap_soft_kernel, dim3(grid), dim3(256), 0, s, a);
        else if (a.mod == 4)
            hipLaunchKernelGGL(demap_soft_qam_kernel<4>, dim3(grid), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(demap_soft_qam64_kernel, dim3(unsigned(std::min<int64_t>(a.n / 512 + 1, OFDM_DEMAP_CAP2))), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

// Two launches, no memset: pass 1 writes every partial it covers.  The caller has checked the arguments and sized a.partial.
template <int MOD>
static void launch_demap_frames_mod(const SegDemapArgs& a, int outs, hipStream_t s) {
    const int64_t items = a.n_seg * a.n_slices;
    hipLaunchKernelGGL(demap_seg_dmin_kernel<MOD>, dim3(unsigned(std::min<int64_t>(items, OFDM_DEMAP_CAP1))), dim3(256), 0, s, a);
    const unsigned g2 = unsigned(std::min<int64_t>(outs ? items : a.n_seg, OFDM_DEMAP_CAP2));
    switch (outs) {
#define OFDM_SEG(O) \
    case O: hipLaunchKernelGGL((demap_seg_soft_kernel<MOD, O>), dim3(g2), dim3(256), 0, s, a); break;
        OFDM_SEG(0) OFDM_SEG(1) OFDM_SEG(2) OFDM_SEG(3) OFDM_SEG(4) OFDM_SEG(5) OFDM_SEG(6) OFDM_SEG(7)
#undef OFDM_SEG
    }
}
hipError_t launch_demap_frames(const SegDemapArgs& a, hipStream_t s) {
    if (a.n_seg <= 0 || a.seg_len <= 0) return hipSuccess;
    const int outs = (a.soft0 ? SEG_OUT_SOFT0 : 0) | (a.soft1 ? SEG_OUT_SOFT1 : 0) | (a.llr ? SEG_OUT_LLR : 0);
    if (!outs && !a.sigma) return hipSuccess;
    switch (a.mod) {
        case 2: launch_demap_frames_mod<2>(a, outs, s); break;
        case 4: launch_demap_frames_mod<4>(a, outs, s); break;
        case 6: launch_demap_frames_mod<6>(a, outs, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ofdm
