// rx_chanavg.hip -- the channel estimate averaged over every sync symbol of a frame (gfx950): chan_avg_kernel,
// chan_avg_finalize_kernel and their launch.
// Contract: include/ofdm_mi355x.h, "channel estimate averaged over every sync symbol of a frame"; tests/chanavg_ref.py restates it
// in fp64 NumPy.
//
// A unit of its own on purpose, as rx_chanwin.hip: the kernels of every other unit keep their module and with it their code.
#include <type_traits>

#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

// Sums of three values over the T lanes of one symbol in ONE round: the lane sums of symbol_sum, then (T > 64) three LDS
// partials per wave behind one barrier, added in wave order.  `red` = the slot's reduction scratch (24 floats, 12 used).
template <int T>
__device__ __forceinline__ void symbol_sum3(float& x, float& y, float& z, float* red, int t) {
    x = lanes_sum<T>(x);
    y = lanes_sum<T>(y);
    z = lanes_sum<T>(z);
    if constexpr (T > 64) {
        constexpr int NW = T / 64;
        if ((t & 63) == 0) {
            red[3 * (t >> 6) + 0] = x;
            red[3 * (t >> 6) + 1] = y;
            red[3 * (t >> 6) + 2] = z;
        }
        wg_barrier();
        x = y = z = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            x += red[3 * w + 0];
            y += red[3 * w + 1];
            z += red[3 * w + 2];
        }
    }
}

__device__ __forceinline__ bool finite_pos(float v) { return v > 0.f && v < __builtin_inff(); }   // false for a NaN

// LDS of chan_avg_kernel<N>: the FFT's carve, then (B0_LDS) N entries per slot for b_0
template <int N>
struct ChanAvgLds {
    static constexpr bool B0_LDS = N <= 2048;
    static constexpr size_t BYTES = WgLds<N>::BYTES + (B0_LDS ? size_t(Plan<N>::SLOTS) * N * sizeof(cf) : 0);
};

}  // namespace

// One work item = (frame, chunk of CHANAVG_CHUNK consecutive patterns) per FFT slot, Plan<N>::SLOTS items per workgroup.
//
// The sums run on the RAW sync-bin values: with g[k] = e^{+j 2pi d k/N} conj(zc[k]) (|g| = 1) the contract's a_p[k] is
// g[k] b_p[k], b_p = sqrt(Ks/E_p)/(1 + 1/snr_ls) y_p, so
//     c_p = sum_k a_p conj(a_0) = sum_k b_p conj(b_0)        d_p = g (conj(u_p) b_p - b_0)        |d_p|^2 = |conj(u_p) b_p - b_0|^2
// and g is applied once per chunk, to the sum, where the partial is stored -- not once per pattern.  Held in registers across
// the pattern loop: the sum, the window in flight and the window being transformed (3 x P complex); b_0 sits in the slot's LDS
// (registers at 4096-pt, see ChanAvgLds).  With all four in registers hipcc needed more than 256 VGPRs at every size from
// 128-pt on (one wave per SIMD); the second launch bound holds the kernel to two.
//
// Per item: b_0 from the window of pattern 0 (every chunk of a frame runs the same arithmetic on the same samples, so it is the
// same bits in all of them), then the chunk's patterns in ascending p.  The loads of pattern p + 1 are issued BEFORE the FFT of
// pattern p and first used after it.  One reduction round per pattern carries E_p, Re c_p and Im c_p; c_p is formed with the
// unnormalised y_p (only its direction is used).
// A row without a sync, or whose pattern 0 does not take part, runs the arithmetic on zeros (the barriers are workgroup-wide) and
// leaves count 0, sum-of-squares +0 and rot +0.
template <int N>
__global__ void __launch_bounds__(Plan<N>::WG, 2) chan_avg_kernel(RxDev rx, ChanAvgArgs a) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P, CH = CHANAVG_CHUNK;
    constexpr bool B0_LDS = ChanAvgLds<N>::B0_LDS;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = (T >= 64) ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;
    const int t = tid % T;
    cf* smem = reinterpret_cast<cf*>(smem_raw);
    cf* lds = smem + slot * WgLds<N>::STRIDE;
    float* red = reinterpret_cast<float*>(lds + WgLds<N>::ELEMS);
    const cf* w1tab = wg_init_w1<N>(smem, rx.tw, tid);
    std::conditional_t<PL::R0 == 16, CompactTwiddles<N>, LaneTwiddles<N>> tw;
    load_twiddles(tw, rx.tw, t);

    const int64_t n_items = a.n_frames * a.n_chunks;
    const int64_t item = int64_t(blockIdx.x) * PL::SLOTS + slot;
    const bool in_range = item < n_items;
    const int64_t frame = in_range ? item / a.n_chunks : 0;
    const int chunk = in_range ? int(item - frame * a.n_chunks) : 0;
    const bool active = in_range && a.tsr[frame * 4 + 3] == 1;
    const int64_t t0 = active ? int64_t(a.tsr[frame * 4 + 0]) : 0;
    const int lag = active ? a.tsr[frame * 4 + 1] : 0;
    const int64_t step = int64_t(rx.L) * (rx.S + rx.D);
    const cf* fiq = a.iq + frame * a.frame_stride;
    const int Ks = rx.Ks;
    // pattern 0 is every chunk's reference and chunk 0's first member: u_0 = 1 and d_0 = 0 by definition, so the loop starts behind it
    const int p_begin = chunk * CH + (chunk == 0 ? 1 : 0);
    const int p_end = min(a.n_pat, chunk * CH + CH);
    // trips of the pattern loop, the same for every lane of the workgroup (the FFT's barriers are workgroup-wide): the item's own
    // where the workgroup has one item, else those of the longest chunk of a frame
    const int n_it = PL::SLOTS == 1 ? max(p_end - p_begin, 0) : (a.n_chunks == 1 ? a.n_pat - 1 : CH);

    // which of this lane's register slots hold a sync bin (bit s), and which one holds the bin listed twice (Ks == N: bin N/2)
    unsigned used = 0, dup = 0;
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int k = (t + T * j) + PL::NC * kl;
            int in_, ip_;
            if (bin_neg(k, Ks, N, in_) || bin_pos(k, Ks, ip_)) used |= 1u << out_slot<N>(j, kl);
            if (Ks == N && k == N / 2) dup |= 1u << out_slot<N>(j, kl);
        }
    }

    // window of pattern p: a candidate iff it lies inside the frame (never zero-padded); 8 B per lane, coalesced, read once
    auto load_win = [&](cf (&buf)[P], int p, bool on) {
        const int64_t w = t0 + step * p;
        const bool cand = on && w >= 0 && w + N <= a.frame_len;
        if (cand) {
            const cf* src = fiq + w + t;
#pragma unroll
            for (int n0 = 0; n0 < P; ++n0) buf[n0] = __builtin_nontemporal_load(src + T * n0);
        } else {
#pragma unroll
            for (int n0 = 0; n0 < P; ++n0) buf[n0] = cf{0.f, 0.f};
        }
        return cand;
    };

    cf v[P], nxt[P];
    const bool cand0 = load_win(v, 0, active);
    bool cand_nxt = load_win(nxt, p_begin, active && p_begin < p_end);
    wg_fft<N>(v, lds, tw, w1tab, t);
    if constexpr (T <= 64) wg_barrier();                   // every lane is through the last pass before the region is rewritten
    float e0 = 0.f;
#pragma unroll
    for (int s = 0; s < P; ++s) {
        const float m2 = cnorm2(v[s]);
        e0 += ((used >> s) & 1u) ? m2 : 0.f;
        e0 += ((dup >> s) & 1u) ? m2 : 0.f;
    }
    e0 = symbol_sum<T>(e0, red, t);
    const bool row_on = cand0 && finite_pos(e0);
    const float sc0 = row_on ? sqrtf(float(Ks) / e0) * rx.inv_ls : 0.f;
    // b_0: entry s of lane t at [s*T + t] of the slot's own LDS region behind the pass-1 table (a lane reads back what it wrote:
    // no barrier, no bank conflict), or -- 4096-pt, whose exchange region leaves no room for it below 64 KB -- in registers
    cf b0r[B0_LDS ? 1 : P], sum[P];
    cf* b0l = smem + WgLds<N>::STRIDE * PL::SLOTS + WgLds<N>::W1_ELEMS + slot * N + t;
    auto b0 = [&](int s) -> cf {
        if constexpr (B0_LDS)
            return b0l[s * T];
        else
            return b0r[s];
    };
#pragma unroll
    for (int s = 0; s < P; ++s) {
        const cf b = (row_on && ((used >> s) & 1u)) ? cscale(v[s], sc0) : cf{0.f, 0.f};
        if constexpr (B0_LDS)
            b0l[s * T] = b;
        else
            b0r[s] = b;
        sum[s] = cf{0.f, 0.f};
    }
    float q = 0.f;
    int cnt = (chunk == 0 && row_on) ? 1 : 0;
    if (in_range && t == 0 && a.rot && chunk == 0 && a.n_pat > 0)
        a.rot[frame * a.n_pat] = row_on ? cf{1.f, 0.f} : cf{0.f, 0.f};

#pragma unroll 1
    for (int it = 0; it < n_it; ++it) {
        const int p = p_begin + it;
        // opaque per pattern: the sixteen slot predicates are formed where they are used, not held in SGPR pairs across the loop
        unsigned um = used, dm = dup;
        asm volatile("" : "+v"(um), "+v"(dm));
        const bool cand = cand_nxt;
#pragma unroll
        for (int n0 = 0; n0 < P; ++n0) v[n0] = nxt[n0];
        cand_nxt = load_win(nxt, p + 1, active && it + 1 < n_it && p + 1 < p_end);     // in flight during the FFT below
        wg_fft<N>(v, lds, tw, w1tab, t);
        if constexpr (T <= 64) wg_barrier();
        float e = 0.f, cre = 0.f, cim = 0.f;
#pragma unroll
        for (int s = 0; s < P; ++s) {
            const float m2 = cnorm2(v[s]);
            e += ((um >> s) & 1u) ? m2 : 0.f;
            e += ((dm >> s) & 1u) ? m2 : 0.f;
            const cf c = cmulc(v[s], b0(s));               // b_0 is zero outside the sync bins
            cre += c.x;
            cim += c.y;
        }
        symbol_sum3<T>(e, cre, cim, red, t);
        const float cabs = sqrtf(cre * cre + cim * cim);
        const bool takes = cand && row_on && finite_pos(e) && finite_pos(cabs);
        const cf u = takes ? cf{cre / cabs, cim / cabs} : cf{0.f, 0.f};
        const float sc = takes ? sqrtf(float(Ks) / e) * rx.inv_ls : 0.f;
        if (takes) {
#pragma unroll
            for (int s = 0; s < P; ++s) {
                const cf d = ((um >> s) & 1u) ? cmulc(cscale(v[s], sc), u) - b0(s) : cf{0.f, 0.f};
                sum[s] = sum[s] + d;
                q += cnorm2(d);
            }
            cnt += 1;
        }
        if (in_range && t == 0 && a.rot && p < p_end) a.rot[frame * a.n_pat + p] = u;
    }
    if constexpr (T > 64) wg_barrier();                    // the last round's partials are read before the scratch is rewritten
    q = symbol_sum<T>(q, red, t);

    if (!in_range) return;
    if (t == 0) {
        a.part_q[item] = row_on ? q : 0.f;
        a.part_n[item] = cnt;
    }
    if (!row_on) return;
    // g = e^{+j 2pi d k/N} conj(zc[k]) on the sum (and, from chunk 0, on b_0): consecutive lanes store consecutive bins.  The
    // lag's index is an unsigned product, so a negative lag wraps (chan_window_kernel).
    const cf* zp = rx.zcp + t;
    cf* pd = a.part_d + item * N;
    cf* pa = a.part_a0 + frame * N;
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int k = (t + T * j) + PL::NC * kl;
            const int s = out_slot<N>(j, kl);
            if ((used >> s) & 1u) {
                const cf rot = cconj(rx.tw[(unsigned(lag) * unsigned(k)) & unsigned(N - 1)]);
                const cf g = cmul(cconj(zp[s * T]), rot);
                pd[k] = cmul(g, sum[s]);
                if (chunk == 0) pa[k] = cmul(g, b0(s));
            }
        }
    }
}

// One frame per workgroup of 256 lanes, lane i at bins i, i + 256, ...: a frame's chunk partials added in chunk order from +0,
// the mean on the sync bins, the gains of sync_finalize from it, the spread.  The sum over bins of |sum_p d_p|^2 has a fixed
// order: a lane's bins ascending, the 64 lanes through wave_sum, the four waves in wave order.
__global__ void __launch_bounds__(256) chan_avg_finalize_kernel(RxDev rx, ChanAvgArgs a) {
    __shared__ float red[4];
    const int64_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = rx.nfft, Ks = rx.Ks, Kd = rx.Kd, nch = a.n_chunks;
    const bool active = a.tsr[f * 4 + 3] == 1;
    const int lag = a.tsr[f * 4 + 1];
    const float* pq = a.part_q + f * nch;
    const int* pn = a.part_n + f * nch;
    const bool on = active && nch > 0 && pn[0] > 0;        // pattern 0 takes part: chunk 0 counted it
    int n = 0;
    float Q = 0.f;
    if (on) {
        for (int c = 0; c < nch; ++c) {
            n += pn[c];
            Q += pq[c];
        }
    }
    const float fn = float(n > 0 ? n : 1);
    float acc = 0.f;
    for (int k = tid; k < N; k += 256) {
        int in_, ip_;
        const bool sync_bin = bin_neg(k, Ks, N, in_) || bin_pos(k, Ks, ip_);
        cf D = cf{0.f, 0.f};
        if (on && sync_bin)
            for (int c = 0; c < nch; ++c) D = D + a.part_d[(f * nch + c) * N + k];
        acc += cnorm2(D);
        if (!on) continue;
        const cf Hk = sync_bin ? a.part_a0[f * N + k] + cf{D.x / fn, D.y / fn} : cf{0.f, 0.f};
        if (a.H_out) a.H_out[f * N + k] = Hk;
        if (a.gain) {
            const cf rot = cconj(rx.tw[(unsigned(lag) * unsigned(k)) & unsigned(N - 1)]);
            const cf gk = cmul(cscale(cconj(Hk), 1.f / (cnorm2(Hk) + rx.inv_snr_data)), rot);
            int id_;
            if (bin_neg(k, Kd, N, id_)) a.gain[f * Kd + id_] = gk;
            if (bin_pos(k, Kd, id_)) a.gain[f * Kd + id_] = gk;
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        const float s2 = ((red[0] + red[1]) + red[2]) + red[3];
        if (a.spread) a.spread[f] = (on && n >= 2) ? (Q - s2 / fn) / (float(n - 1) * float(Ks)) : 0.f;
        if (a.n_used) a.n_used[f] = on ? n : 0;
    }
}

// sigma2[f] = double(spread[f]): the layout OFDM_MRC_NOISE_SEG takes
__global__ void __launch_bounds__(256) chan_spread_kernel(const float* spread, int64_t n, double* sigma2) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) sigma2[i] = double(spread[i]);
}

template <int N>
static hipError_t launch_chan_avg_n(const RxDev& rx, const ChanAvgArgs& a, hipStream_t s) {
    const int64_t n_items = a.n_frames * a.n_chunks;
    const unsigned grid = unsigned((n_items + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    hipLaunchKernelGGL(chan_avg_kernel<N>, dim3(grid), dim3(Plan<N>::WG), ChanAvgLds<N>::BYTES, s, rx, a);
    return hipGetLastError();
}

hipError_t launch_chan_average(const RxDev& rx, const ChanAvgArgs& a, hipStream_t s) {
    if (a.n_frames <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.n_chunks > 0) {
        switch (rx.nfft) {
            case 64: e = launch_chan_avg_n<64>(rx, a, s); break;
            case 128: e = launch_chan_avg_n<128>(rx, a, s); break;
            case 256: e = launch_chan_avg_n<256>(rx, a, s); break;
            case 512: e = launch_chan_avg_n<512>(rx, a, s); break;
            case 1024: e = launch_chan_avg_n<1024>(rx, a, s); break;
            case 2048: e = launch_chan_avg_n<2048>(rx, a, s); break;
            case 4096: e = launch_chan_avg_n<4096>(rx, a, s); break;
            default: return hipErrorInvalidValue;
        }
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(chan_avg_finalize_kernel, dim3(unsigned(a.n_frames)), dim3(256), 0, s, rx, a);
    return hipGetLastError();
}

hipError_t launch_chan_spread(const float* spread, int64_t n, double* sigma2, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(chan_spread_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, spread, n, sigma2);
    return hipGetLastError();
}

hipError_t chan_average_prepare() {
    return load_kernels(chan_spread_kernel, chan_avg_finalize_kernel, chan_avg_kernel<64>, chan_avg_kernel<128>, chan_avg_kernel<256>,
                        chan_avg_kernel<512>, chan_avg_kernel<1024>, chan_avg_kernel<2048>, chan_avg_kernel<4096>);
}

}  // namespace ofdm
