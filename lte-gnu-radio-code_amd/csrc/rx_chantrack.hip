// rx_chantrack.hip -- the channel tracked across the sync symbols of a frame (gfx950): chan_track_est_kernel,
// chan_track_link_kernel, rx_demod_track_kernel, the hard-decision pass and their launches.
// Contract: include/ofdm_mi355x.h, "channel tracked across the sync symbols of a frame"; tests/chantrack_ref.py restates it in
// fp64 NumPy.
//
// A unit of its own on purpose, as rx_chanavg.hip: the kernels of every other unit keep their module and with it their code.
#include <type_traits>

#include "demap_hard.hpp"
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

__device__ __forceinline__ bool finite_pos(float v) { return v > 0.f && v < __builtin_inff(); }   // false for a NaN

// which of lane t's FFT output registers hold a bin of binsP(K) (bit s of `used`), and which one holds the bin listed twice
// (K == N: bin N/2)
template <int N>
__device__ __forceinline__ void bin_masks(int t, int K, unsigned& used, unsigned& dup) {
    using PL = Plan<N>;
    used = dup = 0;
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int k = (t + PL::T * j) + PL::NC * kl;
            int in_, ip_;
            if (bin_neg(k, K, N, in_) || bin_pos(k, K, ip_)) used |= 1u << out_slot<N>(j, kl);
            if (K == N && k == N / 2) dup |= 1u << out_slot<N>(j, kl);
        }
    }
}

// sum of |v[s]|^2 over the list: the slots of `used`, the doubled bin once more
template <int P>
__device__ __forceinline__ float list_power(const cf (&v)[P], unsigned used, unsigned dup) {
    float e = 0.f;
#pragma unroll
    for (int s = 0; s < P; ++s) {
        const float m2 = cnorm2(v[s]);
        e += ((used >> s) & 1u) ? m2 : 0.f;
        e += ((dup >> s) & 1u) ? m2 : 0.f;
    }
    return e;
}

}  // namespace

// One work item = (frame, pattern) per FFT slot, Plan<N>::SLOTS items per workgroup: chan_avg_kernel without the sums.  The
// window of the pattern's sync symbol (8 B per lane, coalesced, read once), the FFT, E_p in one reduction round, then the row
// a_p = sqrt(Ks/E_p)/(1 + 1/snr_ls) y_p g with g[k] = e^{+j 2pi d k/N} conj(zc[k]) on the sync bins and +0 on every other bin,
// consecutive lanes on consecutive bins.  A pattern that does not take part (no candidate, E_p not finite and positive, a frame
// without a sync) runs the arithmetic on zeros, writes a row of +0 and the flag 0.
template <int N>
__global__ void __launch_bounds__(Plan<N>::WG) chan_track_est_kernel(RxDev rx, ChanTrackArgs a) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
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

    const int64_t n_items = a.n_frames * a.n_pat;
    const int64_t item = int64_t(blockIdx.x) * PL::SLOTS + slot;
    const bool in_range = item < n_items;
    const int64_t frame = in_range ? item / a.n_pat : 0;
    const int p = in_range ? int(item - frame * a.n_pat) : 0;
    const bool active = in_range && a.tsr[frame * 4 + 3] == 1;
    const int64_t t0 = active ? int64_t(a.tsr[frame * 4 + 0]) : 0;
    const int lag = active ? a.tsr[frame * 4 + 1] : 0;
    const int Ks = rx.Ks;
    unsigned used, dup;
    bin_masks<N>(t, Ks, used, dup);

    // a candidate iff the window lies inside the frame (never zero-padded)
    const int64_t w = t0 + int64_t(rx.L) * (rx.S + rx.D) * p;
    const bool cand = active && w >= 0 && w + N <= a.frame_len;
    cf v[P];
    if (cand) {
        const cf* src = a.iq + frame * a.frame_stride + w + t;
#pragma unroll
        for (int n0 = 0; n0 < P; ++n0) v[n0] = __builtin_nontemporal_load(src + T * n0);
    } else {
#pragma unroll
        for (int n0 = 0; n0 < P; ++n0) v[n0] = cf{0.f, 0.f};
    }
    wg_fft<N>(v, lds, tw, w1tab, t);
    const float e = symbol_sum<T>(list_power<P>(v, used, dup), red, t);
    const bool takes = cand && finite_pos(e);
    const float sc = takes ? sqrtf(float(Ks) / e) * rx.inv_ls : 0.f;

    if (!in_range) return;
    if (t == 0) a.flag[item] = takes ? 1 : 0;
    // the lag's index is an unsigned product, so a negative lag wraps (chan_window_kernel)
    const cf* zp = rx.zcp + t;
    cf* row = a.H_pat + item * N;
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int k = (t + T * j) + PL::NC * kl;
            const int s = out_slot<N>(j, kl);
            cf out = cf{0.f, 0.f};
            if (takes && ((used >> s) & 1u)) {
                const cf rot = cconj(rx.tw[(unsigned(lag) * unsigned(k)) & unsigned(N - 1)]);
                out = cmul(cmul(cconj(zp[s * T]), rot), cscale(v[s], sc));
            }
            row[k] = out;
        }
    }
}

// One frame per workgroup of 256 lanes.  A frame without a sync, or whose pattern 0 does not take part, is a frame without a
// sync: its flags are cleared and the rows a later pattern wrote are set to +0.  Otherwise lane i takes the patterns i, i + 256,
// ...: lo = the nearest q <= p that takes part (pattern 0 does), hi = the nearest q > p that does, -1 without one or in hold
// mode.  The walks are as long as the gaps between the patterns that take part.
__global__ void __launch_bounds__(256) chan_track_link_kernel(RxDev rx, ChanTrackArgs a) {
    const int64_t f = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = rx.nfft, n_pat = a.n_pat;
    int* fl = a.flag + f * n_pat;
    const bool live = a.tsr[f * 4 + 3] == 1 && fl[0] == 1;
    const int lag = a.tsr[f * 4 + 1];
    if (!live) {
        for (int p = 1; p < n_pat; ++p) {
            if (fl[p] == 0) continue;                      // the same for every lane: nothing below writes a flag yet
            cf* row = a.H_pat + (f * n_pat + p) * N;
            for (int k = tid; k < N; k += 256) row[k] = cf{0.f, 0.f};
        }
    }
    __syncthreads();                                       // every lane has read the flags it needs before they are cleared
    for (int p = tid; p < n_pat; p += 256) {
        const int64_t r = f * n_pat + p;
        const int tk = live ? fl[p] : 0;
        int lo = 0, hi = -1;
        if (live) {
            lo = p;
            while (fl[lo] == 0) --lo;
            if (a.linear) {
                hi = p + 1;
                while (hi < n_pat && fl[hi] == 0) ++hi;
                if (hi == n_pat) hi = -1;
            }
        } else {
            fl[p] = 0;
        }
        a.nb[r] = int2{lo, hi};
        if (a.takes) a.takes[r] = tk;
        if (a.row_tsr) {
            int4 w;
            w.x = 0;
            w.y = lag;
            w.z = 0;
            w.w = tk;
            reinterpret_cast<int4*>(a.row_tsr)[r] = w;
        }
    }
}

// One work item = (frame, run of CHANTRACK_RUN consecutive data symbols) per FFT slot, Plan<N>::SLOTS items per workgroup; the
// trip count is the same for every lane of a workgroup (the FFT's barriers are workgroup-wide).  The loads of symbol q + 1 are
// issued BEFORE the FFT of symbol q and first used after it.  A symbol is equalised straight from the FFT's output registers:
// the power over the data-bin list through the slot masks, the two estimate rows a_lo and a_hi read in lane order (consecutive
// lanes on consecutive bins; a row is re-read by up to 2 D symbols and comes from L2), H = a_lo + w (a_hi - a_lo), the gain and
// z in registers, consecutive lanes on consecutive list entries of the output rows.
// A symbol of a frame without a sync, or of a pattern whose guard fails, gets a row of zeros.
template <int N>
__global__ void __launch_bounds__(Plan<N>::WG, 2) rx_demod_track_kernel(RxDev rx, ChanTrackArgs a) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P, RUN = CHANTRACK_RUN;
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

    const int64_t n_items = a.n_frames * a.n_runs;
    const int64_t item = int64_t(blockIdx.x) * PL::SLOTS + slot;
    const bool in_range = item < n_items;
    const int64_t frame = in_range ? item / a.n_runs : 0;
    const int run = in_range ? int(item - frame * a.n_runs) : 0;
    const bool alive = in_range && a.tsr[frame * 4 + 3] == 1 && a.flag[frame * a.n_pat] == 1;
    const int64_t t0 = alive ? int64_t(a.tsr[frame * 4 + 0]) : 0;
    const int lag = alive ? a.tsr[frame * 4 + 1] : 0;
    const int D = rx.D, SD = rx.S + rx.D, Kd = rx.Kd;
    const int64_t L = rx.L;
    const cf* fiq = a.iq + frame * a.frame_stride;
    const int q0 = run * RUN;
    const int q1 = in_range ? min(a.n_dsym, q0 + RUN) : q0;
    const int n_it = PL::SLOTS == 1 ? q1 - q0 : RUN;
    unsigned used, dup;
    bin_masks<N>(t, Kd, used, dup);

    // data symbol q of the frame: demodulated iff the frame is alive and ptr_p + N - 1 <= frame_len; the window is zero-padded
    // outside the frame, like fft(x, N)
    auto load_sym = [&](cf (&buf)[P], int q, bool on) {
        const int p = q / D, m = q - p * D;
        const int64_t ptr = t0 + L * (int64_t(p) * SD + 1);
        const bool dem = on && ptr + N - 1 <= a.frame_len;
        const int64_t start = ptr + L * m;
        if (dem && start >= 0 && start + N <= a.frame_len) {
            const cf* src = fiq + start + t;
#pragma unroll
            for (int n0 = 0; n0 < P; ++n0) buf[n0] = __builtin_nontemporal_load(src + T * n0);
        } else {
#pragma unroll
            for (int n0 = 0; n0 < P; ++n0) {
                const int64_t i = start + t + T * n0;
                buf[n0] = (dem && i >= 0 && i < a.frame_len) ? __builtin_nontemporal_load(fiq + i) : cf{0.f, 0.f};
            }
        }
        return dem;
    };

    cf v[P], nxt[P];
    bool dem_nxt = load_sym(nxt, q0, alive && q0 < q1);
#pragma unroll 1
    for (int it = 0; it < n_it; ++it) {
        const int q = q0 + it;
        // opaque per symbol: the slot predicates are formed where they are used, not held in SGPR pairs across the loop
        unsigned um = used, dm = dup;
        asm volatile("" : "+v"(um), "+v"(dm));
        const bool dem = dem_nxt;
#pragma unroll
        for (int n0 = 0; n0 < P; ++n0) v[n0] = nxt[n0];
        dem_nxt = load_sym(nxt, q + 1, alive && q + 1 < q1);     // in flight during the FFT below
        wg_fft<N>(v, lds, tw, w1tab, t);
        if constexpr (T <= 64) wg_barrier();               // every lane is through the last pass before the region is rewritten
        const float ps = symbol_sum<T>(list_power<P>(v, um, dm), red, t);
        if (q >= q1) continue;

        // opaque per symbol as well: what the output phase derives from the lane index and the lag (bin offsets, list positions,
        // de-rotation factors) is formed here, not held in registers across the FFT.  The lag's index is an unsigned product, so
        // a negative lag wraps (chan_window_kernel).
        int tt = t;
        unsigned lg = unsigned(lag);
        asm volatile("" : "+v"(tt), "+v"(lg));
        const cf rot_t = cconj(rx.tw[(lg * unsigned(tt)) & unsigned(N - 1)]);
        const int p = q / D, m = q - p * D;
        int2 nb = int2{0, -1};
        if (alive) nb = a.nb[frame * a.n_pat + p];
        const int lo = nb.x, hi = nb.y;
        const float w = hi >= 0 ? float(p * SD + 1 + m - lo * SD) / float((hi - lo) * SD) : 0.f;
        const cf* Hlo = a.H_pat + (frame * a.n_pat + lo) * N;
        const cf* Hhi = a.H_pat + (frame * a.n_pat + (hi >= 0 ? hi : lo)) * N;
        const float sc = sqrtf(float(Kd) / ps);
        const int64_t orow = frame * a.n_dsym + q;
        cf* eqr = a.eq ? a.eq + orow * Kd : nullptr;
        float* csr = a.csi ? a.csi + orow * Kd : nullptr;
#pragma unroll
        for (int j = 0; j < PL::C; ++j) {
#pragma unroll
            for (int kl = 0; kl < PL::RL; ++kl) {
                // the estimate rows are read four bins at a time: with all 2 P loads of a symbol hoisted to the top of this phase
                // hipcc needed more than 256 VGPRs and spilled
                if ((j * PL::RL + kl) % 4 == 0) asm volatile("" ::: "memory");
                const int k = (tt + T * j) + PL::NC * kl;
                const int s = out_slot<N>(j, kl);
                int in_, ip_;
                const bool neg = bin_neg(k, Kd, N, in_), pos = bin_pos(k, Kd, ip_);
                if (!(neg || pos)) continue;
                cf H = cf{0.f, 0.f};
                if (alive) {
                    H = Hlo[k];
                    if (hi >= 0) H = H + cscale(Hhi[k] - H, w);
                }
                if (eqr) {
                    cf z = cf{0.f, 0.f};
                    if (dem) {
                        // e^{+j 2pi d k/N} = the lane's factor times the register slot's, which is the same for every lane
                        const cf rot = cmul(rot_t, cconj(rx.tw[(lg * unsigned(T * j + PL::NC * kl)) & unsigned(N - 1)]));
                        const cf g = cscale(cconj(H), 1.f / (cnorm2(H) + rx.inv_snr_data));
                        z = cmul(cmul(cscale(v[s], sc), g), rot);
                    }
                    if (neg) eqr[in_] = z;
                    if (pos) eqr[ip_] = z;
                }
                if (csr) {
                    const float c = __fadd_rn(__fmul_rn(H.x, H.x), __fmul_rn(H.y, H.y));
                    if (neg) csr[in_] = c;
                    if (pos) csr[ip_] = c;
                }
            }
        }
    }
}

// Hard decisions of the stored rows by the rules of demap_hard.hpp: one lane per four consecutive symbols (packed: Kd % 4 == 0,
// so the four never straddle a byte)
template <int MOD, int BMODE>
__global__ void __launch_bounds__(256) chan_track_bits_kernel(const cf* eq, int64_t n_sym, uint8_t* bits) {
    const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 4;
    if (i >= n_sym) return;
    const int cnt = int(min(int64_t(4), n_sym - i));
    cf z[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = e < cnt ? eq[i + e] : cf{0.f, 0.f};
    store_bits<MOD, BMODE>(bits, i, z, cnt);
}

template <int N>
static hipError_t launch_est_n(const RxDev& rx, const ChanTrackArgs& a, hipStream_t s) {
    const int64_t n_items = a.n_frames * a.n_pat;
    const unsigned grid = unsigned((n_items + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    hipLaunchKernelGGL(chan_track_est_kernel<N>, dim3(grid), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, a);
    return hipGetLastError();
}

template <int N>
static hipError_t launch_demod_n(const RxDev& rx, const ChanTrackArgs& a, hipStream_t s) {
    const int64_t n_items = a.n_frames * a.n_runs;
    const unsigned grid = unsigned((n_items + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    hipLaunchKernelGGL(rx_demod_track_kernel<N>, dim3(grid), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, a);
    return hipGetLastError();
}

template <int MOD, int BMODE>
static hipError_t launch_bits_mb(const cf* eq, int64_t n_sym, uint8_t* bits, hipStream_t s) {
    const unsigned grid = unsigned(((n_sym + 3) / 4 + 255) / 256);
    hipLaunchKernelGGL((chan_track_bits_kernel<MOD, BMODE>), dim3(grid), dim3(256), 0, s, eq, n_sym, bits);
    return hipGetLastError();
}

hipError_t launch_chan_track_est(const RxDev& rx, const ChanTrackArgs& a, hipStream_t s) {
    if (a.n_frames <= 0 || a.n_pat <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    switch (rx.nfft) {
        case 64: e = launch_est_n<64>(rx, a, s); break;
        case 128: e = launch_est_n<128>(rx, a, s); break;
        case 256: e = launch_est_n<256>(rx, a, s); break;
        case 512: e = launch_est_n<512>(rx, a, s); break;
        case 1024: e = launch_est_n<1024>(rx, a, s); break;
        case 2048: e = launch_est_n<2048>(rx, a, s); break;
        case 4096: e = launch_est_n<4096>(rx, a, s); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(chan_track_link_kernel, dim3(unsigned(a.n_frames)), dim3(256), 0, s, rx, a);
    return hipGetLastError();
}

hipError_t launch_chan_track_demod(const RxDev& rx, const ChanTrackArgs& a, hipStream_t s) {
    if (a.n_frames <= 0 || a.n_dsym <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.eq || a.csi) {
        switch (rx.nfft) {
            case 64: e = launch_demod_n<64>(rx, a, s); break;
            case 128: e = launch_demod_n<128>(rx, a, s); break;
            case 256: e = launch_demod_n<256>(rx, a, s); break;
            case 512: e = launch_demod_n<512>(rx, a, s); break;
            case 1024: e = launch_demod_n<1024>(rx, a, s); break;
            case 2048: e = launch_demod_n<2048>(rx, a, s); break;
            case 4096: e = launch_demod_n<4096>(rx, a, s); break;
            default: return hipErrorInvalidValue;
        }
    }
    if (e != hipSuccess || !a.bits) return e;
    const int64_t n_sym = a.n_frames * a.n_dsym * rx.Kd;
    const bool packed = a.bits_mode == 1;
    switch (a.mod) {
        case 1: return packed ? hipErrorInvalidValue : launch_bits_mb<1, 2>(a.eq, n_sym, a.bits, s);
        case 2: return packed ? launch_bits_mb<2, 1>(a.eq, n_sym, a.bits, s) : launch_bits_mb<2, 2>(a.eq, n_sym, a.bits, s);
        case 4: return packed ? launch_bits_mb<4, 1>(a.eq, n_sym, a.bits, s) : launch_bits_mb<4, 2>(a.eq, n_sym, a.bits, s);
        case 6: return packed ? launch_bits_mb<6, 1>(a.eq, n_sym, a.bits, s) : launch_bits_mb<6, 2>(a.eq, n_sym, a.bits, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t chan_track_prepare() {
    return load_kernels(chan_track_link_kernel, chan_track_est_kernel<64>, chan_track_est_kernel<128>, chan_track_est_kernel<256>,
                        chan_track_est_kernel<512>, chan_track_est_kernel<1024>, chan_track_est_kernel<2048>,
                        chan_track_est_kernel<4096>, rx_demod_track_kernel<64>, rx_demod_track_kernel<128>,
                        rx_demod_track_kernel<256>, rx_demod_track_kernel<512>, rx_demod_track_kernel<1024>,
                        rx_demod_track_kernel<2048>, rx_demod_track_kernel<4096>, chan_track_bits_kernel<1, 2>,
                        chan_track_bits_kernel<2, 1>, chan_track_bits_kernel<2, 2>, chan_track_bits_kernel<4, 1>,
                        chan_track_bits_kernel<4, 2>, chan_track_bits_kernel<6, 1>, chan_track_bits_kernel<6, 2>);
}

}  // namespace ofdm
