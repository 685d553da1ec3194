// rx_sync.hip -- sync search kernels of the receive path (gfx950), the receiver's host tables and its size dispatch.
//
//   rx_sync_kernel         sequential timing search + finalize (mode 0) / trial table (mode 1)
//   rx_sync_scan_kernel    screened search of the batch path and of the stream block's segments (rx_sync_scan.hpp)
//   fo_decide_kernel, rx_fo_finalize_kernel     batch CFO receiver
//   rx_chan_time_kernel    est_chan_time on demand
#include "rx_sync.hpp"
#include "rx_sync_scan.hpp"     // one unit with the kernels below: the header says why

namespace ofdm {

// est_chan_time = ifft(est_chan_freq_P row) (:202,212) for rows of H, the same arithmetic as the finalize stage above.  The batch
// path computes it ON DEMAND (ofdm_rx_get_frame_state) instead of once per frame and launch: one FFT and 8 N bytes per frame that
// nothing on the data path reads.
template <int N>
__global__ void __launch_bounds__(Plan<N>::WG) rx_chan_time_kernel(RxDev rx, const cf* H, cf* htime, int n_rows) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = (T >= 64) ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;
    const int t = tid % T;
    cf* smem = reinterpret_cast<cf*>(smem_raw);
    cf* lds = smem + slot * WgLds<N>::STRIDE;
    const cf* w1tab = wg_init_w1<N>(smem, rx.tw, tid);
    std::conditional_t<PL::R0 == 16, CompactTwiddles<N>, LaneTwiddles<N>> tw;
    load_twiddles(tw, rx.tw, t);
    const int64_t row = int64_t(blockIdx.x) * PL::SLOTS + slot;
    const bool active = row < n_rows;
    cf v[P];
#pragma unroll
    for (int n0 = 0; n0 < P; ++n0) v[n0] = active ? cconj(H[row * N + t + T * n0]) : cf{0.f, 0.f};
    wg_fft<N>(v, lds, tw, w1tab, t);
    if (active) {
#pragma unroll
        for (int j = 0; j < PL::C; ++j) {
#pragma unroll
            for (int kl = 0; kl < PL::RL; ++kl)
                htime[row * N + (t + T * j) + PL::NC * kl] = cscale(cconj(v[out_slot<N>(j, kl)]), 1.f / float(N));
        }
    }
}

// TABLE: the trial table (mode 1) of a frame batch only -- frame = blockIdx.y -- without the mode-0 search and finalize, so that
// its register budget is that of one trial (batch CFO receiver).  TABLE = false is the stream blocks' kernel with both modes.
template <int N, int MINW = 3, bool TABLE = false>
__global__ void __launch_bounds__(Plan<N>::WG, MINW) rx_sync_kernel(RxDev rx, SyncArgs a) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = (T >= 64) ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;    // a wave lies inside one slot: uniform
    const int t = tid % T;
    cf* smem = reinterpret_cast<cf*>(smem_raw);
    cf* lds = smem + slot * WgLds<N>::STRIDE;
    float* red = reinterpret_cast<float*>(lds + WgLds<N>::ELEMS);
    const cf* w1tab = wg_init_w1<N>(smem, rx.tw, tid);

    // radix-16 first pass: 4 base twiddles + products on the fly (8 VGPRs instead of 30) keep the 168-register build off scratch
    std::conditional_t<PL::R0 == 16, CompactTwiddles<N>, LaneTwiddles<N>> tw;
    load_twiddles(tw, rx.tw, t);

    const int64_t unit = int64_t(blockIdx.x) * PL::SLOTS + slot;

    if (TABLE || a.mode == 1) {
        // ---- trial table: unit = cand * p_count + trial of frame blockIdx.y (TABLE) / of frame 0 (the stream blocks)
        const int64_t frame = TABLE ? int64_t(blockIdx.y) : 0;
        const int n_rot = a.n_rot > 1 ? a.n_rot : 1;
        const bool active = unit < int64_t(a.p_count) * n_rot;
        const int cand = active ? int(unit / a.p_count) : 0;            // candidate-major: unit = cand * p_count + w
        const int Ptrial = a.p_begin + int(unit % a.p_count);
        const cf* rot = a.rot ? a.rot + int64_t(cand) * N : nullptr;
        const bool valid = active && (a.host_valid || int64_t(rx.S) * rx.L + int64_t(Ptrial) * rx.stride + N + rx.cp < a.frame_len);  // :144
        cf Z[P];
        cf zdup;
        float p_est, m;
        int dhat;
        sync_trial<N>(rx, a.iq + frame * a.frame_stride, a.frame_len, valid, Ptrial, lds, red, tw, w1tab, t, Z, zdup, p_est, m, dhat,
                      nullptr, rot, a.off_delta);
        if (active && t == 0) {
            const int64_t o = frame * a.p_count * n_rot + unit;
            a.trial_m[o] = valid ? m : -1.f;
            a.trial_d[o] = valid ? dhat : 0;
        }
        return;
    }

    // ---- mode 0: sequential search per frame (first accepted trial wins, :166-219), then finalize
    const bool active = unit < a.n_frames;
    const int frame = active ? int(unit) : 0;
    const cf* frame_iq = a.iq + int64_t(frame) * a.frame_stride;
    cf* ysc = a.yscratch ? a.yscratch + int64_t(frame) * rx.MM : nullptr;

    bool found = false;
    cf Zs[P];                       // Z of the accepted trial
    cf zdups = cf{0.f, 0.f};
    float pests = 0.f, ms = 0.f;
    int dhats = 0, Phit = 0;
    if constexpr (PL::SLOTS == 1) {
        // one frame per workgroup: every decision is workgroup-uniform, so the accepted trial's registers are used
        // in place (no second copy of Z to keep alive across the search loop)
        for (int it = 0;; ++it) {
            const int Ptrial = a.p_begin + it;
            const bool valid = active && (a.p_count <= 0 || it < a.p_count) &&
                               (a.host_valid || int64_t(rx.S) * rx.L + int64_t(Ptrial) * rx.stride + N + rx.cp < a.frame_len);
            if (!valid) break;
            sync_trial<N>(rx, frame_iq, a.frame_len, valid, Ptrial, lds, red, tw, w1tab, t, Zs, zdups, pests, ms, dhats, ysc, a.rot, a.off_delta);
            if (a.force_dhat_p1 > 0) dhats = a.force_dhat_p1 - 1;
            if (a.force_accept || ms > rx.gate_mm) {                                    // :166
                found = true;
                Phit = Ptrial;
                break;
            }
        }
        if (!found) {
#pragma unroll
            for (int s = 0; s < P; ++s) Zs[s] = cf{0.f, 0.f};
            zdups = cf{0.f, 0.f};
            pests = 0.f;
            ms = 0.f;
            dhats = 0;
        }
    } else {
#pragma unroll
        for (int s = 0; s < P; ++s) Zs[s] = cf{0.f, 0.f};
        for (int it = 0;; ++it) {
            const int Ptrial = a.p_begin + it;
            const bool valid = active && !found && (a.p_count <= 0 || it < a.p_count) &&
                               (a.host_valid || int64_t(rx.S) * rx.L + int64_t(Ptrial) * rx.stride + N + rx.cp < a.frame_len);
            if (!__syncthreads_or(valid ? 1 : 0)) break;
            cf Z[P];
            cf zdup;
            float p_est, m;
            int dhat;
            sync_trial<N>(rx, frame_iq, a.frame_len, valid, Ptrial, lds, red, tw, w1tab, t, Z, zdup, p_est, m, dhat, ysc, a.rot, a.off_delta);
            if (a.force_dhat_p1 > 0) dhat = a.force_dhat_p1 - 1;
            if (valid && (a.force_accept || m > rx.gate_mm)) {                          // :166
                found = true;
#pragma unroll
                for (int s = 0; s < P; ++s) Zs[s] = Z[s];
                zdups = zdup;
                pests = p_est;
                ms = m;
                dhats = dhat;
                Phit = Ptrial;
            }
        }
    }

    sync_finalize<N>(rx, a, frame, active, found, Phit, Zs, zdups, pests, ms, dhats, lds, tw, w1tab, t, ysc);
}

// ------------------------------------------------------------------------------------------ batch CFO receiver
// What ofdm_fo_work decides on the host between its trial-table and finalize launches (SynchEstAndFO.py:282-298), for every
// frame of a batch at once: one wave per frame.  Per trial the best candidate (first maximum, strict >, :282-285); the trials
// that pass the gate (:288) are walked in order, 64 at a time from a ballot, by one lane that applies the distance rule
// against the previous accepted sync (:289-291, no break) and stops the frame at a 101st sync (:294-296).
__global__ void __launch_bounds__(64) fo_decide_kernel(RxDev rx, FoDecideArgs a) {
    __shared__ float s_m[64];
    __shared__ int s_d[64];
    __shared__ int s_state[3];                           // {rows accepted, last accepted window start, error}
    const int frame = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t base = int64_t(frame) * a.n_rot * a.p_count;
    const float* tm = a.trial_m + base;
    const int* td = a.trial_d + base;
    if (lane == 0) {
        s_state[0] = 0;
        s_state[1] = 0;
        s_state[2] = 0;
    }
    __syncthreads();
    int last_best = -1;                                  // :283 dmax_tmp_ind of the last trial (lane (p_count-1) % 64 holds it)
    const int64_t row0 = int64_t(frame) * a.rows;
    for (int p0 = 0; p0 < a.p_count; p0 += 64) {
        const int w = p0 + lane;
        const bool in = w < a.p_count;
        int best = 0;
        float bm = in ? tm[w] : 0.f;
        int bd = in ? td[w] : 0;
        for (int c = 1; c < a.n_rot; ++c) {
            const float v = in ? tm[int64_t(c) * a.p_count + w] : 0.f;
            if (v > bm) {
                bm = v;
                best = c;
                bd = td[int64_t(c) * a.p_count + w];
            }
        }
        if (in) last_best = best;
        const bool pass = in && bm > rx.gate_mm;
        unsigned long long mask = __ballot(pass);
        s_m[lane] = bm;
        s_d[lane] = bd;
        __syncthreads();
        if (lane == 0 && !s_state[2]) {
            int n = s_state[0], last = s_state[1];
            while (mask) {
                const int b = __ffsll(static_cast<long long>(mask)) - 1;
                mask &= mask - 1;
                const int pos = (p0 + b) * rx.stride + rx.cp;
                if (!(n == 0 || pos - last > 2 * rx.cp + rx.nfft)) continue;                  // :291
                if (n >= a.rows) {                                                              // :294-296 IndexError
                    s_state[2] = 1;
                    break;
                }
                const int lag = s_d[b], mi = int(s_m[b]);
                if (a.tsr_out) {
                    int* o = a.tsr_out + (row0 + n) * 3;
                    o[0] = pos;
                    o[1] = lag;
                    o[2] = mi;
                }
                int* u = a.u_tsr + (row0 + n) * 4;
                u[0] = pos;
                u[1] = lag;
                u[2] = mi;
                u[3] = 1;
                ++n;
                last = pos;
            }
            s_state[0] = n;
            s_state[1] = last;
        }
        __syncthreads();
    }
    // the last trial's pick sits in lane (p_count - 1) % 64 of the final pass
    const int src = a.p_count > 0 ? (a.p_count - 1) % 64 : 0;
    last_best = __shfl(last_best, src);
    const int n_sync = s_state[0];
    const bool err = s_state[2] != 0;
    if (lane == 0) {
        a.status[frame] = err ? a.err_index : n_sync;
        if (a.fo_idx) a.fo_idx[frame] = a.p_count > 0 ? last_best : -1;
    }
    // rows past the last sync: zero (an erroring frame keeps no live unit at all)
    for (int r = (err ? 0 : n_sync) + lane; r < a.rows; r += 64) {
        int* u = a.u_tsr + (row0 + r) * 4;
        u[0] = 0;
        u[1] = 0;
        u[2] = 0;
        u[3] = 0;
        if (a.tsr_out && r >= n_sync) {
            int* o = a.tsr_out + (row0 + r) * 3;
            o[0] = 0;
            o[1] = 0;
            o[2] = 0;
        }
    }
}

// LS estimate of one accepted sync per (frame, row) unit: the finalize launch of ofdm_fo_work (sync vector of the LAST candidate,
// lag of the best one, FO:268-274,300-329) with the trial and lag read from the decide kernel's table.  The same device functions
// as rx_sync_kernel mode 0 with force_accept, so the same numbers.  Units past a frame's syncs write zero rows; a workgroup with
// no live unit writes them without running the trial.
template <int N, int MINW>
__global__ void __launch_bounds__(Plan<N>::WG, MINW) rx_fo_finalize_kernel(RxDev rx, SyncArgs a, int units_per_frame) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = (T >= 64) ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;
    const int t = tid % T;
    const int64_t unit = int64_t(blockIdx.x) * PL::SLOTS + slot;
    const bool active = unit < a.n_frames;
    const int64_t u = active ? unit : 0;
    const int* ut = a.tsr + u * 4;
    const int pos = active ? ut[0] : 0, lag = active ? ut[1] : 0;
    const bool live = active && ut[3] != 0;
    const int Ptrial = (pos - rx.cp) / rx.stride;
    cf* ysc = a.esf ? a.esf + u * rx.MM : nullptr;      // raw sync-bin values go where est_synch_freq is formed from them, in place
    if (!__syncthreads_or(live ? 1 : 0)) {
        if (active) {
            for (int k = t; k < N; k += T) {
                if (a.H) a.H[u * N + k] = cf{0.f, 0.f};
                if (a.htime) a.htime[u * N + k] = cf{0.f, 0.f};
            }
            if (a.esf)
                for (int k = t; k < rx.MM; k += T) a.esf[u * rx.MM + k] = cf{0.f, 0.f};
        }
        return;
    }
    cf* smem = reinterpret_cast<cf*>(smem_raw);
    cf* lds = smem + slot * WgLds<N>::STRIDE;
    float* red = reinterpret_cast<float*>(lds + WgLds<N>::ELEMS);
    const cf* w1tab = wg_init_w1<N>(smem, rx.tw, tid);
    std::conditional_t<PL::R0 == 16, CompactTwiddles<N>, LaneTwiddles<N>> tw;
    load_twiddles(tw, rx.tw, t);
    const cf* frame_iq = a.iq + (u / units_per_frame) * a.frame_stride;
    const bool valid = live && int64_t(rx.S) * rx.L + int64_t(Ptrial) * rx.stride + N + rx.cp < a.frame_len;   // :249 (defensive)
    cf Z[P];
    cf zdup;
    float p_est, m;
    int dhat;
    sync_trial<N>(rx, frame_iq, a.frame_len, valid, Ptrial, lds, red, tw, w1tab, t, Z, zdup, p_est, m, dhat, ysc, a.rot, 0);
    sync_finalize<N, decltype(tw), true>(rx, a, int(u), active, valid, Ptrial, Z, zdup, p_est, m, lag, lds, tw, w1tab, t, ysc);
}

// ------------------------------------------------------------------------------------------ launchers
template <int N>
static hipError_t launch_sync_n(const RxDev& rx, const SyncArgs& a, hipStream_t s) {
    const int64_t units = (a.mode == 1) ? int64_t(a.p_count) * (a.n_rot > 1 ? a.n_rot : 1) : a.n_frames;
    const unsigned grid = unsigned((units + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    if (grid == 0) return hipSuccess;
    if (a.mode == 0 && a.scan_block > 0) return launch_sync_scan_n<N>(rx, a, grid, s);
    // 3 waves per SIMD (168 VGPRs, a few spills off the trial path): 0.14 ms instead of 0.21 ms per 4369-frame launch; the
    // unconstrained build takes 192 VGPRs + 256 AGPRs (1 wave per SIMD), a 128-register build spills into the trial (0.20 ms)
    if (a.mode == 1 && a.n_frames > 1) {
        // trial table of a frame batch: one grid row per frame (gridDim.y <= 65535: the batch CFO path launches larger batches in parts)
        if (a.n_frames > 65535) return hipErrorInvalidValue;
        // 1024 / 2048-pt: 2 waves per SIMD keep the trial off scratch (3 spill 6 / 9 VGPRs)
        constexpr int TMW = (N == 1024 || N == 2048) ? 2 : 3;
        hipLaunchKernelGGL((rx_sync_kernel<N, TMW, true>), dim3(grid, unsigned(a.n_frames)), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((rx_sync_kernel<N, 3>), dim3(grid), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, a);
    return hipGetLastError();
}

// one translation unit per FFT size defines its own (rx_demod_<N>.hip)
#define OFDM_DECLARE_DEMOD(n) hipError_t launch_rx_demod_##n(const RxDev& rx, const DemodArgs& a, hipStream_t s);
OFDM_DECLARE_DEMOD(64)
OFDM_DECLARE_DEMOD(128)
OFDM_DECLARE_DEMOD(256)
OFDM_DECLARE_DEMOD(512)
OFDM_DECLARE_DEMOD(1024)
OFDM_DECLARE_DEMOD(2048)
OFDM_DECLARE_DEMOD(4096)
#undef OFDM_DECLARE_DEMOD

hipError_t launch_rx_demod(const RxDev& rx, const DemodArgs& a, hipStream_t s) {
#define CALL(n) launch_rx_demod_##n(rx, a, s)
    OFDM_DISPATCH_N(rx.nfft, CALL, hipErrorInvalidValue)
#undef CALL
}
hipError_t launch_rx_sync(const RxDev& rx, const SyncArgs& a, hipStream_t s) {
#define CALL(n) launch_sync_n<n>(rx, a, s)
    OFDM_DISPATCH_N(rx.nfft, CALL, hipErrorInvalidValue)
#undef CALL
}
hipError_t launch_fo_decide(const RxDev& rx, const FoDecideArgs& a, hipStream_t s) {
    if (a.n_frames <= 0) return hipSuccess;
    if (!a.status || !a.u_tsr || a.rows <= 0 || a.n_rot < 1 || a.p_count < 0 || (a.p_count > 0 && (!a.trial_m || !a.trial_d)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fo_decide_kernel, dim3(unsigned(a.n_frames)), dim3(64), 0, s, rx, a);
    return hipGetLastError();
}
// 2 waves per SIMD: the trial and the finalize of one unit stay in registers (no scratch; a unit runs once per sync)
template <int N>
static hipError_t launch_fo_finalize_n(const RxDev& rx, const SyncArgs& a, int units_per_frame, hipStream_t s) {
    const unsigned grid = unsigned((int64_t(a.n_frames) + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL((rx_fo_finalize_kernel<N, 2>), dim3(grid), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, a, units_per_frame);
    return hipGetLastError();
}
hipError_t launch_fo_finalize(const RxDev& rx, const SyncArgs& a, int units_per_frame, hipStream_t s) {
    if (units_per_frame < 1 || !a.tsr || !a.gain) return hipErrorInvalidValue;
#define CALL(n) launch_fo_finalize_n<n>(rx, a, units_per_frame, s)
    OFDM_DISPATCH_N(rx.nfft, CALL, hipErrorInvalidValue)
#undef CALL
}
template <int N>
static std::vector<cf> zc_lane_table_n(int Ks, int S, const cf* zc) {
    using PL = Plan<N>;
    std::vector<cf> out(size_t(S) * N, cf{0.f, 0.f});
    const int h = Ks / 2;
    for (int LL = 0; LL < S; ++LL)
        for (int t = 0; t < PL::T; ++t)
            for (int j = 0; j < PL::C; ++j)
                for (int kl = 0; kl < PL::RL; ++kl) {
                    const int k = (t + PL::T * j) + PL::NC * kl;
                    cf z = cf{0.f, 0.f};
                    if (k >= N - h) z = zc[LL * Ks + (k - (N - h))];            // negative half of binsP(Ks)
                    if (k >= 1 && k <= h) z = zc[LL * Ks + (h + k - 1)];        // positive half (the later entry of a bin listed twice)
                    out[size_t(LL) * N + size_t(out_slot<N>(j, kl)) * PL::T + t] = z;
                }
    return out;
}

std::vector<cf> rx_zc_lane_table(int nfft, int Ks, int S, const cf* zc) {
#define CALL(n) zc_lane_table_n<n>(Ks, S, zc)
    OFDM_DISPATCH_N(nfft, CALL, std::vector<cf>(size_t(S) * nfft, cf{0.f, 0.f}))
#undef CALL
}

size_t rx_lds_bytes(int nfft) {
#define CALL(n) WgLds<n>::BYTES
    OFDM_DISPATCH_N(nfft, CALL, 0)
#undef CALL
}

template <int N>
static hipError_t launch_chan_time_n(const RxDev& rx, const cf* H, cf* htime, int n_rows, hipStream_t s) {
    const unsigned grid = unsigned((n_rows + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    hipLaunchKernelGGL(rx_chan_time_kernel<N>, dim3(grid), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, H, htime, n_rows);
    return hipGetLastError();
}
hipError_t launch_rx_chan_time(const RxDev& rx, const cf* H, cf* htime, int n_rows, hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
#define CALL(n) launch_chan_time_n<n>(rx, H, htime, n_rows, s)
    OFDM_DISPATCH_N(rx.nfft, CALL, hipErrorInvalidValue)
#undef CALL
}

}  // namespace ofdm
