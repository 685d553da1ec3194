// rx_sync.hpp -- one sync trial and the finalize stage of the receive path (gfx950), shared by the sync kernels (rx_sync.hip)
// and the screened search (rx_sync_scan.hpp).
//
//   sync_trial       Zadoff-Chu lag-correlation of one window: FFT, correlation, inverse FFT, arg-max lag
//                    (reference: gr-utsa_ofdm/python/SynchAndChanEst.py:143-164)
//   sync_finalize    LS channel estimate + equaliser gains of the accepted trial   (:171-218)
//
// Layout: one OFDM symbol is owned by T = N/16 lanes (fft_core.hpp); a workgroup holds max(T,64)
// lanes = SLOTS symbols side by side.  A symbol is read from HBM exactly once (coalesced, CP skipped
// by offset), lives in VGPRs/LDS through the FFT, and leaves as one coalesced 16 B/lane store of
// its Kd equalised bins (+ packed bits).  No MFMA: the path is FFT + elementwise, HBM-bound.
#pragma once
#include <type_traits>

#include "ofdm_launch.hpp"

namespace ofdm {

// ------------------------------------------------------------------------------------------ sync
// One sync trial P of one frame (SynchAndChanEst.py:145-164).  On return: Z (per-lane bins, register
// slot order) = sum over the S sync symbols of Y[k]*conj(zc), zdup = negative-half part of a bin that
// is listed twice (K == N only), p_est, m = max|del_mat|, dhat = argmax lag.
// KEEP > 0 (scan kernel, S == 1): additionally returns, per lane, the COMPLEX lag correlations c[a] for a = t + T*q, q < KEEP
// (ukeep), the in-band energy sum |Y|^2 (ekeep) and -- in red[16..19] -- the DC and Nyquist bins of the window's FFT.
template <int N, class TW, int KEEP = 0>
__device__ __forceinline__ void sync_trial(const RxDev& rx, const cf* frame_iq, int64_t frame_len, bool active,
                                           int Ptrial, cf* lds, float* red, const TW& tw, const cf* w1tab, int t,
                                           cf (&Z)[Plan<N>::P], cf& zdup, float& p_est, float& m, int& dhat,
                                           cf* yscratch, const cf* rot = nullptr, int off = 0,
                                           cf* ukeep = nullptr, float* ekeep = nullptr) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
    int* redi = reinterpret_cast<int*>(red) + 8;
#pragma unroll
    for (int s = 0; s < P; ++s) Z[s] = cf{0.f, 0.f};
    zdup = cf{0.f, 0.f};
    float psum = 0.f;
    for (int LL = 0; LL < rx.S; ++LL) {
        const int64_t w0 = int64_t(rx.L) * LL + int64_t(Ptrial) * rx.stride + rx.cp + off;   // :146
        cf v[P];
#pragma unroll
        for (int n0 = 0; n0 < P; ++n0) {
            const int64_t idx = w0 + t + T * n0;
            v[n0] = (active && idx < frame_len) ? frame_iq[idx] : cf{0.f, 0.f};
            if (rot) v[n0] = cmul(v[n0], rot[t + T * n0]);          // sig_with_fo = dat_time * cfo[fo]  (SynchEstAndFO.py:264)
        }
        wg_fft<N>(v, lds, tw, w1tab, t);                                                       // :152
        if constexpr (KEEP > 0) {
            if (t == 0) {                                   // bins 0 and N/2 both live in lane 0
                const cf y0 = v[out_slot<N>(0, 0)], yh = v[out_slot<N>(0, PL::RL / 2)];
                red[16] = y0.x;
                red[17] = y0.y;
                red[18] = yh.x;
                red[19] = yh.y;
            }
        }
        int Ks_ = rx.Ks;                      // opaque per segment: keeps the 32 per-slot table offsets out of long-lived VGPRs
        asm volatile("" : "+s"(Ks_));
        const cf* zcs = rx.zc + LL * Ks_;
        cf* ys = yscratch ? yscratch + LL * Ks_ : nullptr;
        // The Zadoff-Chu entry of every bin this lane holds, from the LANE-ORDER copy of the table (RxDev::zcp): entry
        // [slot*T + t], zero for bins outside the list.  One base address, sixteen independent coalesced reads in flight together.
        // (Gathering zc[list index of bin k] through per-bin index arithmetic put 48 loop-invariant VGPRs of indices and addresses
        // across the trial loop and made hipcc wait for every read on its own: 16 global-memory latencies per FFT.)
        const cf* zp = rx.zcp + LL * N + t;
        cf zt[P];
#pragma unroll
        for (int s = 0; s < P; ++s) zt[s] = zp[s * T];
        // every read issued before any is consumed (one opaque use of all of them: hipcc otherwise sinks each read to its use
        // and waits for it there)
        if constexpr (P == 16) {
            asm volatile("" : "+v"(zt[0]), "+v"(zt[1]), "+v"(zt[2]), "+v"(zt[3]), "+v"(zt[4]), "+v"(zt[5]), "+v"(zt[6]), "+v"(zt[7]),
                              "+v"(zt[8]), "+v"(zt[9]), "+v"(zt[10]), "+v"(zt[11]), "+v"(zt[12]), "+v"(zt[13]), "+v"(zt[14]), "+v"(zt[15]));
        } else {
            asm volatile("" : "+v"(zt[0]), "+v"(zt[1]), "+v"(zt[2]), "+v"(zt[3]), "+v"(zt[4]), "+v"(zt[5]), "+v"(zt[6]), "+v"(zt[7]));
        }
#pragma unroll
        for (int j = 0; j < PL::C; ++j) {
#pragma unroll
            for (int kl = 0; kl < PL::RL; ++kl) {
                const int k = (t + T * j) + PL::NC * kl;
                const int s = out_slot<N>(j, kl);
                int in_, ip_;
                const bool neg = bin_neg(k, Ks_, N, in_), pos = bin_pos(k, Ks_, ip_);   // :153-161
                const bool used = neg || pos;
                Z[s] = Z[s] + cmulc(v[s], zt[s]);
                psum += used ? cnorm2(v[s]) : 0.f;
            }
        }
        if (Ks_ == N) {                             // K == N lists bin N/2 twice (ofdm_chain.py:83 wiring); zcp holds its LAST
#pragma unroll                                      // (positive-half) entry, the first (negative-half) one is added here
            for (int j = 0; j < PL::C; ++j) {
#pragma unroll
                for (int kl = 0; kl < PL::RL; ++kl) {
                    const int k = (t + T * j) + PL::NC * kl;
                    const int s = out_slot<N>(j, kl);
                    if (k == N / 2) {
                        const cf c = cmulc(v[s], zcs[0]);                               // negative half: list index 0
                        zdup = zdup + c;
                        Z[s] = Z[s] + c;
                        psum += cnorm2(v[s]);
                    }
                }
            }
        }
        if (ys && active) {                         // raw sync-bin values for est_synch_freq, AFTER the reads above: a store
#pragma unroll                                      // between two table reads would order them (the pointers may alias)
            for (int j = 0; j < PL::C; ++j) {
#pragma unroll
                for (int kl = 0; kl < PL::RL; ++kl) {
                    const int k = (t + T * j) + PL::NC * kl;
                    int in_, ip_;
                    const bool neg = bin_neg(k, Ks_, N, in_);
                    const bool pos = bin_pos(k, Ks_, ip_);
                    if (neg) ys[in_] = v[out_slot<N>(j, kl)];
                    if (pos) ys[ip_] = v[out_slot<N>(j, kl)];
                }
            }
        }
        wg_barrier();
    }
    psum = symbol_sum<T>(psum, red, t);
    p_est = sqrtf(float(rx.MM) / psum);                                                 // :157
    if constexpr (KEEP > 0) *ekeep = psum;

    // del_mat[d] = sum_k e^{+j 2pi d k/N} Z[k]  == unnormalised inverse DFT of Z read at d = 0..cp
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) lds[(t + T * j) + PL::NC * kl] = Z[out_slot<N>(j, kl)];
    }
    wg_barrier();
    cf v[P];
#pragma unroll
    for (int n0 = 0; n0 < P; ++n0) v[n0] = cconj(lds[t + T * n0]);
    wg_barrier();
    wg_fft<N>(v, lds, tw, w1tab, t);
    float best = -1.f;
    int bi = -1;
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int d = (t + T * j) + PL::NC * kl;
            const float m2 = cnorm2(v[out_slot<N>(j, kl)]);
            if (d <= rx.cp && (bi < 0 || m2 > best || (m2 == best && d < bi))) {        // :163 first max
                best = m2;
                bi = d;
            }
        }
    }
    if constexpr (KEEP > 0) {
        // lag a = t + T*q sits in register slot (j, kl) = (q % C, q / C): NC = T*C
#pragma unroll
        for (int q = 0; q < KEEP; ++q) ukeep[q] = cconj(v[out_slot<N>(q % PL::C, q / PL::C)]);
    }
    symbol_argmax<T>(best, bi, red, redi, t);
    m = p_est * sqrtf(best);                                                            // :164
    dhat = bi;
    wg_barrier();
}

// ---- finalize (:171-218): LS estimate on the sync bins, equaliser gains, channel impulse response.
// Shared by the sequential and the screened search kernels; Zs .. dhats describe the accepted trial (zeros if none).
// OPT_H (batch CFO receiver only): est_chan_freq_P is an optional output, a.H may be null.
template <int N, class TW, bool OPT_H = false>
__device__ __forceinline__ void sync_finalize(const RxDev& rx, const SyncArgs& a, int frame, bool active, bool found, int Phit,
                                              const cf (&Zs)[Plan<N>::P], cf zdups, float pests, float ms, int dhats, cf* lds,
                                              const TW& tw, const cf* w1tab, int t, cf* ysc) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
    const int Ks = rx.Ks, Kd = rx.Kd;
    if (active && t == 0) {
        int* o = a.tsr + int64_t(frame) * 4;
        if (found || !a.keep_on_miss) {
            o[0] = found ? Phit * rx.stride + rx.cp + a.off_delta : 0;                  // :173
            o[1] = found ? dhats : 0;                                                    // :174
            o[2] = found ? int(ms) : 0;                                                  // :175
        }
        o[3] = found ? 1 : 0;
        if (a.tsr_host) {
            int* oh = a.tsr_host + int64_t(frame) * 4;
            if (found || !a.keep_on_miss) {
                oh[0] = o[0];
                oh[1] = o[1];
                oh[2] = o[2];
            }
            oh[3] = found ? 1 : 0;
        }
    }
    active = active && (found || !a.keep_on_miss);     // from here on `active` only gates the stores
    // Z (register slot order) -> LDS in natural bin order, then a rolled loop over this lane's bins: the finalize
    // arithmetic runs once per frame, so it is kept small in registers rather than unrolled 16-fold.
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int k = (t + T * j) + PL::NC * kl;
            lds[k] = Zs[out_slot<N>(j, kl)];
            if (Ks == N && k == N / 2) lds[N] = zdups;          // negative-half part of the bin listed twice (K == N)
        }
    }
    wg_barrier();
    const float sc = pests * rx.inv_ls;                                                 // p_est / (S (1+1/snr)) :180-184
    // the lag de-rotation e^{+j 2pi d k/N} of this lane's 16 bins (:177): sixteen independent table reads issued together
    // (one per loop iteration, each waited for on its own, was a third of the kernel's time in the aligned case)
    cf rots[P];
#pragma unroll
    for (int q = 0; q < P; ++q) rots[q] = rx.tw[(dhats * (t + T * q)) & (N - 1)];
    if constexpr (P == 16) {
        asm volatile("" : "+v"(rots[0]), "+v"(rots[1]), "+v"(rots[2]), "+v"(rots[3]), "+v"(rots[4]), "+v"(rots[5]), "+v"(rots[6]), "+v"(rots[7]),
                          "+v"(rots[8]), "+v"(rots[9]), "+v"(rots[10]), "+v"(rots[11]), "+v"(rots[12]), "+v"(rots[13]), "+v"(rots[14]), "+v"(rots[15]));
    } else {
        asm volatile("" : "+v"(rots[0]), "+v"(rots[1]), "+v"(rots[2]), "+v"(rots[3]), "+v"(rots[4]), "+v"(rots[5]), "+v"(rots[6]), "+v"(rots[7]));
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
        const int k = t + T * q;
        const cf Zk = lds[k];
        int in_, ip_;
        const bool neg = bin_neg(k, Ks, N, in_);
        const bool pos = bin_pos(k, Ks, ip_);
        const cf zd = (pos && neg) ? lds[N] : cf{0.f, 0.f};
        const cf rot = cconj(rots[q]);                                                  // e^{+j 2pi d k/N}  :177
        const cf Hn = cscale(cmul(rot, (pos && neg) ? zd : Zk), sc);
        const cf Hp = cscale(cmul(rot, (pos && neg) ? (Zk - zd) : Zk), sc);
        // chan_est1[synch_bins] = chan_est : a bin listed twice keeps its LAST (positive-half) entry :186-188
        cf Hk = cf{0.f, 0.f};
        if (found && neg) Hk = Hn;
        if (found && pos) Hk = Hp;
        lds[k] = Hk;                               // natural-order H for the est_chan_time inverse FFT below (same lane, same slot)
        if (active) {
            if (!OPT_H || a.H) a.H[int64_t(frame) * N + k] = Hk;
            if (a.eqg || a.esf) {
                // eq_gain = conj(chan_est)/(|chan_est|^2 + 1/snr) (:213-216); est_synch_freq = eq_gain * r (:217-218)
                if (neg) {
                    const cf e = found ? cscale(cconj(Hn), 1.f / (cnorm2(Hn) + rx.inv_snr_eqsync)) : cf{0.f, 0.f};
                    if (a.eqg) a.eqg[int64_t(frame) * Ks + in_] = e;
                    if (a.esf && ysc)
                        for (int LL = 0; LL < rx.S; ++LL)
                            a.esf[int64_t(frame) * rx.MM + LL * Ks + in_] =
                                found ? cmul(e, cscale(cmul(rot, ysc[LL * Ks + in_]), pests)) : cf{0.f, 0.f};
                }
                if (pos) {
                    const cf e = found ? cscale(cconj(Hp), 1.f / (cnorm2(Hp) + rx.inv_snr_eqsync)) : cf{0.f, 0.f};
                    if (a.eqg) a.eqg[int64_t(frame) * Ks + ip_] = e;
                    if (a.esf && ysc)
                        for (int LL = 0; LL < rx.S; ++LL)
                            a.esf[int64_t(frame) * rx.MM + LL * Ks + ip_] =
                                found ? cmul(e, cscale(cmul(rot, ysc[LL * Ks + ip_]), pests)) : cf{0.f, 0.f};
                }
            }
            // data-bin gain: conj(Hd)/(|Hd|^2 + 1/SNR_lin) (:242-246) folded with the lag de-rotation (:237-240)
            const cf Hg = a.H_for_gain ? a.H_for_gain[int64_t(frame) * N + k] : Hk;
            const cf rot_g = a.gain_lag_set ? cconj(rx.tw[(a.gain_lag * k) & (N - 1)]) : rot;
            const cf gk = cmul(cscale(cconj(Hg), 1.f / (cnorm2(Hg) + rx.inv_snr_data)), rot_g);
            int id_;
            if (bin_neg(k, Kd, N, id_)) a.gain[int64_t(frame) * Kd + id_] = gk;
            if (bin_pos(k, Kd, id_)) a.gain[int64_t(frame) * Kd + id_] = gk;
        }
    }
    if (a.htime) {                                                                      // :202,212  ifft(chan_est1)
        wg_barrier();
        cf v[P];
#pragma unroll
        for (int n0 = 0; n0 < P; ++n0) v[n0] = cconj(lds[t + T * n0]);
        wg_barrier();
        wg_fft<N>(v, lds, tw, w1tab, t);
        if (active) {
#pragma unroll
            for (int j = 0; j < PL::C; ++j) {
#pragma unroll
                for (int kl = 0; kl < PL::RL; ++kl)
                    a.htime[int64_t(frame) * N + (t + T * j) + PL::NC * kl] =
                        cscale(cconj(v[out_slot<N>(j, kl)]), 1.f / float(N));
            }
        }
    }
}

// return CALL(n) of the compiled FFT size n == nfft, MISS for every other nfft (host code)
#define OFDM_DISPATCH_N(nfft, CALL, MISS) \
    switch (nfft) {                       \
        case 64: return CALL(64);         \
        case 128: return CALL(128);       \
        case 256: return CALL(256);       \
        case 512: return CALL(512);       \
        case 1024: return CALL(1024);     \
        case 2048: return CALL(2048);     \
        case 4096: return CALL(4096);     \
        default: return MISS;             \
    }

}  // namespace ofdm
