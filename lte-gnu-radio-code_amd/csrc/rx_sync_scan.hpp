// rx_sync_scan.hpp -- the screened sync search of the receive path (gfx950): rx_sync_scan_kernel and its launches.
//
// Compiled as part of rx_sync.hip, not as a unit of its own, on purpose.  hipcc's inliner orders its work by how many callers a
// helper has in the module, and the FFT helpers are shared: without the scan kernels beside them the 512-, 1024- and 2048-pt
// instantiations of rx_sync_kernel, rx_fo_finalize_kernel and rx_chan_time_kernel come out with other LDS address arithmetic
// (profiles/rx_split_isa_identity.txt).  A unit of its own is a change of those kernels and has to be measured as one.
#pragma once
#include "rx_sync.hpp"

#ifndef OFDM_SCAN_MINW
#define OFDM_SCAN_MINW 2        // waves per SIMD the screened sync search is compiled for (3: a 168-VGPR budget)
#endif

namespace ofdm {

// ------------------------------------------------------------------------------------------ screened sync search
// The reference tries the windows P = 0, 1, 2, ... one sample apart and, for each, forms the cp+1 lag correlations
// c_P[d] = sum_k e^{j 2pi d k/N} Y_P[k] conj(zc_k) from a fresh FFT (SynchAndChanEst.py:143-164).  Consecutive windows
// share N-1 samples: with D_P = x[w+N] - x[w] (w = first sample of window P),
//     Y_{P+1}[k] = (Y_P[k] + D_P) e^{j 2pi k/N}      =>      c_{P+1}[d] = c_P[d+1] + D_P * G[d+1],
//     G[m] = sum_k e^{j 2pi m k/N} conj(zc_k)   (a table, built once per handle)
// and, for num_synch_bins = N-2 (every bin but DC and Nyquist, the reference's convention), the in-band energy that
// normalises the correlation (:157) follows from three sliding sums:  E_P = N sum|x|^2 - |sum x|^2 - |sum (-1)^n x|^2.
// In "alignment" coordinates a = d + (P - P0) every correlation value is a running sum u[a] += D * G[a - j + 1], one
// complex multiply-add per step j and alignment: O(B + cp) per trial instead of two N-point FFTs.
//
// The recurrence runs in fp32, so it only SCREENS: a block of B trials starts from an exactly evaluated anchor trial
// (the same sync_trial as everywhere else); a trial whose screened peak exceeds (1 - 2e-4) * gate * MM -- or whose window
// energy is too small for the sliding sums to be trusted -- is re-evaluated exactly, in order, and only the exact value
// decides (:166).  Trials the screen rejects lie at least 2e-4 * gate * MM below the gate, ten times what the recurrence
// can drift over one block (<= 256 steps of ~6e-8 relative rounding), so the accepted trial and its lag are those of the
// exhaustive search.  Frames whose sync sits at trial 0 never enter the recurrence.
// Preconditions checked by the host: S == 1, stride == 1, Ks == N - 2, no rotator, B + cp <= SCAN_QM * T.
#ifndef OFDM_SCAN_MX_T256
#define OFDM_SCAN_MX_T256 5
#endif
template <int N>
struct ScanGeom {
    static constexpr int T = Plan<N>::T;
    static constexpr int QM = (T >= 256) ? 2 : (T >= 128) ? 3 : (T >= 64) ? 4 : (T >= 32) ? 6 : (Plan<N>::P < 12 ? Plan<N>::P : 12);
    static constexpr int BMAX = (QM * T < 256) ? QM * T : 256;        // longest block (trials per anchor) the recurrence walks
    // The cold-block test (below) needs no recurrence state, only the anchor's lag vector: where one frame owns the workgroup it
    // looks MX blocks ahead, so a frame whose sync lies far away pays one anchor per MX * B trials.
    static constexpr int MX = (T >= 256) ? OFDM_SCAN_MX_T256 : (T >= 128) ? 3 : (T >= 64) ? 2 : 1;     // (two at 1024-pt: three would spill)
    static constexpr int BX = MX * BMAX;                              // window-edge samples / thresholds held per anchor
    static constexpr int KX = MX * QM;                                // lag values per lane the anchor keeps (alignments a < KX * T)
    static_assert(KX <= Plan<N>::P, "the anchor's inverse FFT holds P lags per lane");
    static constexpr int RMAX = (BX + T - 1) / T;                     // window-edge samples per lane
    static constexpr int UNR = QM >= 8 ? 1 : (QM >= 6 ? 2 : 4);       // recurrence steps per loop iteration (register budget)
    // extra LDS per slot (cf units): dl[BX + 2 UNR] | xn[BX] | BMAX zeros, then G[0 .. QM*T] | thr[BX + 2 UNR floats] | flag
    static constexpr int DL_OFF = 0, XN_OFF = BX + 2 * UNR, GZ_OFF = XN_OFF + BX, G_OFF = GZ_OFF + BMAX,
                         THR_OFF = G_OFF + QM * T + 2;
    static constexpr int FLAG_OFF = THR_OFF + (BX + 2 * UNR + 1) / 2;
    static constexpr int CK = 16;                                     // steps per checkpoint window (a multiple of 2 UNR)
    static constexpr int NCHK = BMAX / CK + 2;
    static constexpr int CHK_OFF = FLAG_OFF + 1;                      // tchk[NCHK floats]
    static constexpr int BLK_OFF = CHK_OFF + (NCHK + 1) / 2;          // per wave {min thr, sum |D|} of the long and of the first block
    static constexpr int EXTRA = BLK_OFF + 10;                        // 16 floats of block totals + 4 of first hot lags
    static constexpr size_t BYTES = WgLds<N>::BYTES + size_t(Plan<N>::SLOTS) * EXTRA * sizeof(cf);
};

// u += d * g  (complex) in two packed FMAs: (d.x g.x + u.x, d.x g.y + u.y), then (d.y (-g.y) + u.x, d.y g.x + u.y)
__device__ __forceinline__ void cfma(cf& u, cf d, cf g) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "+v"(u)
        : "v"(d), "v"(g));
}

//
// SEG (stream block, one long buffer): the trial range is cut into segments of a.seg_len trials, one per workgroup slot, searched in
// parallel, in one or more launches.  Each segment publishes its first accepted trial with an atomicMin; a one-workgroup launch
// behind them (a.seg_final) re-evaluates the overall minimum exactly (the same code at the same trial: the same numbers) and
// finalizes it, so the search still returns the reference's "first accepted trial" and its estimate.  Segments behind an
// already published hit stop early.  (Round 2 let the segment that finished last finalize: one ticket per segment on one word,
// ~2000 serialised atomics per 240-symbol buffer -- most of that launch's 0.12 ms.)
template <int N, int MINW = 2, bool SEG = false>
__global__ void __launch_bounds__(Plan<N>::WG, MINW) rx_sync_scan_kernel(RxDev rx, SyncArgs a) {
    using PL = Plan<N>;
    using SG = ScanGeom<N>;
    constexpr int T = PL::T, P = PL::P, QM = SG::QM, SLOTS = PL::SLOTS;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = (T >= 64) ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;    // a wave lies inside one slot: uniform
    const int t = tid % T;
    cf* smem = reinterpret_cast<cf*>(smem_raw);
    cf* lds = smem + slot * WgLds<N>::STRIDE;
    float* red = reinterpret_cast<float*>(lds + WgLds<N>::ELEMS);
    int* redi = reinterpret_cast<int*>(red);
    if constexpr (SEG) {
        if (a.seg_final) {
            // (both words are stable here: every search launch whose result this launch looks at lies before it in its stream)
            const int w0 = __hip_atomic_load(a.seg_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int done = __hip_atomic_load(a.seg_state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.seg_final == 2) {
                if (w0 == 0x7fffffff) return;                  // early finalize, nothing found yet: the later stages go on
            } else if (done || (w0 == 0x7fffffff && a.keep_on_miss)) {
                // the early finalize has done the work, or the search ends without a hit (the old estimate stays in force, only
                // "not detected" is reported): re-arm, no table, no transform
                if (tid == 0) {
                    if (!done) {
                        a.tsr[3] = 0;
                        if (a.tsr_host) a.tsr_host[3] = 0;
                    }
                    __hip_atomic_store(a.seg_state, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(a.seg_state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                return;
            }
        }
        if (!a.seg_final) {
            // A workgroup whose segments all lie behind an already published hit has nothing to do -- before any table is loaded.
            // (Voted: the waves of a workgroup may read different values of the word, which only ever decreases.)
            const int64_t first_p = int64_t(a.p_begin) + (int64_t(a.seg_base) + int64_t(blockIdx.x) * SLOTS) * a.seg_len;
            if (__syncthreads_and(__hip_atomic_load(a.seg_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < first_p ? 1 : 0)) return;
        }
    }
    const cf* w1tab = wg_init_w1<N>(smem, rx.tw, tid);
    cf* extra = smem + WgLds<N>::STRIDE * SLOTS + WgLds<N>::W1_ELEMS + slot * SG::EXTRA;
    cf* xo = extra + SG::DL_OFF;          // window-edge samples leaving; overwritten by dl[i] = xn[i] - xo[i]
    cf* xn = extra + SG::XN_OFF;          // window-edge samples entering
    cf* Gl = extra + SG::G_OFF;           // preceded by BMAX zero entries: alignments that are not needed yet add nothing
    float* thr = reinterpret_cast<float*>(extra + SG::THR_OFF);
    int* cflag = reinterpret_cast<int*>(extra + SG::FLAG_OFF);
    float* tchk = reinterpret_cast<float*>(extra + SG::CHK_OFF);
    float* blk = reinterpret_cast<float*>(extra + SG::BLK_OFF);
    const float gmax = a.scan_g[N + 1].x * (1.f + 1e-5f);             // max |G[m]| (host, fp64), rounded up

    std::conditional_t<PL::R0 == 16, CompactTwiddles<N>, LaneTwiddles<N>> tw;
    load_twiddles(tw, rx.tw, t);

    const int64_t unit = (SEG ? int64_t(a.seg_base) : 0) + int64_t(blockIdx.x) * SLOTS + slot;
    // (a staged segment search: this launch owns the segments seg_base .. seg_base + seg_launch - 1 of n_seg)
    bool active = unit < (SEG ? int64_t(min(a.n_seg, a.seg_base + a.seg_launch)) : a.n_frames);
    const int frame = (active && !SEG) ? int(unit) : 0;
    const cf* frame_iq = a.iq + int64_t(frame) * a.frame_stride;
    // (a run-time pointer on purpose: with a literal nullptr hipcc's schedule of the trial needs ~3000 spills at 168 VGPRs)
    cf* ysc = a.yscratch ? a.yscratch + int64_t(frame) * rx.MM : nullptr;
    const int B = a.scan_block, cp = rx.cp;
    // trials p_begin <= P < nvalid are searched: P valid iff S*L + P + N + cp < frame_len (:144), P < p_count
    int64_t nvalid64 = a.frame_len - (int64_t(rx.S) * rx.L + N + cp);
    if (nvalid64 < 0) nvalid64 = 0;
    if (a.p_count > 0 && nvalid64 > a.p_count) nvalid64 = a.p_count;
    int nvalid = active ? int(nvalid64 < (1 << 30) ? nvalid64 : (1 << 30)) : 0;
    int P0 = a.p_begin;
    if constexpr (SEG) {
        const int64_t first = int64_t(a.p_begin) + (active ? unit : 0) * a.seg_len;
        P0 = int(first < (1 << 30) ? first : (1 << 30));
        if (int64_t(nvalid) > first + a.seg_len) nvalid = int(first + a.seg_len);
    }

    if constexpr (SEG) {
        if (a.seg_final) {
            // the launch behind the search: ONE slot re-evaluates the published first hit exactly (the same code at the same
            // trial: the same numbers), finalizes it and re-arms the word for the next search
            int win = 0x7fffffff;
            if (unit == 0) win = __hip_atomic_load(a.seg_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            active = unit == 0;
            P0 = (active && win != 0x7fffffff) ? win : 0;
            nvalid = (active && win != 0x7fffffff) ? win + 1 : 0;
        }
    }

    // the table G[1 .. B + cp] -> LDS once; entries -BMAX .. 0 are ZERO: alignments behind the current trial add nothing, branch-free
    for (int i = t - SG::BMAX; i <= QM * T; i += T) Gl[i] = i > 0 ? a.scan_g[i] : cf{0.f, 0.f};

    // Every iteration evaluates ONE trial exactly (the anchor at P0) and then screens the trials after it; the first flagged
    // trial becomes the next anchor, so "verification" and "anchor" are the same code.  The accepted trial is always the most
    // recent anchor: with one frame per workgroup its registers are used in place.
    bool found = false;
    cf Zs[P];
    cf zdups = cf{0.f, 0.f};
    float pests = 0.f, ms = 0.f;
    int dhats = 0, Phit = 0;
    if constexpr (SLOTS > 1) {
#pragma unroll
        for (int s_ = 0; s_ < P; ++s_) Zs[s_] = cf{0.f, 0.f};
    }
    // Screening margin.  A trial is handed to the exact evaluation when its screened peak exceeds (1 - 2e-4) * gate * MM.  What the
    // margin has to cover is the fp32 drift of the recurrence over one block -- at most 256 steps of one rounding each, 1.5e-5 of
    // the peak if every rounding went the same way -- and the 1e-6 of the sliding energy sums: 2e-4 is ten times that.  (Round 2
    // used 1e-3: the correlation climbs by about MM/N per trial as the window slides into the sync symbol, so a band of 1e-3 *
    // gate * MM was ~1.4 trials wide and most frames paid an anchor for a trial that the exact evaluation then turned down.)
    const float gate_s = rx.gate_mm * (1.f - 2e-4f);
    const float thr_k = gate_s * gate_s / float(rx.MM);                // |u|^2 > thr_k * E  <=>  p_est |u| > gate_s

#ifdef OFDM_EXPERIMENTS
    unsigned acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory");
#define SCAN_STAMP(i)                                                              \
    do {                                                                           \
        unsigned long long tn_;                                                    \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tn_)::"memory"); \
        acc[i] += unsigned(tn_ - tprev);                                           \
        tprev = tn_;                                                               \
    } while (0)
#else
#define SCAN_STAMP(i) do { } while (0)
#endif
    {
    for (;;) {
        bool blk_on = !found && P0 < nvalid;
        if constexpr (SEG) {
            // A hit published by an earlier segment ends this one: nothing at or after P0 can be the first accepted trial.  Every
            // thread reads the word itself.  Where one segment spans the whole workgroup (SLOTS == 1) its waves may see different
            // values, so they vote: ANY wave that saw the earlier hit stops the segment (the word only ever decreases) and blk_on
            // is workgroup-uniform as the anchor trial below assumes.  Where a workgroup holds several segments (SLOTS > 1) a
            // segment lies inside one wave, whose lanes read the word in one instruction: uniform per segment without a vote.
            const bool stop = !a.seg_final && __hip_atomic_load(a.seg_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < P0;
            if constexpr (SLOTS == 1) {
                if (__syncthreads_or(stop ? 1 : 0)) blk_on = false;
            } else if (stop) {
                blk_on = false;
            }
        }
        if (!__syncthreads_or(blk_on ? 1 : 0)) break;
        SCAN_STAMP(0);
        // ---- (1) anchor: exact trial at P0
        cf ux[SG::KX];                                                   // lags a = t + T*q, q < KX (the recurrence uses the first QM)
        cf (&u)[QM] = *reinterpret_cast<cf(*)[QM]>(&ux[0]);
        float e0;
        if constexpr (SLOTS == 1) {
            sync_trial<N, decltype(tw), SG::KX>(rx, frame_iq, a.frame_len, blk_on, P0, lds, red, tw, w1tab, t, Zs, zdups, pests, ms, dhats,
                                                ysc, nullptr, 0, ux, &e0);
            if (ms > rx.gate_mm) {                                                      // :166 (blk_on is workgroup-uniform here)
                found = true;
                Phit = P0;
                break;
            }
        } else {
            cf Z[P];
            cf zdup;
            float p_est, m;
            int dhat;
            sync_trial<N, decltype(tw), SG::KX>(rx, frame_iq, a.frame_len, blk_on, P0, lds, red, tw, w1tab, t, Z, zdup, p_est, m, dhat, ysc,
                                                nullptr, 0, ux, &e0);
            if (blk_on && m > rx.gate_mm) {                                             // :166
                found = true;
                Phit = P0;
#pragma unroll
                for (int s_ = 0; s_ < P; ++s_) Zs[s_] = Z[s_];
                zdups = zdup;
                pests = p_est;
                ms = m;
                dhats = dhat;
            }
        }
        const cf y0 = cf{red[16], red[17]}, yh = cf{red[18], red[19]};
        SCAN_STAMP(1);                                                       // .. anchor trial
        // ---- (2) screen the trials P0+1 .. P0+nb-1 with the recurrence
        int nb = (blk_on && !found) ? min(B, nvalid - P0) : 0;            // trials of this block (incl. the anchor)
        int nbx = (blk_on && !found) ? min(SG::MX * B, nvalid - P0) : 0;   // ... of the long block the cold test looks over
        int cand = 0x7fffffff;
        bool long_ok = false;
        float ucold = 3.0e38f;
        if (__syncthreads_or(nb > 1 ? 1 : 0)) {
            if constexpr (SG::MX > 1) {
                // How far ahead is the long block worth looking?  From far away the sync symbol already shows in the anchor's lag
                // vector at the alignments that will see it whole (the cp + 1 lags before its own): the long block ends where the
                // first lag at half the anchor's own threshold would come within reach (a <= n - 1 + cp), so that the cold test
                // below has a chance over all of it.  Only the amount of work depends on this guess, never a decision.
                float ah = 3.0e38f, um = 0.f;                           // um: the largest lag magnitude^2 BELOW that level
                const float half2 = 0.25f * thr_k * e0;
#pragma unroll
                for (int q = 0; q < SG::KX; ++q) {
                    const float m2 = cnorm2(ux[q]);
                    if (!(m2 < half2))
                        ah = fminf(ah, float(t + T * q));
                    else
                        um = fmaxf(um, m2);
                }
                ah = wave_min(ah);
                um = -wave_min(-um);
                if ((t & 63) == 0) {
                    blk[16 + (t >> 6)] = ah;
                    blk[(t >> 6) * 4] = um;
                }
                wg_barrier();
                um = 0.f;
#pragma unroll
                for (int w = 0; w < (T + 63) / 64; ++w) {
                    ah = fminf(ah, blk[16 + w]);
                    um = fmaxf(um, blk[w * 4]);
                }
                const int a_first = ah < 1.0e9f ? int(ah) : 0x3fffffff;
                long_ok = a_first - cp >= nb;                            // the first hot lag lies outside the long block's reach
                nbx = max(nb, min(nbx, a_first - cp));
                ucold = sqrtf(um) * (1.f + 1e-5f);                      // no lag the long block can reach starts above this
                wg_barrier();                                            // blk[] is read by everyone before it is rewritten below
            }
            // window edges: xo[i] = x[w0 + i], xn[i] = x[w0 + N + i], w0 = P0 + cp;  i < nbx - 1
            const int64_t w0 = int64_t(P0) + cp;
            float dw = 0.f, wadd = 0.f, dlane = 0.f;
            cf da = cf{0.f, 0.f}, db = cf{0.f, 0.f};
#pragma unroll
            for (int r = 0; r < SG::RMAX; ++r) {
                const int i = t * SG::RMAX + r;                          // contiguous chunk per lane
                if (i < nbx - 1) {
                    const cf o = frame_iq[w0 + i], n_ = frame_iq[w0 + N + i];
                    xo[i] = o;
                    xn[i] = n_;
                    const float sgn = (i & 1) ? 1.f : -1.f;             // (-1)^(i+1)
                    dw += cnorm2(n_) - cnorm2(o);
                    wadd += cnorm2(n_);
                    da = da + (n_ - o);
                    db = db + cscale(o - n_, sgn);
                    dlane += sqrtf(cnorm2(n_ - o));
                }
            }
            SCAN_STAMP(2);                                                   // .. window-edge loads
            // inclusive scan of the per-lane totals over the T lanes of the slot (T <= 64: inside one wave; else via LDS)
            float sw = dw, swa = wadd, sd = dlane;
            cf sa = da, sb = db;
            constexpr int W = T < 64 ? T : 64;
            constexpr bool PREFIX_D = SLOTS == 1 && SG::MX > 1;          // the |D| prefix feeds the long block's cold test only
#pragma unroll
            for (int dlt = 1; dlt < W; dlt <<= 1) {
                const float o1 = __shfl_up(sw, dlt, W), o2 = __shfl_up(swa, dlt, W);
                const float o3 = __shfl_up(sa.x, dlt, W), o4 = __shfl_up(sa.y, dlt, W);
                const float o5 = __shfl_up(sb.x, dlt, W), o6 = __shfl_up(sb.y, dlt, W);
                float o7 = 0.f;
                if constexpr (PREFIX_D) o7 = __shfl_up(sd, dlt, W);
                if ((t & (W - 1)) >= dlt) {
                    sw += o1;
                    swa += o2;
                    sa = sa + cf{o3, o4};
                    sb = sb + cf{o5, o6};
                    sd += o7;
                }
            }
            float tot_add;
            if constexpr (T > 64) {
                constexpr int NW = T / 64;
                if ((t & 63) == 63) {
                    float* r6 = red + (t >> 6) * 6;                      // NW <= 4 waves x 6 floats = the 24-dword scratch
                    r6[0] = sw;
                    r6[1] = swa;
                    r6[2] = sa.x;
                    r6[3] = sa.y;
                    r6[4] = sb.x;
                    r6[5] = sb.y;
                    if constexpr (PREFIX_D) blk[(t >> 6) * 4 + 1] = sd;  // (the wave's |D| total: next to the scratch, not in it)
                }
                wg_barrier();
                tot_add = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const float* r6 = red + w * 6;
                    tot_add += r6[1];
                    if (w < (t >> 6)) {
                        sw += r6[0];
                        sa = sa + cf{r6[2], r6[3]};
                        sb = sb + cf{r6[4], r6[5]};
                        if constexpr (PREFIX_D) sd += blk[w * 4 + 1];
                    }
                }
            } else {
                tot_add = __shfl(swa, W - 1, W);
            }
            // exclusive prefix of this lane's chunk
            float pw = sw - dw;
            cf pa = sa - da, pb = sb - db;
            // anchor: E_0 = e0 (in band), N W_0 = e0 + |Y[0]|^2 + |Y[N/2]|^2, sum x = Y[0], sum (-1)^n x = Y[N/2]
            const float nw0 = e0 + cnorm2(y0) + cnorm2(yh);
            const float wbound = nw0 + float(N) * tot_add;               // >= N W_j for every j of the block
            // this lane's share of {min_j thr_j, sum_i |D_i|} of the first block, and the first trial of the long block that its
            // own margin does not keep cold (below)
            float my_tminb = 3.0e38f, my_dabsb = 0.f;
            float sdrun = sd - dlane;                                    // sum of |D_i| before this lane's chunk
            int my_fail = 0x7fffffff;
#pragma unroll
            for (int r = 0; r < SG::RMAX; ++r) {
                const int i = t * SG::RMAX + r;
                if (i < nbx - 1) {
                    const cf o = xo[i], n_ = xn[i];
                    const float sgn = (i & 1) ? 1.f : -1.f;
                    pw += cnorm2(n_) - cnorm2(o);
                    pa = pa + (n_ - o);
                    pb = pb + cscale(o - n_, sgn);
                    // state AFTER step i, i.e. of trial j = i + 1
                    const float nwj = nw0 + float(N) * pw;
                    const float ej = nwj - cnorm2(y0 + pa) - cnorm2(yh + pb);
                    // too little energy left for the sliding sums to be trusted -> force an exact evaluation
                    const bool weak = !(nwj > 1e-4f * wbound) || !(ej > 1e-3f * nwj);
                    const float th_ = weak ? -1.f : thr_k * ej;
                    thr[i + 1] = th_;
                    xo[i] = n_ - o;                                      // dl[i] (this lane's own entry)
                    const float dm = sqrtf(cnorm2(n_ - o));
                    if (i < nb - 1) {
                        my_tminb = fminf(my_tminb, th_);
                        my_dabsb += dm;
                    }
                    if constexpr (PREFIX_D) {
                        // trial j = i + 1 stays cold if sqrt(thr_j) - max|G| * sum_{i' <= i} |D_i'| still clears every lag it can see
                        sdrun += dm;
                        const float margin = sqrtf(fmaxf(th_, 0.f)) - sdrun * gmax * (1.f + 1e-4f);
                        if ((!(th_ > 0.f) || !(margin > ucold)) && my_fail == 0x7fffffff) my_fail = i + 1;
                    }
                }
            }
            if constexpr (SLOTS == 1) {
                my_tminb = wave_min(my_tminb);
                my_dabsb = wave_sum(my_dabsb);
                const float ff = wave_min(float(min(my_fail, 1 << 24)));      // (exact in a float)
                if ((t & 63) == 0) {
                    float* b4 = blk + (t >> 6) * 4;
                    b4[0] = ff;
                    b4[2] = my_tminb;
                    b4[3] = my_dabsb;
                }
            }
            // Cold blocks.  c_{P0+j}[d] = c_{P0}[d + j] + sum_{i<j} D_i G[.] exactly, so at trial j no correlation value can lie
            // above |u_a(0)| + max|G| * sum_{i<j} |D_i|.  Where that stays below the trial's threshold for every alignment in
            // reach, the trial cannot be flagged -- let alone accepted: the thresholds sit 2e-4 below the gate -- and needs no
            // recurrence.  Over the long block (up to MX * B trials, ending before the first lag at half the anchor's threshold
            // comes within reach) this is decided TRIAL BY TRIAL with the running sum of |D| and the trial's own threshold against
            // the largest lag below that level: the trials before the first one that fails are skipped, however many they are (the
            // running sum eats the margin after ~500 trials at 2048-pt; testing whole blocks against their lowest threshold and
            // their total sum, as the first version did, skipped 240 where this skips 480-550: profiles/r03_sync_leads.txt).  If
            // that does not reach past the first block, the first block alone is tested by its totals against every lag it can
            // see.  Weak-energy trials (thr < 0) and blocks near the sync fail both and take the screened recurrence below.
            bool run_block = true;
            if constexpr (SLOTS == 1) {
                wg_barrier();                                            // blk[] and the thresholds are written
                auto cold = [&](int n_tr) {                              // the first block, by its totals
                    float tmin_b = 3.0e38f, dtot = 0.f;
#pragma unroll
                    for (int w = 0; w < (T + 63) / 64; ++w) {
                        tmin_b = fminf(tmin_b, blk[w * 4 + 2]);
                        dtot += blk[w * 4 + 3];
                    }
                    const float room = sqrtf(fmaxf(tmin_b, 0.f)) - dtot * gmax * (1.f + 1e-5f);
                    bool hot = !(tmin_b > 0.f) || !(room > 0.f);
                    const float lim2 = room * room * (1.f - 1e-5f);
#pragma unroll
                    for (int q = 0; q < SG::KX; ++q) hot |= (t + T * q <= n_tr - 1 + cp) && !(cnorm2(ux[q]) < lim2);
                    return __syncthreads_or(hot ? 1 : 0) == 0;
                };
                int n_cold = 0;                                          // trials 1 .. n_cold - 1 of the long block are proven cold
                if constexpr (SG::MX > 1) {
                    if (long_ok && nbx > nb) {
                        float ff = 3.0e38f;
#pragma unroll
                        for (int w = 0; w < (T + 63) / 64; ++w) ff = fminf(ff, blk[w * 4]);
                        n_cold = min(int(ff), nbx);
                    }
                }
                if (n_cold > nb) {
                    nb = n_cold;                                         // skip them all; the next anchor is the first trial not proven
                    run_block = false;
                } else if (cold(nb)) {
                    run_block = false;
                }
            }
            if (run_block) {
                // padding read by the unrolled loop past the block's last step: adds nothing, never flags
                for (int idx = t; idx < SG::BMAX + 2 * SG::UNR; idx += T) {
                    if (idx >= nb - 1) xo[idx] = cf{0.f, 0.f};
                    if (idx >= nb) thr[idx] = 3.0e38f;
                }
                if (t == 0) *cflag = 0x7fffffff;
                wg_barrier();
            }
            if (run_block) {
            // Checkpoints.  Window c = steps c CK + 1 .. (c+1) CK.  One step changes a correlation value by D_j G[.], at most
            // |D_j| max|G|, so no value can pass its threshold inside the window unless it starts the window within
            // sum |D| max|G| of the window's lowest threshold: |u|^2 > tchk[c] = (sqrt(min thr) - sum|D| max|G|)^2 is tested
            // once per window and only windows that pass it run the per-step tests (tchk < 0: always).
            if constexpr (T >= SG::CK) {
                // one (threshold, |D|) entry per lane, reduced over the CK lanes of a window
                for (int e0 = 0; e0 < SG::NCHK * SG::CK; e0 += T) {
                    const int e = e0 + t;
                    const bool in = e + 1 < SG::BMAX + 2 * SG::UNR;
                    float lo = in ? thr[e + 1] : 3.0e38f;
                    float dsum = in ? sqrtf(cnorm2(xo[e])) : 0.f;
#pragma unroll
                    for (int m = SG::CK >> 1; m >= 1; m >>= 1) {
                        lo = fminf(lo, __shfl_xor(lo, m, SG::CK));
                        dsum += __shfl_xor(dsum, m, SG::CK);
                    }
                    const float s_ = sqrtf(fmaxf(lo, 0.f)) - dsum * gmax;
                    if ((e & (SG::CK - 1)) == 0 && e < SG::NCHK * SG::CK) tchk[e / SG::CK] = (lo > 0.f && s_ > 0.f) ? s_ * s_ : -1.f;
                }
            } else {
                for (int c = t; c < SG::NCHK; c += T) {
                    float lo = 3.0e38f, dsum = 0.f;
#pragma unroll
                    for (int i = 0; i < SG::CK; ++i) {
                        const int j = c * SG::CK + 1 + i;
                        if (j < SG::BMAX + 2 * SG::UNR) {
                            lo = fminf(lo, thr[j]);
                            dsum += sqrtf(cnorm2(xo[j - 1]));
                        }
                    }
                    const float s_ = sqrtf(fmaxf(lo, 0.f)) - dsum * gmax;
                    tchk[c] = (lo > 0.f && s_ > 0.f) ? s_ * s_ : -1.f;
                }
            }
            wg_barrier();
            SCAN_STAMP(3);                                                   // .. prefix scan + thresholds
            // ---- recurrence over the steps j = 1 .. nb-1, UNR steps per iteration with all their LDS reads issued up front.
            // No barrier inside: lanes leave the loop on their own (first flagged trial, or the end of their frame's block).
            // The first flagged trial is published in LDS (cflag) and every lane of the frame stops there: without that, only
            // the lane that owns the flagged alignment would leave and its wave would still run to the end of the block.
            {
                const cf* dl = xo;
                cf dA[SG::UNR], gA[SG::UNR][QM], dB[SG::UNR], gB[SG::UNR][QM];
                float tA[SG::UNR], tB[SG::UNR];
                const cf* gbase = Gl + t + 1;                            // G index of alignment t + T*q at trial j: (t + 1 - j) + T*q
                auto fetch = [&](int j, cf (&dd)[SG::UNR], float (&th)[SG::UNR], cf (&gg)[SG::UNR][QM]) {
#pragma unroll
                    for (int s_ = 0; s_ < SG::UNR; ++s_) {
                        dd[s_] = dl[j + s_ - 1];
                        th[s_] = thr[j + s_];
#pragma unroll
                        for (int q = 0; q < QM; ++q) gg[s_][q] = gbase[T * q - (j + s_)];   // index >= -BMAX: zeros below 1
                    }
                };
                auto step = [&](int j, const cf (&dd)[SG::UNR], const float (&th)[SG::UNR], const cf (&gg)[SG::UNR][QM]) {
                    int first = SG::UNR;
#pragma unroll
                    for (int s_ = 0; s_ < SG::UNR; ++s_) {
                        bool h = false;
#pragma unroll
                        for (int q = 0; q < QM; ++q) {
                            cfma(u[q], dd[s_], gg[s_][q]);
                            h |= (unsigned(t + T * q - (j + s_)) <= unsigned(cp)) && (cnorm2(u[q]) > th[s_]);
                        }
                        if (h && first == SG::UNR) first = s_;
                    }
                    if (first < SG::UNR) {
                        cand = j + first;
                        atomicMin(cflag, cand);
                    }
                };
                auto advance = [&](const cf (&dd)[SG::UNR], const cf (&gg)[SG::UNR][QM]) {   // the recurrence alone
#pragma unroll
                    for (int s_ = 0; s_ < SG::UNR; ++s_) {
#pragma unroll
                        for (int q = 0; q < QM; ++q) cfma(u[q], dd[s_], gg[s_][q]);
                    }
                };
                int j = 1;
                int lim = nb;
                bool tests = true;                                       // per-step threshold tests in this window (wave-uniform)
                if (j < lim) fetch(j, dA, tA, gA);
                while (j < lim) {
                    if (((j - 1) & (SG::CK - 1)) == 0) {
                        const float tc = tchk[(j - 1) / SG::CK];
                        bool h = false;
#pragma unroll
                        for (int q = 0; q < QM; ++q)
                            h |= (unsigned(t + T * q - j) <= unsigned(cp + SG::CK - 1)) && (cnorm2(u[q]) > tc);
                        tests = __builtin_amdgcn_ballot_w64(h) != 0;
                    }
                    fetch(j + SG::UNR, dB, tB, gB);                      // reads past the block's end hit the padding
                    const int seen = *cflag;
                    if (tests) step(j, dA, tA, gA); else advance(dA, gA);
                    j += SG::UNR;
                    lim = min(lim, seen);
                    if (cand != 0x7fffffff || j >= lim) break;
                    fetch(j + SG::UNR, dA, tA, gA);
                    const int seen2 = *cflag;
                    if (tests) step(j, dB, tB, gB); else advance(dB, gB);
                    j += SG::UNR;
                    lim = min(lim, seen2);
                    if (cand != 0x7fffffff) break;
                }
            }
            SCAN_STAMP(4);                                                   // .. recurrence loop
            // first flagged trial of the slot
#pragma unroll
            for (int mk = W >> 1; mk >= 1; mk >>= 1) cand = min(cand, __shfl_xor(cand, mk, W));
            if constexpr (T > 64) {
                wg_barrier();                                            // red[] above has been read by everyone
                if ((t & 63) == 0) redi[t >> 6] = cand;
                wg_barrier();
                int c2 = redi[0];
#pragma unroll
                for (int w = 1; w < T / 64; ++w) c2 = min(c2, redi[w]);
                cand = c2;
                wg_barrier();
            }
            }   // run_block
        }
        // the first flagged trial is the next anchor (evaluated exactly there); an unflagged block is skipped whole
        if (nb > 0) P0 += (cand < nb) ? cand : nb;
        SCAN_STAMP(5);                                                       // .. candidate reduction
    }
    }
    if constexpr (SEG) {
        if (!a.seg_final) {
            // publish and leave: the finalize launch behind the search picks the overall minimum up
            if (t == 0 && active && found) atomicMin(a.seg_state, Phit);
            return;
        }
        if (tid == 0) {
            if (a.seg_final == 2) {
                __hip_atomic_store(a.seg_state + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // finalized; word 0 stays:
            } else {                                                                                   // it stops the later stages
                __hip_atomic_store(a.seg_state, 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
                __hip_atomic_store(a.seg_state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    SCAN_STAMP(6);
    sync_finalize<N>(rx, a, frame, active, found, Phit, Zs, zdups, pests, ms, dhats, lds, tw, w1tab, t, ysc);
#ifdef OFDM_EXPERIMENTS
    SCAN_STAMP(7);                                                           // .. finalize
    if (a.stamps && tid == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a.stamps[int64_t(blockIdx.x) * 8 + i] = acc[i];
    }
#endif
#undef SCAN_STAMP
}

// ------------------------------------------------------------------------------------------ launchers
template <int N>
static int scan_block_n(const RxDev& rx) {
    using SG = ScanGeom<N>;
    if (rx.S != 1 || rx.stride != 1 || rx.Ks != N - 2) return 0;
    int B = SG::QM * SG::T - rx.cp;
    if (B > SG::BMAX) B = SG::BMAX;
    return B >= 16 ? B : 0;
}

// The screened search of launch_rx_sync (mode 0 with a.scan_block > 0, grid > 0 workgroups of whole frames): the frames of a batch,
// or the staged segments of one long buffer.
template <int N>
static hipError_t launch_sync_scan_n(const RxDev& rx, const SyncArgs& a, unsigned grid, hipStream_t s) {
    if (a.scan_block != scan_block_n<N>(rx) || !a.scan_g || a.rot || a.force_accept || a.host_valid || a.off_delta || a.force_dhat_p1 ||
        a.p_begin < 0)
        return hipErrorInvalidValue;
    // register budget: 168 VGPRs (3 waves per SIMD) costs ~23 spills for one frame per workgroup (N >= 1024); the packed small
    // sizes keep a second copy of Z and get 256
    if (a.n_seg > 0) {
        if (a.n_frames != 1 || a.seg_len <= 0 || !a.seg_state) return hipErrorInvalidValue;
        // Staged: every workgroup resident when the launch starts runs its anchor before the first hit can be published, so
        // one launch over a 240-symbol buffer (~2000 segments) cost ~0.12 ms for a sync that sits in segment ~25.  The first
        // SYNC_STAGE_SEGS segments go first; the rest are launched behind them and, when the hit is already published,
        // only take their tickets.  Same decisions: the tickets and the published minimum span both launches.
        if (a.seg_base < 0 || a.seg_launch < 0 || a.seg_base % Plan<N>::SLOTS) return hipErrorInvalidValue;
        if constexpr (ScanGeom<N>::BYTES > 65536) {
            static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(&rx_sync_scan_kernel<N, OFDM_SCAN_MINW, true>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, int(ScanGeom<N>::BYTES));
            if (once != hipSuccess) return once;
        }
        SyncArgs st = a;
        int base = a.seg_base;
        const int end = a.seg_launch > 0 ? std::min(a.n_seg, a.seg_base + a.seg_launch) : a.n_seg;
        while (base < end) {
            int cnt = end - base;
            if (a.seg_launch == 0 && base == 0 && cnt > 2 * SYNC_STAGE_SEGS) cnt = SYNC_STAGE_SEGS;
            st.seg_base = base;
            st.seg_launch = cnt;
            st.seg_final = 0;
            const unsigned gseg = unsigned((int64_t(cnt) + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
            hipLaunchKernelGGL((rx_sync_scan_kernel<N, OFDM_SCAN_MINW, true>), dim3(gseg), dim3(Plan<N>::WG), ScanGeom<N>::BYTES, s, rx, st);
            base += cnt;
        }
        if (a.seg_final) {                       // 1: the search ends with this part; 2: early finalize behind a first stage
            st.seg_base = 0;
            st.seg_launch = Plan<N>::SLOTS;
            st.seg_final = a.seg_final;
            hipLaunchKernelGGL((rx_sync_scan_kernel<N, OFDM_SCAN_MINW, true>), dim3(1), dim3(Plan<N>::WG), ScanGeom<N>::BYTES, s, rx, st);
        }
        return hipGetLastError();
    }
    if constexpr (ScanGeom<N>::BYTES > 65536) {                  // (a compile-time size: announced once)
        static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(&rx_sync_scan_kernel<N, OFDM_SCAN_MINW>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(ScanGeom<N>::BYTES));
        if (once != hipSuccess) return once;
    }
    hipLaunchKernelGGL((rx_sync_scan_kernel<N, OFDM_SCAN_MINW>), dim3(grid), dim3(Plan<N>::WG), ScanGeom<N>::BYTES, s, rx, a);
    return hipGetLastError();
}

int rx_sync_scan_block(const RxDev& rx) {
#define CALL(n) scan_block_n<n>(rx)
    OFDM_DISPATCH_N(rx.nfft, CALL, 0)
#undef CALL
}

}  // namespace ofdm
