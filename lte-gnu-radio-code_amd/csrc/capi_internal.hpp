// capi_internal.hpp -- what the host-only units of the C ABI (capi_*.hip) share: the error plumbing, the four handle structs
// and the small helpers of their create / destroy / reserve / per-call paths.  Nothing in here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/ofdm_mi355x.h"
#ifdef OFDM_EXPERIMENTS
#include "../../tools/experiments/ofdm_experiments.h"
#endif
#include "ofdm_launch.hpp"

using namespace ofdm;

// ---- defined once, in capi_common.hip
#pragma GCC visibility push(hidden)
int fail(int code, const char* fmt, ...);                              // sets ofdm_last_error(), returns code
std::vector<cf> make_twiddles(int n);
std::vector<cf> make_zc(int mm, int root, int parity_of);
std::vector<cf> make_scan_table(int N, int Ks, const std::vector<cf>& zc);
int fill_rxdev(const ofdm_rx_cfg& cfg, RxDev& d);                      // derived constants; returns the Zadoff-Chu root
int upload_rx_tables(RxDev& d, cf** d_tw, cf** d_zc, const std::vector<cf>& zc);
// capi_chanavg.hip: the averaging stage of ofdm_rx_demod_frames, in place on the rows its sync launch just wrote
int chan_average_in_place(ofdm_rx* h, const cf* iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len, hipStream_t s);
// capi_rx.hip: the sync leg of ofdm_rx_demod_frames alone -- its search launch into the handle's per-frame state (the workspace
// covers n_frames)
int rx_sync_leg(ofdm_rx* h, const cf* iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len, hipStream_t s);
#pragma GCC visibility pop

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(OFDM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// DFT-spread OFDM: the plans a handle holds (capi_dft.hip).  A plan is its DftPlan and the twiddle table on the device.
struct DftPlanCache {
    static constexpr int SLOTS = 8;
    DftPlan pl[SLOTS] = {};
    cf* d_tw[SLOTS] = {};
    uint64_t used[SLOTS] = {};           // tick of the last use: the smallest one makes room
    uint64_t tick = 0;
    int n = 0;
};

// Multi-user allocations of DFT-spread OFDM (capi_dft.hip, ofdm_*_set_allocations): the set owns what its kernels read -- one
// buffer with the twiddle tables of its sizes and the descriptor table -- and does not touch the plan cache above.
struct DftAllocSet {
    int n = 0;
    int max_end = 0;                     // max(start + M)
    DftAllocDesc h[DFT_MAX_ALLOCS] = {}; // the host copy of d_set (tw: device pointers into d_tw)
    DftAllocDesc* d_set = nullptr;       // [n]
    cf* d_tw = nullptr;                  // the tables of the distinct sizes, one after the other
    int n_gap = 0;                       // runs of entries below max_end that no allocation covers, ascending
    int gap_start[DFT_MAX_ALLOCS + 1] = {}, gap_len[DFT_MAX_ALLOCS + 1] = {};
};

struct ofdm_rx {
    ofdm_rx_cfg cfg{};
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;       // stream block: the first stage of the sync search runs here, under the rest of the upload
    hipEvent_t ev_up = nullptr, ev_s1 = nullptr;
    RxDev dev{};
    cf* d_tw = nullptr;
    cf* d_zc = nullptr;
    // ---- stream block state (SynchAndChanEst.py:72,83-100)
    int count = 0;
    int corr_obs = -1;
    double tsr[3] = {0, 0, 0};
    cf* d_in = nullptr;
    int64_t in_cap = 0;
    cf* d_edf = nullptr;                 // est_data_freq [num_ofdm_symb][Kd]
    cf* d_pack = nullptr;                // the same rows without the deleted ones (:249-255), one contiguous copy to the host
    int* pin_tsr = nullptr;              // [4] pinned host copy of s_tsr, written by the search kernel itself (tsr_host)
    int* pin_tsr_dev = nullptr;          //     its device address
    // GNU Radio sized buffers (a few symbols): a copy in the stream costs more than it moves (5-10 us of engine latency plus a
    // 10-20 us bubble next to the kernels), so buffers up to PIN_IN_BYTES / PIN_OUT_BYTES go through pinned host memory that the kernels read and
    // write in place over the link; the host's share is a memcpy of a few tens of KB
    // (thresholds measured: input in place pays up to ~1 MB -- a 32-symbol buffer 0.107 -> 0.098 ms -- and loses at 4 MB, 0.21 ->
    // 0.26-0.55 ms; output in place loses at 1.7 MB, 0.21 -> 0.275 ms)
    static constexpr size_t PIN_IN_BYTES = size_t(1024) << 10, PIN_OUT_BYTES = size_t(256) << 10;
    cf* pin_in = nullptr;
    cf* pin_in_dev = nullptr;
    cf* pin_out = nullptr;
    cf* pin_out_dev = nullptr;
    int* s_tsr = nullptr;                // [4]
    cf* s_H = nullptr;                   // [2][N]   rows 0 / 1 of est_chan_freq_P
    cf* s_htime = nullptr;               // [2][N]
    cf* s_esf = nullptr;                 // [2][MM]
    cf* s_eqg = nullptr;                 // [Ks]
    cf* s_gain = nullptr;                // [Kd]
    cf* s_ysc = nullptr;                 // [MM]
    float* d_trial_m = nullptr;
    int* d_trial_d = nullptr;
    static constexpr int TRIAL_CAP = 1024;
    double* d_partial = nullptr;
    // ---- batch (frame) workspace
    int64_t cap_frames = 0;
    int* f_tsr = nullptr;
    cf* f_H = nullptr;
    cf* f_gain = nullptr;
    cf* f_htime = nullptr;
    // ---- delay-window denoising of the channel estimate (ofdm_rx_set_chan_window): off while win_post == 0
    int win_pre = 0, win_post = 0;
    float* f_tail = nullptr;             // [cap_frames] tail power of the last windowed ofdm_rx_demod_frames call
    int64_t tail_frames = -1;            // frames of the last ofdm_rx_demod_frames call if the window was on in it, else -1
    // ---- channel estimate averaged over the sync symbols of a frame (ofdm_rx_set_chan_average): off while avg_n == 0
    int avg_n = 0;                       // patterns averaged (-1 = all of a frame)
    float* f_spread = nullptr;           // [cap_frames] spread of the last averaged ofdm_rx_demod_frames call
    int64_t spread_frames = -1;          // frames of the last ofdm_rx_demod_frames call if the stage was on in it, else -1
    cf* a_part_d = nullptr;              // [frames][chunks][N] chunk partials (ChanAvgArgs)
    cf* a_part_a0 = nullptr;             // [frames][N]
    float* a_part_q = nullptr;           // [frames][chunks]
    int* a_part_n = nullptr;             // [frames][chunks]
    int64_t cap_avg_frames = 0, cap_avg_items = 0;   // frames, frames * chunks
    // ---- channel tracked across the sync symbols of a frame (ofdm_rx_reserve_chan_track)
    cf* k_H = nullptr;                   // [frames][n_pat][N] a_p when the caller does not take H_pat (ChanTrackArgs)
    int64_t cap_trk_H = 0;               // rows of k_H: grown by the reserve call and by calls without H_pat only
    int* k_flag = nullptr;               // [frames][n_pat]
    int2* k_nb = nullptr;                // [frames][n_pat] {lo, hi}
    int* k_rtsr = nullptr;               // [frames][n_pat][4] row tsr of the delay-window launch
    int64_t cap_trk_rows = 0;            // frames * n_pat
    cf* k_eq = nullptr;                  // equalised rows of a call that wants bits without eq
    int64_t cap_trk_eq = 0;              // symbols
    double* f_seg_partial = nullptr;     // [n_seg][seg_slices(seg_len)] sigma partials of ofdm_demap_frames
    int64_t cap_seg_partial = 0;
    // ---- pilot tracking stage (ofdm_rx_set_pilots): K = cfg.num_data_bins occupied bins, n_pilots of them pilots
    int n_pilots = 0;
    int* p_idx = nullptr;                // [n_pilots] ascending list indices into binsP(K)
    float* p_k = nullptr;                // [n_pilots] their signed bin offsets
    uint16_t* p_src = nullptr;           // [K - n_pilots, rounded up to even] list index of the j-th data entry
    cf pilot_conj = cf{1.f, 0.f};
    float p_kbar = 0.f, p_inv_skk = 0.f;
    cf* f_usum = nullptr;                // [n_seg][rows] pilot sums of ofdm_pilot_track_frames (read by the cfo launch)
    int64_t cap_usum = 0;
    // ---- channel-state-weighted LLRs (ofdm_rx_reserve_csi)
    int64_t last_frames = 0;             // frames of the last ofdm_rx_demod_frames call: the rows of f_H ofdm_rx_csi_frames may read
    double* c_part_e = nullptr;          // [n_seg][seg_slices(rows*row_len)] noise partials
    long long* c_part_n = nullptr;       //                                   their usable counts
    int64_t cap_csi_items = 0;
    float2* c_tab = nullptr;             // [n_seg][row_len] {s_j, w_j}
    float* c_a = nullptr;                // [n_seg][row_len] |H|^2 rows of ofdm_rx_demod_frames_csi
    int64_t cap_csi_tab = 0;
    // ---- receive-diversity combining (ofdm_rx_reserve_mrc); the composite call also uses the workspace above
    float2* m_tab = nullptr;             // [n_branch*n_seg][row_len] {c, t}
    int64_t cap_mrc_tab = 0;
    double* m_sigma2 = nullptr;          // [n_branch*n_seg] estimated variances of ofdm_rx_demod_frames_mrc
    int64_t cap_mrc_units = 0;
    // ---- DFT-spread OFDM (ofdm_rx_reserve_despread)
    DftPlanCache dft{};
    float4* ds_tab = nullptr;            // [n_seg] {float(1/beta), weight, beta, usable} (DespreadArgs)
    float* ds_a = nullptr;               // [n_seg][Kd] |H|^2 rows of ofdm_rx_demod_frames_despread
    int64_t cap_ds_seg = 0;
    // ---- receive diversity for DFT-spread OFDM (ofdm_rx_reserve_mrc_despread); the plans are those above
    float2* md_tab = nullptr;            // [n_branch*n_seg][M] {c, t} (mrc_table_kernel)
    int64_t cap_md_tab = 0;
    float* md_a = nullptr;               // [n_branch*n_frames][Kd] |H|^2 rows of ofdm_rx_demod_frames_mrc_despread
    int64_t cap_md_units = 0;
    // ---- multi-user allocations of DFT-spread OFDM (ofdm_rx_set_allocations, ofdm_rx_reserve_despread_alloc)
    DftAllocSet alloc{};
    float4* da_tab = nullptr;            // [n_alloc][n_seg] {float(1/beta), weight, beta, usable}
    int64_t cap_da_tab = 0;              // entries
    float* da_a = nullptr;               // [n_seg][Kd] |H|^2 rows of ofdm_rx_demod_frames_despread_alloc
    int64_t cap_da_seg = 0;
    // ---- receive diversity for multi-user allocations (ofdm_rx_reserve_mrc_despread_alloc); the set is the one above
    float2* ma_tab = nullptr;            // [n_branch*n_seg][row_len] {c, t} over the whole rows (mrc_table_kernel)
    int64_t cap_ma_tab = 0;              // entries
    float* ma_a = nullptr;               // [n_branch*n_frames][Kd] |H|^2 rows of ofdm_rx_demod_frames_mrc_despread_alloc
    int64_t cap_ma_a = 0;                // floats
    // ---- turbo decoder workspace (ofdm_rx_reserve_turbo): extrinsic values [n_blocks][K], then the forward checkpoints;
    // ofdm_rx_reserve_turbo_es: a second [n_blocks][K] array (post) between the two.  One buffer, laid out per call.
    float* t_ws = nullptr;
    int64_t cap_turbo = 0;               // floats
    // ---- transport-block layer (ofdm_rx_reserve_tb): the decoder's packed bits, dense [n_tb][count][K / 8] per K
    uint8_t* tb_ws = nullptr;
    int64_t cap_tb = 0;                  // bytes
    int max_trials = 0;
    int scan_block = 0;                  // > 0: the batch path's sync search is screened in blocks of this many trials
    cf* d_scan_g = nullptr;              // [N + 2] recurrence kernel G, then {max |G|, 0}
    int* d_seg_state = nullptr;          // [2] {first hit, segments done} of the stream block's segment-parallel search
    unsigned* d_work = nullptr;          // [2] work queue of the batch demod launch {next chunk, workgroups done}
    bool use_queue = true;
    bool seg_armed = false;              // the kernel re-arms the two words itself; false after a launch that did not complete
    int variant = 0;
    unsigned* d_stamps = nullptr;
    bool profiling = false;
    static constexpr int PROF_RING = 32;       // per-call event triples: no host sync inside a timed loop
    hipEvent_t ev[3 * PROF_RING] = {};
    int64_t prof_calls = 0;
};

struct ofdm_fo {
    ofdm_fo_cfg cfg{};
    hipStream_t stream = nullptr;
    RxDev dev{};
    cf* d_tw = nullptr;
    cf* d_zc = nullptr;
    cf* d_rot = nullptr;                 // [n_fo][N]  self.cfo (SynchEstAndFO.py:192)
    // ---- block state (SynchEstAndFO.py:197-222)
    int count = 0;
    int cor_obs = -1;
    int dmax_tmp_ind = -1;
    double tsr[OFDM_FO_MAX_SYNC][3] = {};
    cf* d_in = nullptr;
    int64_t in_cap = 0;
    int* t_tsr = nullptr;                // [100][4]   device copy used by the kernels
    cf* t_H = nullptr;                   // [100][N]
    cf* t_htime = nullptr;               // [100][N]
    cf* t_esf = nullptr;                 // [100][MM]
    cf* t_gain = nullptr;                // [100][Kd]
    cf* t_edf = nullptr;                 // [100][Kd]  est_data_freq
    cf* d_code = nullptr;                // [dsss]     self.SC      (DSSS variant only)
    cf* t_edfd = nullptr;                // [100][Kd/dsss] est_data_freq_d
    int n_spread = 0;
    cf* s_eqg = nullptr;                 // [Ks]
    cf* s_ysc = nullptr;                 // [MM]
    float* d_trial_m = nullptr;          // [n_fo * TRIAL_WIN]
    int* d_trial_d = nullptr;
    static constexpr int TRIAL_WIN = 256;
    // ---- frame batch workspace (ofdm_fo_demod_frames)
    int64_t cap_frames = 0;
    int64_t cap_table = 0;               // trial-table entries
    float* b_tm = nullptr;               // [frames][n_fo][trials] max|corr|
    int* b_td = nullptr;                 //                        argmax lag
    int* b_tsr = nullptr;                // [frames][100][4] {P*stride+cp, lag, int(max), live}
    int* b_fo = nullptr;                 // [frames] dmax_tmp_ind (when the caller does not ask for it)
    cf* b_gain = nullptr;                // [frames][100][Kd]
    cf* b_edf = nullptr;                 // [frames][100][Kd] est_data_freq for the despreader (dsss > 0 only)
};

struct ofdm_trk {
    ofdm_trk_cfg cfg{};
    hipStream_t stream = nullptr;
    RxDev dev{};
    cf* d_tw = nullptr;
    cf* d_zc = nullptr;
    cf* d_in = nullptr;
    int64_t in_cap = 0;
    int64_t n_in = 0;
    int* t_tsr = nullptr;                // [rows_sync][4]
    cf* t_H = nullptr;                   // [rows_sync][N]
    cf* t_imp = nullptr;                 // [rows_sync][N]
    cf* t_esf = nullptr;                 // [rows_sync][Ks]
    cf* t_gain = nullptr;                // [rows_sync][Kd]
    cf* t_edf = nullptr;                 // [rows_data][Kd]
    cf* s_ysc = nullptr;                 // [Ks]
    float* d_trial_m = nullptr;
    int* d_trial_d = nullptr;
    static constexpr int TRIAL_CAP = 4096;
};

struct ofdm_tx {
    ofdm_tx_cfg cfg{};
    hipStream_t stream = nullptr;
    TxDev dev{};
    cf* d_tw = nullptr;
    cf* d_zc = nullptr;
    // decomposed stages
    cf* d_sync_time = nullptr;           // [S][L] the sync symbol(s) SynchDataMux inserts, synthesised once at creation
    int* d_pilots = nullptr;             // ascending list indices into binsP(Kd + n_pilots)
    int n_pilots = 0;
    cf pilot_value = cf{1.f, 0.f};
    // ---- transport-block layer (ofdm_tx_reserve_tb): the packed code blocks per group, then the groups' encoder outputs
    uint8_t* tb_ws = nullptr;
    int64_t cap_tb = 0;                  // bytes
    // ---- DFT-spread OFDM (ofdm_tx_reserve_spread): the plans, and the rows between the stages of ofdm_tx_modulate_frames_spread
    DftPlanCache dft{};
    cf* sp_sym = nullptr;                // [rows][Kd]
    cf* sp_grid = nullptr;               // [rows][nfft]
    cf* sp_time = nullptr;               // [rows][L]
    int64_t cap_sp_rows = 0;
    DftAllocSet alloc{};                 // ofdm_tx_set_allocations
};

// capi_dft.hip: frees the tables of a handle's plans (the destroys); what else the DFT-spread units share is in capi_dft.hpp
#pragma GCC visibility push(hidden)
void dft_plans_free(DftPlanCache& c);
void dft_alloc_free(DftAllocSet& a);     // capi_dft.hip: frees a handle's allocation set (the destroys)
// capi_mrc.hip, shared with the combining stages of capi_despread.hip: the branch count and what ofdm_combine_csi_frames checks
// about its arguments alone ("" = fine), and the arguments of the combiner's {c, t} table
const char* mrc_bad_branches(int32_t n_branch);
const char* mrc_bad_args(int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride, int64_t csi_stride,
                         float rho, int32_t modulation, int32_t noise_mode, const double* h_noise_var, const double* d_sigma2,
                         bool composite);
MrcArgs mrc_table_args(int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride, const float* d_csi,
                       int64_t csi_stride, float rho, int32_t modulation, const double* h_noise_var, const double* d_sigma2, float2* tab);
#pragma GCC visibility pop

namespace {

template <class H>
hipStream_t pick_stream(const H* h, void* stream) { return stream ? static_cast<hipStream_t>(stream) : h->stream; }

// a create that failed half way: destroy what exists, keep the text of the failure
template <class H>
int create_failed(H* h, int rc, int (*destroy)(H*)) {
    const std::string keep = ofdm_last_error();
    destroy(h);
    return fail(rc, "%s", keep.c_str());
}

template <class T>
int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) return OFDM_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return fail(OFDM_ERR_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
    return OFDM_OK;
}

// allocate-and-clear / allocate-and-copy: every size is written once.  `what` is the text of a failed fill; it is given the
// runtime's error string.
constexpr const char* INIT_FAILED = "device table initialisation failed: %s";
template <class T>
int alloc_zeroed(T** p, size_t count, const char* what = INIT_FAILED) {
    const int rc = dev_alloc(p, count);
    if (rc != OFDM_OK || count == 0) return rc;
    const hipError_t e = hipMemset(*p, 0, count * sizeof(T));
    return e == hipSuccess ? OFDM_OK : fail(OFDM_ERR_HIP, what, hipGetErrorString(e));
}
template <class T>
int upload(T** p, const T* src, size_t count, const char* what = INIT_FAILED) {
    const int rc = dev_alloc(p, count);
    if (rc != OFDM_OK || count == 0) return rc;
    const hipError_t e = hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice);
    return e == hipSuccess ? OFDM_OK : fail(OFDM_ERR_HIP, what, hipGetErrorString(e));
}
template <class T>
int upload(T** p, const std::vector<T>& src, const char* what = INIT_FAILED) { return upload(p, src.data(), src.size(), what); }

// frees and nulls
template <class... T>
void free_dev(T**... p) { ((*p ? (void)hipFree(*p) : (void)0, *p = nullptr), ...); }

// Before buffers of a handle are freed: its device current, its stream and then the device drained (work queued on a caller's
// stream may still read them).
template <class H>
int drain(H* h) {
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipDeviceSynchronize());
    return OFDM_OK;
}

// One workspace group of a handle replaced by a larger one: drain, free every buffer, zero every capacity, allocate, set the
// capacities.  After a failed allocation every capacity of the group is 0 and every pointer null or still owned, so the next
// growth or the destroy frees it.
template <class T>
struct WsBuf {
    T** p;
    size_t count;
};
template <class T>
WsBuf<T> ws_buf(T** p, size_t count) { return {p, count}; }
struct WsCap {
    int64_t* cap;
    int64_t value;
};
template <class H, class... T>
int regrow(H* h, std::initializer_list<WsCap> caps, WsBuf<T>... bufs) {
    const int drained = drain(h);
    if (drained != OFDM_OK) return drained;
    free_dev(bufs.p...);
    for (const WsCap& c : caps) *c.cap = 0;
    int rc = OFDM_OK;
    ((rc = rc == OFDM_OK ? dev_alloc(bufs.p, bufs.count) : rc), ...);
    if (rc != OFDM_OK) return rc;
    for (const WsCap& c : caps) *c.cap = c.value;
    return OFDM_OK;
}

// a workspace that must grow cannot do so inside a stream capture (growing synchronises and allocates)
bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
int refuse_growth_in_capture(hipStream_t s, const char* who, const char* reserve_name) {
    if (stream_is_capturing(s))
        return fail(OFDM_ERR_INVALID, "%s: workspace must grow, which cannot happen inside a capture (call %s first)", who, reserve_name);
    return OFDM_OK;
}
// the tail of every ensure step: the workspace fits, or it grows through `reserve` (the call named reserve_name) -- outside a capture
template <class Reserve>
int grow_outside_capture(bool fits, hipStream_t s, const char* who, const char* reserve_name, Reserve reserve) {
    if (fits) return OFDM_OK;
    const int rc = refuse_growth_in_capture(s, who, reserve_name);
    return rc != OFDM_OK ? rc : reserve();
}

// input buffer of a stream block: grown with a quarter of headroom, after the work queued on `s` has drained
int grow_input(cf** d_in, int64_t* in_cap, int64_t n_in, hipStream_t s) {
    if (n_in <= *in_cap) return OFDM_OK;
    HIP_TRY(hipStreamSynchronize(s));
    free_dev(d_in);
    *in_cap = 0;
    const int64_t cap = n_in + n_in / 4 + 1024;
    const int rc = dev_alloc(d_in, size_t(cap));
    if (rc == OFDM_OK) *in_cap = cap;
    return rc;
}

// Trials a work() call evaluates on n_in samples: trial P iff S*L + P*stride + N + cp < n_in (SynchAndChanEst.py:144,
// SynchEstAndFO.py:249) and P < round(n_in/stride) (:139,143 / FO:246).
int64_t valid_trials(const RxDev& d, int64_t n_in) {
    const int64_t n_trials = int64_t(std::nearbyint(double(n_in) / double(d.stride)));
    const int64_t lim = n_in - (int64_t(d.S) * d.L + d.nfft + d.cp);    // P*stride < lim
    const int64_t p_valid = lim > 0 ? (lim + d.stride - 1) / d.stride : 0;
    return std::min(p_valid, n_trials);
}

// mode-1 search over one host-fed buffer: max|corr| and its lag of trials p_begin .. p_begin+cnt-1 into the trial table
SyncArgs trial_window_args(const cf* iq, int64_t n_in, int64_t p_begin, int cnt, float* trial_m, int* trial_d) {
    SyncArgs sa{};
    sa.iq = iq;
    sa.frame_stride = n_in;
    sa.frame_len = n_in;
    sa.n_frames = 1;
    sa.mode = 1;
    sa.p_begin = int(p_begin);
    sa.p_count = cnt;
    sa.trial_m = trial_m;
    sa.trial_d = trial_d;
    return sa;
}

// what ofdm_rx_demod_frames and the calls that run stages behind it check about the batch and the hard bits; "" = fine
const char* demod_bad_args(const RxDev& d, int64_t n_frames, int64_t n_dsym, const uint8_t* d_bits, int32_t bits_mode) {
    if (n_frames > INT32_MAX / 8 || n_dsym > INT32_MAX / 8) return "batch too large";
    if (d_bits) {
        if (bits_mode != OFDM_BITS_PACKED && bits_mode != OFDM_BITS_UNPACKED)
            return "bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
        if (bits_mode == OFDM_BITS_PACKED && ((d.Kd & 3) || (d.bps & 1)))
            return "packed bits need num_data_bins % 4 == 0 and an even number of bits per symbol";
    }
    return "";
}
// The opening of the calls that run stages behind ofdm_rx_demod_frames (ofdm_rx_demod_frames_*): the handle, then the batch
// arguments with the buffers the call cannot do without (`bufs`); `what` is the text of the second refusal.
int demod_stage_open(const ofdm_rx* h, bool bufs, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const char* who,
                     const char* what = "bad argument") {
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (!bufs || n_frames < 0 || frame_len < 0 || frame_stride < frame_len) return fail(OFDM_ERR_INVALID, "%s: %s", who, what);
    return OFDM_OK;
}
// data symbols of a frame of frame_len samples: whole patterns of S sync and D data symbols
int64_t frame_data_symbols(const RxDev& d, int64_t frame_len) { return frame_len / d.L / (d.S + d.D) * d.D; }

// ---- the soft-output stages (segmented soft de-mapper, pilot tracking, channel-state-weighted LLRs, combining)
// Index range of their kernels: 64-bit throughout; the bounds keep every product of them inside int64 and a row position in int.
constexpr int64_t SOFT_MAX_N = int64_t(1) << 31;      // segments (combining: units = n_branch * n_seg)
constexpr int64_t SOFT_MAX_LEN = int64_t(1) << 40;    // symbols per segment, n_seg*seg_stride and n_seg*csi_stride
constexpr int64_t SOFT_MAX_ROW = int64_t(1) << 30;    // entries per row
bool soft_mod_ok(int bits_per_symbol) { return bits_per_symbol == 2 || bits_per_symbol == 4 || bits_per_symbol == 6; }

// ---- configuration checks the creates share (each sets the error text itself)
int check_nfft(int n) {
    if (n == 64 || n == 128 || n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096) return OFDM_OK;
    return fail(OFDM_ERR_INVALID, "nfft=%d unsupported (64,128,...,4096)", n);
}
int check_bins(int nfft, int Ks, int Kd) {
    if (Ks < 2 || Ks > nfft || (Ks & 1)) return fail(OFDM_ERR_INVALID, "num_synch_bins=%d must be even and in [2, nfft]", Ks);
    if (Kd < 2 || Kd > nfft || (Kd & 1)) return fail(OFDM_ERR_INVALID, "num_data_bins=%d must be even and in [2, nfft]", Kd);
    return OFDM_OK;
}
int check_pattern(int S, int D, int num_ofdm_symb) {
    if (S < 1 || D < 1) return fail(OFDM_ERR_INVALID, "synch_dat must be [>=1, >=1]");
    if (num_ofdm_symb < 1) return fail(OFDM_ERR_INVALID, "num_ofdm_symb must be >= 1");
    return OFDM_OK;
}

// ---- what the batch calls of the codecs share (capi_tbcc.hip, capi_turbo.hip, capi_bitproc.hip, capi_tb.hip); "" = fine
constexpr int64_t MAX_BLOCKS = (int64_t(1) << 31) - 1;        // one workgroup per block: the grid's x range
constexpr int64_t MAX_ITEMS = int64_t(1) << 40;               // n_seg * seg_stride (floats) and n_seg * seg_bits
bool bits_mode_ok(int32_t m) { return m == OFDM_BITS_PACKED || m == OFDM_BITS_UNPACKED; }
bool batch_items_ok(int64_t n_seg, int64_t per_seg) { return per_seg <= MAX_ITEMS && (n_seg <= 0 || per_seg <= MAX_ITEMS / n_seg); }
// what an encode checks after its geometry: `need` coded bits per segment, `short_text` the text for a shorter segment
const char* enc_bad_args(int32_t info_mode, int32_t coded_mode, int64_t n_seg, int64_t seg_bits, int64_t need, const char* short_text) {
    if (!bits_mode_ok(info_mode) || !bits_mode_ok(coded_mode)) return "bit modes must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    if (seg_bits < 0 || seg_bits < need) return short_text;
    if (coded_mode == OFDM_BITS_PACKED && (seg_bits & 7)) return "packed coded bits need seg_bits % 8 == 0";
    if (!batch_items_ok(n_seg, seg_bits)) return "batch beyond the kernel's index range";
    return "";
}
// what a decode checks after its geometry: `need` LLRs per segment, `short_text` the text for a shorter stride
template <class Out>
const char* dec_bad_args(int64_t n_seg, int64_t seg_stride, int64_t need, const char* short_text, const Out* out) {
    if (seg_stride < need) return short_text;
    if (!batch_items_ok(n_seg, seg_stride)) return "batch beyond the kernel's index range";
    if (out && out->bits && !bits_mode_ok(out->bits_mode)) return "bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    return "";
}
// the fields every encoder's and every decoder's argument struct has
template <class Args>
void enc_fill(Args& a, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg, uint8_t* d_coded,
              int32_t coded_mode, int64_t seg_bits) {
    a.info = d_info;
    a.info_mode = info_mode;
    a.n_seg = n_seg;
    a.blocks_per_seg = blocks_per_seg;
    a.coded = d_coded;
    a.coded_mode = coded_mode;
    a.seg_bytes = coded_mode == OFDM_BITS_PACKED ? seg_bits >> 3 : seg_bits;
}
template <class Args, class Out>
void dec_fill(Args& a, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, const Out* out) {
    a.llr = d_llr;
    a.seg_stride = seg_stride;
    a.n_blocks = n_seg * blocks_per_seg;
    a.blocks_per_seg = blocks_per_seg;
    a.bits = out->bits;
    a.bits_mode = out->bits_mode;
}
// a reserve call with no workspace: it loads the code objects a first launch inside a capture would otherwise have to
template <class H>
int prepare_only(H* h, const char* who, hipError_t (*prepare)()) {
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(prepare());
    return OFDM_OK;
}

}  // namespace
