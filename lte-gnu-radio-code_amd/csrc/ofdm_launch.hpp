// ofdm_launch.hpp -- host-visible argument structs + launch wrappers of the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "ofdm_device.hpp"
#include "dft_mixed.hpp"

namespace ofdm {

// Loads the code objects of the given kernels, so that a first launch inside a stream capture has nothing left to set up (the
// *_prepare() calls below); the first error, or hipSuccess.
template <class... Kernel>
inline hipError_t load_kernels(Kernel*... kernels) {
    hipFuncAttributes fa;
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernels)) : e), ...);
    return e;
}

// ---- RX data demod (reference: SynchAndChanEst.py:221-248, "Loop B") --------------------------
struct DemodArgs {
    const cf* iq;            // frames, frame f at iq + f*frame_stride
    int64_t frame_stride;
    int64_t frame_len;       // valid samples per frame (windows past the end read zeros, like fft(x, N))
    int n_frames;
    const int* tsr;          // [n_frames][4]  {time_synch_ref[0], lag, int(max), detected}
    const cf* gain;          // [n_frames][Kd] conj(H)/(|H|^2+1/snr) * exp(j 2pi lag k/N)
    cf* eq;                  // [n_frames][rows_per_frame][Kd] or null
    uint8_t* bits;           // hard bits or null
    int bits_mode;           // ofdm_bits_mode
    int mod;                 // bits per symbol of the de-mapper (1,2,4,6)
    int n_dsym;              // data symbols visited per frame (= n_pat * D)
    int spc;                 // data symbols per chunk (one chunk = one symbol slot's loop)
    int chunks_per_frame;
    int row_stride_pat;      // output row = p*row_stride_pat + n   (S+D in stream mode, D in batch mode)
    int rows_per_frame;
    int zero_skipped;        // write zeros for patterns whose guard fails (batch mode)
    int variant;             // kernel tuning variant (0 = default)
    unsigned* stamps;        // diagnostic variant 9: [workgroups][waves][8] phase cycle sums, or null
    const cf* rot;           // per-sample rotator e^{j 2pi fo n/fs} [nfft] applied to every window (CFO receiver), or null
    int host_guard;          // 1: a frame is demodulated iff tsr[frame][3] != 0 (the host applied the reference's own guard)
    unsigned* work;          // [2] device words {next chunk, workgroups done}, both 0 between launches: work queue (batch path), or null
    int units_per_frame;     // > 0: batch CFO receiver -- launch frame u is row u % units_per_frame of IQ frame u / units_per_frame,
                             // demodulated iff tsr[u][3] != 0 (rows past a frame's syncs are written as zeros); 0 = off
    const int* rot_idx;      // with units_per_frame and rot: [IQ frames] device candidate index into rot[n_rot][nfft] per frame
};

// ---- RX sync search + LS estimate (reference: SynchAndChanEst.py:143-219, "Loop A") -----------
struct SyncArgs {
    const cf* iq;
    int64_t frame_stride;
    int64_t frame_len;
    int n_frames;
    int mode;                // 0: per-frame sequential search + finalize; 1: trial table only, units (frame, candidate, trial)
    int p_begin;
    int p_count;             // mode 0: max trials (<=0: unbounded); mode 1: number of trials in the table
    int force_accept;        // mode 0: accept trial p_begin regardless of the gate (host already decided)
    int* tsr;                // [n_frames][4]
    cf* H;                   // [n_frames][N]   est_chan_freq_P row
    const cf* H_for_gain;    // stream block, calls after the first: the data equaliser keeps using row 0 (:242); null = use H
    cf* gain;                // [n_frames][Kd]
    cf* htime;               // [n_frames][N]   est_chan_time row, or null
    cf* esf;                 // [n_frames][MM]  est_synch_freq row, or null
    cf* eqg;                 // [n_frames][Ks]  eq_gain, or null
    cf* yscratch;            // [n_frames][MM]  raw sync-bin values of the current trial (needed for esf), or null
    float* trial_m;          // mode 1: [n_frames][n_rot][p_count] max|corr| (-1 = trial not valid), candidate-major per frame
    int* trial_d;            // mode 1: [n_frames][n_rot][p_count] argmax lag
    const cf* rot;           // carrier-offset rotators [n_rot][nfft] (mode 1) / the one rotator of the finalize (mode 0), or null
    int n_rot;               // mode 1: candidates per trial (0 or 1 = plain)
    int off_delta;           // added to the window start P*stride + cp (+L*LL); 0 = the reference layout of SynchAndChanEst
    int host_valid;          // 1: the host already applied the block's own window-validity rule
    int gain_lag_set;        // 1: the data gains are de-rotated with gain_lag instead of the trial's lag (may be negative)
    int gain_lag;
    int force_dhat_p1;       // mode 0: lag+1 that replaces the trial's own arg-max lag (SynchEstAndFO.py:285,300); 0 = off
    int scan_block;          // mode 0, > 0: screened search (rx_sync_scan_kernel) with blocks of this many trials
    const cf* scan_g;        // [nfft + 2] G[m] = sum_k e^{j 2pi m k/N} conj(zc_k), G[nfft] = G[0], then {max |G|, 0}
    unsigned* stamps;        // OFDM_EXPERIMENTS build only: [workgroups][8] cycle sums per phase of the scan kernel, or null
    int keep_on_miss;        // mode 0: a frame without an accepted trial leaves every output row untouched (stream block: the old
                             // estimate stays in force, SynchAndChanEst.py:166-219 only writes on detection) except tsr[3] = 0
    int* tsr_host;           // mode 0: optional second copy of the frame's tsr words in device-visible HOST memory (stream block: the
                             // host reads them after its one synchronisation without a copy in the stream), or null
    int n_seg;               // screened search of ONE long buffer (n_frames == 1): > 0 = the trials p_begin .. are cut into n_seg
    int seg_len;             //   segments of seg_len trials searched in parallel; the first accepted trial overall is finalized
    int* seg_state;          //   [2] device words {first hit so far = INT_MAX, finalized early = 0}; the last finalize launch re-arms them
    int seg_base;            //   this launch covers the segments seg_base .. seg_base + seg_launch - 1 (seg_launch == 0: launch_rx_sync
    int seg_launch;          //   stages the search itself: the first SYNC_STAGE_SEGS segments, then the rest behind them)
    int seg_final;           //   the one-workgroup launch the launcher adds behind the search launches: 1 = the search ends here
                             //   (finalize the first hit unless an early finalize did, report a miss, re-arm seg_state); 2 = early
                             //   finalize behind a first stage the caller runs on its own (a hit there is the first hit: finalize it
                             //   and mark seg_state[1]; nothing found: leave everything to the later stages); 0 = none
};

// ---- batch CFO receiver (SynchEstAndFO.py:248-358 per frame, fresh instance): the decision the stream block takes on the host
struct FoDecideArgs {
    const float* trial_m;    // [n_frames][n_rot][p_count] trial table of rx_sync_kernel mode 1
    const int* trial_d;
    int n_frames;
    int n_rot;
    int p_count;             // trials per frame (all valid: P*stride < frame_len - (S*L + N + cp), :249)
    int rows;                // table rows per frame (OFDM_FO_MAX_SYNC)
    int err_index;           // status of a frame that reaches row `rows` (OFDM_ERR_INDEX)
    int* status;             // [n_frames] n_sync or err_index
    int* tsr_out;            // [n_frames][rows][3] {P*stride+cp, lag, int(max|corr|)}, rows >= n_sync zero, or null
    int* fo_idx;             // [n_frames] best candidate of the last trial (-1: none), or null
    int* u_tsr;              // [n_frames][rows][4] {P*stride+cp, lag, int(max|corr|), live}: the finalize / demod units
};

// Segments of the first stage of a staged segment search: a continuing stream finds its sync a few symbols into the buffer, so
// the later segments, launched behind the first stage, see the published hit and leave at once.
constexpr int SYNC_STAGE_SEGS = 64;

struct DemapArgs {
    const cf* sym;
    int64_t n;
    int mod;
    uint8_t* hard;           // n*bps bytes or null
    float* soft0;            // n*bps or null (QPSK)
    float* soft1;
    double* partial;         // [DEMAP_PARTIALS] scratch for the dmin mean
};
constexpr int DEMAP_PARTIALS = 256;

// ---- segmented soft de-mapper (ofdm_demap_frames): segment s = seg_len symbols at sym + s*seg_stride, each with its own sigma.
// A segment is cut into slices of SEG_SLICE symbols (the last one shorter); pass 1 writes one double per (segment, slice),
// pass 2 adds a segment's partials in a fixed order.  The geometry depends on seg_len only, so a segment's outputs do not depend
// on the batch it is in, on the grid or on the stream.
constexpr int SEG_SLICE = 2048;
inline int64_t seg_slices(int64_t seg_len) { return (seg_len + SEG_SLICE - 1) / SEG_SLICE; }
enum : int { SEG_OUT_SOFT0 = 1, SEG_OUT_SOFT1 = 2, SEG_OUT_LLR = 4 };
struct SegDemapArgs {
    const cf* sym;
    int64_t n_seg, seg_len, seg_stride;   // symbols
    int64_t n_slices;        // seg_slices(seg_len)
    int mod;                 // 2, 4, 6
    float* soft0;            // [n_seg][seg_len*mod] llrp0, or null
    float* soft1;            // [n_seg][seg_len*mod] llrp1, or null
    float* llr;              // [n_seg][seg_len*mod] soft0 - soft1, or null
    double* sigma;           // [n_seg], or null
    double* partial;         // [n_seg][n_slices] workspace
};

// ---- channel-state-weighted LLRs (ofdm_demap_csi_frames): segment s = rows rows of row_len symbols at sym + s*seg_stride; entry j
// of every row of segment s has the channel power csi[s*csi_stride + j].  The two divides of the contract depend on (segment, entry)
// only and live in tab[s][j] = {s_j, w_j}; the noise sum is cut into the slices of the soft de-mapper above (SEG_SLICE symbols).
struct CsiArgs {
    const cf* sym;
    int64_t n_seg, rows, seg_stride;      // complex items
    int row_len;
    int64_t seg_len;         // rows * row_len
    int64_t n_slices;        // seg_slices(seg_len)
    const float* csi;        // [n_seg][csi_stride] |H|^2 per entry
    int64_t csi_stride;
    float rho;               // 1 / SNR of the equaliser
    int mod;                 // 2, 4, 6
    int est;                 // OFDM_CSI_NOISE_EST (1) / OFDM_CSI_NOISE_GIVEN (0)
    double noise_var;        // GIVEN: sigma^2 of every segment
    float* llr;              // [n_seg][seg_len*mod], or null
    double* sigma2;          // [n_seg], or null
    long long* n_used;       // [n_seg], or null
    float2* tab;             // [n_seg][row_len] workspace {s_j (0: entry is an erasure), a_j until the noise is known, then w_j}
    double* part_e;          // [n_seg][n_slices] workspace
    long long* part_n;       // [n_seg][n_slices] workspace
};
hipError_t launch_demap_csi(const CsiArgs& a, hipStream_t s);
// a[f][j] = |H[f][bin]|^2 of the j-th entry of binsP(K) (src == null) or of its src[j]-th entry (the non-pilot entries)
hipError_t launch_csi_frames(const cf* H, int nfft, int K, const uint16_t* src, int n_out, int64_t n_frames, float* out,
                             int64_t out_stride, hipStream_t s);

// ---- receive-diversity combining (ofdm_combine_csi_frames): unit g = b*n_seg + s is branch b of output segment s, rows rows of
// row_len symbols at sym + g*seg_stride with the channel powers csi[g*csi_stride + j].  tab[g][j] = {c, t} holds the divisions that
// depend on (unit, entry) alone; the work is cut into the slices of the soft de-mapper above (SEG_SLICE output symbols).
constexpr int MRC_MAX_BRANCHES = 8;
struct MrcArgs {
    const cf* sym;
    int n_branch;
    int64_t n_seg, rows, seg_stride;      // complex items
    int row_len;
    int64_t seg_len;         // rows * row_len
    int64_t n_slices;        // seg_slices(seg_len)
    const float* csi;        // [n_branch*n_seg][csi_stride] |H|^2 per entry
    int64_t csi_stride;
    float rho;               // 1 / SNR of the equaliser
    int mod;                 // 2, 4, 6
    double noise_var[MRC_MAX_BRANCHES];   // sigma2 == null: sigma^2 of every unit of branch b
    const double* sigma2;    // [n_branch*n_seg] per unit, or null
    float* llr;              // [n_seg][seg_len*mod], or null
    cf* osym;                // [n_seg][seg_len], or null
    float* weight;           // [n_seg][seg_len], or null
    double* sigma2_out;      // [n_branch*n_seg] the variances used, or null
    float2* tab;             // [n_branch*n_seg][row_len] workspace
};
hipError_t launch_combine_mrc(const MrcArgs& a, hipStream_t s);

// ---- DFT-spread OFDM (dft_spread.hip; contract: include/ofdm_mi355x.h, "DFT-spread OFDM").  A plan (DftPlan,
// dft_mixed.hpp) and its table tw[M] = e^(-2 pi i j / M) serve both directions.  One workgroup per group of
// pl.rows_per_group consecutive rows: the grid is not capped, the callers bound the number of groups by DFT_MAX_GROUPS.
constexpr int64_t DFT_MAX_GROUPS = (int64_t(1) << 31) - 1;
hipError_t launch_dft_rows(const DftPlan& pl, const cf* tw, const cf* in, cf* out, int64_t n_rows, int inverse, hipStream_t s);
// despreading stage (ofdm_dft_despread_frames): segment s = rows rows of pl.M symbols at sym + s*seg_stride; entry k of every row
// of segment s has the channel power csi[s*csi_stride + k]
struct DespreadArgs {
    DftPlan pl;
    const cf* tw;
    const cf* sym;
    int64_t n_seg, rows, seg_stride;      // complex items
    int64_t groups_per_seg;  // ceil(rows / pl.rows_per_group)
    const float* csi;        // [n_seg][csi_stride] |H|^2 per entry, or null (plain inverse transform, beta = weight = 1)
    int64_t csi_stride;
    float rho;               // 1 / SNR of the equaliser
    int noise_mode;          // ofdm_despread_noise
    double noise_var;        // GIVEN: sigma^2 of every segment
    const double* sigma2;    // SEG: [n_seg]
    int mod;                 // 2, 4, 6 (read when llr or bits is wanted)
    int bits_mode;           // ofdm_bits_mode
    cf* osym;                // [n_seg][rows*M], or null; may be sym where seg_stride == rows*M
    float* llr;              // [n_seg][rows*M*mod], or null
    uint8_t* bits;           // hard bits of osym, or null
    float* beta;             // [n_seg], or null
    float* weight;           // [n_seg], or null
    float4* tab;             // [n_seg] workspace {float(1/beta), weight, beta, usable}
};
hipError_t launch_despread(const DespreadArgs& a, hipStream_t s);
hipError_t dft_spread_prepare();         // loads the kernels (before a stream capture)

// ---- receive diversity for DFT-spread OFDM (mrc_despread.hip; contract: include/ofdm_mi355x.h, "receive diversity for DFT-spread
// OFDM").  The {c, t} table of the combiner alone (rx_mrc.hip: a reads n_branch, n_seg, row_len, csi,
// csi_stride, rho, noise_var / sigma2, tab), then one workgroup per (output segment, group of pl.rows_per_group rows): the
// branches combined per bin into LDS, the inverse transform, the row's own weights, the epilogue of the despreading stage.
hipError_t launch_mrc_table(const MrcArgs& a, hipStream_t s);
hipError_t mrc_table_prepare();          // loads mrc_table_kernel
struct MrcDespreadArgs {
    DftPlan pl;
    const cf* tw;
    const cf* sym;           // unit g = b*n_seg + s at sym + g*seg_stride
    int n_branch;
    int64_t n_seg, rows, seg_stride;      // complex items
    int64_t groups_per_seg;  // ceil(rows / pl.rows_per_group)
    const float2* tab;       // [n_branch*n_seg][M] {c, t} of launch_mrc_table
    int mod;                 // 2, 4, 6 (read when llr or bits is wanted)
    int bits_mode;           // ofdm_bits_mode
    cf* osym;                // [n_seg][rows*M], or null
    float* llr;              // [n_seg][rows*M*mod], or null
    uint8_t* bits;           // hard bits of osym, or null
    float* beta;             // [n_seg][rows], or null
    float* weight;           // [n_seg][rows], or null
    cf* comb;                // [n_seg][rows*M] the combined symbols before the transform, or null
};
hipError_t launch_mrc_despread(const MrcDespreadArgs& a, hipStream_t s);   // the caller has checked the arguments and the grid
hipError_t mrc_despread_prepare();       // loads the kernels of both launches (before a stream capture)

// ---- multi-user allocations of DFT-spread OFDM (dft_alloc.hip; contract: include/ofdm_mi355x.h, "multi-user allocations";
// DESIGN.md 9.2.17).  An allocation set is a table of DftAllocDesc on the device, owned by the handle; a launch serves the
// allocations of one class (CAP, modulation) and finds its allocation from blockIdx.x through DftAllocClass::end.
constexpr int DFT_MAX_ALLOCS = 32;
struct DftAllocDesc {
    DftPlan pl;
    const cf* tw;            // [M], the set's own table
    int start, mod;          // first entry of the row; bits per symbol (receiver)
    int64_t sym_before;      // sum of M_v, v < u: block u of the dense outputs starts n_seg*rows*sym_before symbols in
    int64_t bit_before;      // sum of M_v*mod_v, v < u
};
struct DftAllocClass {       // by value in the kernel arguments: it depends on the call's rows and n_seg
    int n;                   // allocations of this launch
    uint8_t idx[DFT_MAX_ALLOCS];     // their places in the set
    unsigned end[DFT_MAX_ALLOCS];    // workgroups up to and including allocation k (a prefix sum of n_seg * groups)
};
struct DespreadAllocArgs {
    const DftAllocDesc* set;
    int n_alloc;
    const cf* sym;           // segment s: rows rows of row_len at sym + s*seg_stride
    int64_t n_seg, rows, row_len, seg_stride;
    const float* csi;        // [n_seg][csi_stride] |H|^2 per entry of the row, or null
    int64_t csi_stride;
    float rho;
    int noise_mode;
    double noise_var;
    const double* sigma2;    // SEG: [n_seg], shared by the allocations of a segment
    int bits_mode;
    cf* osym;                // allocation-major dense blocks, or null
    float* llr;
    uint8_t* bits;
    float* beta;             // [n_alloc][n_seg], or null
    float* weight;
    float4* tab;             // [n_alloc][n_seg] workspace {float(1/beta), weight, beta, usable}
};
// h_set: the host copy of the table (plans, modulations).  The caller has checked the arguments and every grid.
hipError_t launch_despread_alloc(const DespreadAllocArgs& a, const DftAllocDesc* h_set, hipStream_t s);
struct DftAllocRowsArgs {
    const DftAllocDesc* set;
    const cf* in;            // [n_rows][row_len]
    cf* out;                 // [n_rows][row_len], may be `in`
    int64_t n_rows, row_len;
    int n_gap;               // runs of entries outside every allocation, written as +0+0j
    int gap_start[DFT_MAX_ALLOCS + 1], gap_len[DFT_MAX_ALLOCS + 1];
    unsigned zero_groups;    // workgroups behind the class's own that write the gaps (first launch only)
};
hipError_t launch_dft_alloc_rows(DftAllocRowsArgs a, const DftAllocDesc* h_set, int n_alloc, hipStream_t s);
hipError_t dft_alloc_prepare();          // loads the kernels (before a stream capture)

// ---- receive diversity for multi-user allocations of DFT-spread OFDM (mrc_despread_alloc.hip; contract: include/ofdm_mi355x.h,
// "receive diversity for multi-user allocations of DFT-spread OFDM").  launch_mrc_table over the whole rows
// (row_len entries per unit), then one launch per class of the set; a workgroup serves (allocation, segment, group of rows).
struct MrcDespreadAllocArgs {
    const DftAllocDesc* set;
    int n_alloc;
    const cf* sym;           // unit g = b*n_seg + s: rows rows of row_len at sym + g*seg_stride
    int n_branch;
    int64_t n_seg, rows, row_len, seg_stride;     // complex items
    const float2* tab;       // [n_branch*n_seg][row_len] {c, t} of launch_mrc_table
    int bits_mode;           // ofdm_bits_mode
    cf* osym;                // allocation-major dense blocks, or null
    float* llr;
    uint8_t* bits;
    float* beta;             // [n_alloc][n_seg][rows], or null
    float* weight;
    cf* comb;                // the combined symbols before the transform, laid out as osym, or null
};
// h_set: the host copy of the table (plans, modulations).  The caller has checked the arguments and every grid, and run the table.
hipError_t launch_mrc_despread_alloc(const MrcDespreadAllocArgs& a, const DftAllocDesc* h_set, hipStream_t s);
hipError_t mrc_despread_alloc_prepare(); // loads the kernels of both launches (before a stream capture)

// ---- pilot-aided phase tracking (ofdm_pilot_track_frames): rows of K equalised symbols in binsP(K) list order -> rows of
// Kd = K - n_pilots de-rotated data symbols.  A row is owned by a group of 2^g_log2 lanes of one wave (one lane per PAIR of
// consecutive outputs and pass); a group walks rows_per_group consecutive rows, so that a workgroup's share is sized in bytes.
struct PilotArgs {
    const cf* sym;
    int64_t n_seg, rows, seg_stride;      // segment s = rows rows of K symbols at sym + s*seg_stride (complex items)
    int K, Kd, n_pilots;
    int g_log2, rows_per_group;
    int slope;               // OFDM_PILOT_CPE_SLOPE
    int mod;                 // 2, 4, 6 (only read when bits != null)
    cf pilot_conj;           // conj(pilot_value)
    const int* pidx;         // [n_pilots] ascending list indices of the pilots
    const float* pk;         // [n_pilots] their signed bin offsets
    const uint16_t* src;     // [Kd rounded up to even] list index of the j-th data entry
    float kbar, inv_skk;     // mean pilot offset, 1 / sum (k_p - kbar)^2
    cf* data;                // [n_seg][rows][Kd], or null
    uint8_t* bits;           // hard bits of data, or null
    int bits_mode;
    cf* cpe;                 // [n_seg][rows], or null
    float* slope_out;        // [n_seg][rows], or null
    cf* usum;                // [n_seg][rows] workspace: the pilot sum U of a usable row, else 0 (null: cfo not wanted)
    double* cfo;             // [n_seg], or null
    int rows_per_pattern;
    double cfo_scale;        // nfft / (2 pi L)
};
inline int pilot_group_log2(int Kd) {
    int g = 1;
    while (g < 6 && (1 << g) < (Kd + 1) / 2) ++g;
    return g;
}
// rows a lane group walks: about 4 KB of input per wave
inline int pilot_rows_per_group(int K, int g_log2) { return std::max(1, 4096 / (K * 8 * (64 >> g_log2))); }

// ---- TX (reference: MultiAntennaSystem.py:113-218) ---------------------------------------------
struct TxDev {
    int nfft, cp, L, Ks, Kd, S, D, bps;
    const cf* tw;
    const cf* zc;            // [S*Ks]
};
struct ModArgs {
    const uint8_t* bits;
    int bits_mode;
    int64_t bits_stride;     // bytes per frame in `bits`
    int n_frames;
    int n_sym;               // symbols per frame
    cf* iq;
    int64_t frame_stride;
    const cf* sync_time;     // [S][L] the finished sync symbol(s) (synthesised once per handle by the same device functions), or null
};
// decomposed TX stages
struct GridArgs {
    const cf* sym;           // [n_rows][Kd]
    int64_t n_rows;
    const int* pilots;       // [n_pilots] ascending list indices into binsP(Kd + n_pilots), or null
    int n_pilots;
    cf pilot_value;
    cf* grid;                // [n_rows][nfft]
};
struct TimeArgs {
    const cf* in;            // do_ifft: [n_rows][nfft] grid rows; else [n_rows][nfft] time samples
    int64_t n_rows;
    int do_ifft, do_cp;
    cf* out;                 // do_cp: [n_rows][L]; else [n_rows][nfft]
};
struct MuxArgs {
    const cf* sync_time;     // [S][L]
    const cf* data;          // [n_data_sym][L]
    int64_t n_out_sym;
    cf* out;                 // [n_out_sym][L]
};
struct ChanArgs {
    const cf* in;
    int64_t in_stride, in_len;
    int n_frames;
    const cf* taps;
    int n_taps;
    int per_frame_taps;
    float noise_std;         // per real component: sqrt(noise_var/2)
    uint64_t seed;
    cf* out;
    int64_t out_stride, out_len;
};

// ---- LTE tail-biting convolutional code (tbcc.hip; contract: include/ofdm_mi355x.h)
constexpr int TBCC_W = 96;               // wrap-around depth: the decoder runs T = K + 2W trellis steps
constexpr int TBCC_K_MIN = 24, TBCC_K_MAX = 2048;
inline bool tbcc_valid_k(int64_t K) { return K >= TBCC_K_MIN && K <= TBCC_K_MAX && K % 8 == 0; }
struct TbccEncArgs {
    const uint8_t* info;     // dense [n_seg][blocks_per_seg][K] bits
    int info_mode;           // ofdm_bits_mode
    int64_t n_seg;
    int blocks_per_seg, K;
    uint8_t* coded;          // [n_seg][seg_bytes]: blocks_per_seg*3K coded bits from bit 0, then zeros
    int coded_mode;          // ofdm_bits_mode
    int64_t seg_bytes;       // seg_bits (one bit per byte) or seg_bits / 8 (packed)
};
struct TbccDecArgs {
    const float* llr;        // block (seg, b) = 3K floats at llr + seg*seg_stride + b*3K
    int64_t seg_stride;      // floats
    int64_t n_blocks;        // n_seg * blocks_per_seg: one workgroup of one wave each
    int blocks_per_seg, K;
    uint8_t* bits;           // dense [n_blocks][K] bits, or null
    int bits_mode;           // ofdm_bits_mode
    float* metric;           // [n_blocks], or null
    int32_t* tb_ok;          // [n_blocks], or null
};
// Rate matching (TS 36.212 5.1.4.2): what the sub-block interleaver's closed form needs, all of it from K
constexpr int TBCC_RM_MAX_COPIES = 16;   // E <= 3K * 16
inline bool tbcc_valid_e(int64_t K, int64_t E) { return E >= 1 && E <= 3 * TBCC_RM_MAX_COPIES * K; }
struct TbccRmGeom {
    int E;                   // rate-matched bits per block
    int R, ND;               // rows of the 32-column matrix = ceil(K / 32), NULLs in front of a stream = 32R - K
    uint32_t nullmask;       // bit c set iff permuted column c starts with a NULL: P[c] < ND
};
TbccRmGeom tbcc_rm_geom(int K, int E);
struct TbccEncRmArgs : TbccEncArgs { TbccRmGeom g; };       // coded: blocks_per_seg*E bits from bit 0, then zeros
struct TbccDecRmArgs : TbccDecArgs { TbccRmGeom g; };       // llr: block (seg, b) = E floats at llr + seg*seg_stride + b*E
struct TbccDematchArgs {
    const float* llr;        // block (seg, b) = E floats at llr + seg*seg_stride + b*E
    int64_t seg_stride;      // floats
    int64_t n_blocks;        // n_seg * blocks_per_seg
    int blocks_per_seg, K;
    float* out;              // block (seg, b) = 3K floats at out + seg*out_stride + b*3K, [3i + j]: what TbccDecArgs::llr takes
    int64_t out_stride;      // floats
    TbccRmGeom g;
};
hipError_t launch_tbcc_encode(const TbccEncArgs& a, hipStream_t s);
hipError_t launch_tbcc_decode(const TbccDecArgs& a, hipStream_t s);
hipError_t launch_tbcc_encode_rm(const TbccEncRmArgs& a, hipStream_t s);
hipError_t launch_tbcc_dematch(const TbccDematchArgs& a, hipStream_t s);
hipError_t launch_tbcc_decode_rm(const TbccDecRmArgs& a, hipStream_t s);
// loads the decoders' code objects (so that a first launch inside a stream capture has nothing left to set up)
hipError_t tbcc_decode_prepare();
size_t tbcc_lds_bytes(int K);            // survivor memory of one block: 8 B per trellis step, rounded up to 32 steps

// ---- CRC and Gold-sequence scrambling (bitproc.hip; contract: include/ofdm_mi355x.h)
constexpr int GOLD_CH = 1024;            // sequence bits one lane produces after its jump
constexpr int GOLD_LEVELS = 21;          // jump tables M^(GOLD_CH * 2^k), k < 21: every bit index below 2^31
constexpr int GOLD_SPAN = 64 * GOLD_CH;  // bits of a segment one workgroup (one wave) owns
constexpr int64_t GOLD_MAX_BITS = (int64_t(1) << 31) - 1600;   // seg_bits < this: n + 1600 stays below 2^31
struct GoldArgs {
    const void* in;          // LLR: float [n_seg][in_stride]; bits: uint8 [n_seg][in_stride] (one per byte, or packed MSB-first)
    void* out;               // the same layout at out_stride; out == in (equal strides) is allowed
    int64_t in_stride, out_stride;       // elements: floats or bytes
    int64_t n_seg, seg_bits;
    const uint32_t* cinit;   // [n_seg]
};
constexpr int CRC_A_MIN = 8, CRC_A_MAX = 2040, CRC_K_MAX = 2048;
struct CrcArgs {
    int kind, A;             // ofdm_crc_kind, payload bits
    int64_t n_blocks;
    uint32_t mask;           // XORed into the parity (p0 = MSB), used when mask_dev is null
    const uint32_t* mask_dev;            // [n_blocks], or null
    int info_mode, payload_mode;         // ofdm_bits_mode
    // attach (info_out != null): payload_in dense [n_blocks][A] -> info_out dense [n_blocks][A + L]
    const uint8_t* payload_in;
    uint8_t* info_out;
    // check: info_in dense [n_blocks][A + L] -> each of the outputs that is not null
    const uint8_t* info_in;
    uint8_t* ok;             // [n_blocks]
    uint32_t* syndrome;      // [n_blocks]
    uint8_t* payload_out;    // dense [n_blocks][A]
};
hipError_t launch_gold_llr(const GoldArgs& a, hipStream_t s);
hipError_t launch_gold_bits(const GoldArgs& a, int packed, hipStream_t s);
hipError_t launch_crc(const CrcArgs& a, hipStream_t s);
hipError_t bitproc_prepare();            // loads the kernels' code objects (before a stream capture)
int crc_bits(int kind);                  // 24 / 24 / 16 / 8, 0 for an unknown kind
uint32_t crc_host(int kind, const uint8_t* bits_packed, int A);            // the kernels' remainder routine on the host
void gold_bits_host(uint32_t c_init, int64_t first, int64_t n, uint8_t* out);   // c(first ..) from the kernels' jump tables

// ---- LTE turbo code (turbo.hip; contract: include/ofdm_mi355x.h)
constexpr int TURBO_K_MIN = 40, TURBO_K_MAX = 6144;
constexpr int TURBO_ITER_MAX = 16;
constexpr int TURBO_GROUP = 8;           // code blocks per wave of the decoder: lane = (block, state)
constexpr int TURBO_CKPT = 32;           // trellis steps between two stored forward metrics (a multiple of 8, the normalisation grid)
inline bool turbo_valid_k(int64_t K) { return K >= TURBO_K_MIN && K <= TURBO_K_MAX && K % 8 == 0; }
bool turbo_qpp_valid(int64_t K, int64_t f1, int64_t f2);     // host, O(K): a valid K, 0 <= f1, f2 < K and pi a permutation
struct TurboQpp {            // pi(i) = (f1 i + f2 i^2) mod K and the increments the kernels step it with, all reduced mod K
    int K, f1, f2;
    int g2;                  // 2 f2:           (pi(i+2) - pi(i+1)) - (pi(i+1) - pi(i))
    int c8, c16, c128;       // 8 f1 + 64 f2, 16 f2, 128 f2:  pi(i+8) - pi(i) = c8 + c16 i, which grows by c128 per 8 steps
};
TurboQpp turbo_qpp(int K, int f1, int f2);
struct TurboEncArgs {
    const uint8_t* info;     // dense [n_seg][blocks_per_seg][K] bits
    int info_mode;           // ofdm_bits_mode
    int64_t n_seg;
    int blocks_per_seg;
    uint8_t* coded;          // [n_seg][seg_bytes]: blocks_per_seg*(3K+12) coded bits from bit 0, then zeros
    int coded_mode;          // ofdm_bits_mode
    int64_t seg_bytes;       // seg_bits (one bit per byte) or seg_bits / 8 (packed)
    TurboQpp q;
};
struct TurboDecArgs {
    const float* llr;        // block (seg, b) = 3K+12 floats at llr + seg*seg_stride + b*(3K+12)
    int64_t seg_stride;      // floats
    int64_t n_blocks;        // n_seg * blocks_per_seg: one wave per TURBO_GROUP of them
    int blocks_per_seg;
    int n_iter;
    float* ext;              // workspace [n_blocks][K]: the extrinsic values, at the end llr in natural order
    float* ckpt;             // workspace [waves][ceil(K / TURBO_CKPT)][64]: forward metrics at the tile starts
    uint8_t* bits;           // dense [n_blocks][K] bits, or null
    int bits_mode;           // ofdm_bits_mode
    float* llr_out;          // dense [n_blocks][K], or null
    TurboQpp q;
};
int64_t turbo_ws_floats(int64_t n_blocks, int K);            // ext + ckpt of a decode of n_blocks blocks, ext first
hipError_t launch_turbo_encode(const TurboEncArgs& a, hipStream_t s);
hipError_t launch_turbo_decode(const TurboDecArgs& a, hipStream_t s);
hipError_t turbo_decode_prepare();       // loads the decoder's code object (before a stream capture)

// ---- turbo decoder with early termination by CRC (turbo_es.hip; contract: include/ofdm_mi355x.h)
struct TurboDecEsArgs {
    const float* llr;        // as TurboDecArgs
    int64_t seg_stride;
    int64_t n_blocks;
    int blocks_per_seg;
    int min_iter, max_iter;  // 1 <= min_iter <= max_iter <= TURBO_ITER_MAX
    int crc_kind;            // ofdm_crc_kind of the stop check: zero mask, all K bits
    float* ext;              // workspace [n_blocks][K]: the extrinsic values
    float* post;             // workspace [n_blocks][K]: post of the block's latest stop-eligible iteration, natural order
    float* ckpt;             // workspace [waves][ceil(K / TURBO_CKPT)][64]
    uint8_t* bits;           // dense [n_blocks][K] bits, or null
    int bits_mode;
    float* llr_out;          // dense [n_blocks][K], or null
    uint8_t* iters;          // block (seg, b) at seg*stat_stride + b, or null
    uint8_t* crc_ok;         // likewise
    int64_t stat_stride;     // resolved (not 0)
    TurboQpp q;
};
int64_t turbo_es_ws_floats(int64_t n_blocks, int K);         // ext + post + ckpt, in this order
hipError_t launch_turbo_decode_es(const TurboDecEsArgs& a, hipStream_t s);
hipError_t turbo_decode_es_prepare();    // loads the kernel (before a stream capture)

// ---- turbo rate matching (turbo_rm.hip; TS 36.212 5.1.4.1; contract: include/ofdm_mi355x.h)
constexpr int TURBO_RM_MAX_COPIES = 16;  // E <= 16 Navail
struct TurboRmGeom {         // what the closed form of the sub-block interleavers and the circular buffer needs, all of it from K, E, Ncb
    int E;                   // rate-matched bits per block
    int D, R, ND, Kpi;       // K + 4, rows of the 32-column matrices = ceil(D / 32), NULLs in front of a stream = 32R - D, 32R
    int Ncb, navail;         // buffer length (Kpi .. 3 Kpi) and the non-NULL entries of w[0 .. Ncb)
    int rank0[4];            // per rv: the non-NULL entries of w[0 .. k0)
    uint32_t mask01, mask2;  // bit c set iff column c of v0 / v1 (P[c] < ND) resp. of v2 (P[c] < ND - 1) starts with a NULL
};
// non-NULL entries in front of (column c, row r) of a stream whose NULLs are row 0 of mask's columns; c < 32
__host__ __device__ inline int turbo_rm_stream_count(uint32_t mask, int R, int c, int r) {
    return c * R + r - __builtin_popcount(mask & ((1u << c) - 1u)) - (r > 0 ? int((mask >> c) & 1u) : 0);
}
// non-NULL entries of w[0 .. p), 0 <= p <= 3 Kpi: v0, then v1 and v2 interlaced; v2's last entry is its extra NULL
__host__ __device__ inline int turbo_rm_count(const TurboRmGeom& g, int p) {
    auto stream = [&](uint32_t mask, int k) { return k >= g.Kpi ? g.D : turbo_rm_stream_count(mask, g.R, k / g.R, k % g.R); };
    if (p <= g.Kpi) return stream(g.mask01, p);
    const int q = p - g.Kpi;
    return g.D + stream(g.mask01, (q + 1) >> 1) + stream(g.mask2, q >> 1);
}
inline int turbo_rm_kpi(int K) { return 32 * ((K + 4 + 31) / 32); }
inline int turbo_rm_k0(int K, int Ncb, int rv) {             // Ncb already resolved (not 0)
    const int R = turbo_rm_kpi(K) / 32;
    return R * (2 * ((Ncb + 8 * R - 1) / (8 * R)) * rv + 2);
}
TurboRmGeom turbo_rm_geom(int K, int E, int Ncb);            // Ncb = 0 means 3 Kpi; E is only stored
struct TurboEncRmArgs : TurboEncArgs {   // coded: blocks_per_seg*E bits from bit 0, then zeros
    TurboRmGeom g;
    int rv;                  // redundancy version of every segment, unless
    const int32_t* rv_dev;   // [n_seg] on the device (low two bits), or null
};
struct TurboDematchArgs {
    const float* llr;        // block (seg, b) = E floats at llr + seg*seg_stride + b*E
    int64_t seg_stride;      // floats
    int64_t n_blocks;        // n_seg * blocks_per_seg
    int blocks_per_seg, K;
    float* out;              // block (seg, b) = 3K+12 floats at out + seg*out_stride + b*(3K+12), [3i + j]: what TurboDecArgs::llr takes
    int64_t out_stride;      // floats
    int accumulate;          // != 0: out = old + L
    TurboRmGeom g;
    int rv;
    const int32_t* rv_dev;
};
int turbo_rm_group(int E, int coded_mode);                   // blocks per workgroup of the encoder: their bits end on a byte
hipError_t launch_turbo_encode_rm(const TurboEncRmArgs& a, hipStream_t s);
hipError_t launch_turbo_dematch(const TurboDematchArgs& a, hipStream_t s);
hipError_t turbo_rm_prepare();           // loads both kernels (before a stream capture)

// ---- transport-block layer (tb.hip; TS 36.212 5.1.1, 5.1.2, 5.1.5; contract: include/ofdm_mi355x.h)
constexpr int TB_A_MIN = 8, TB_A_MAX = (1 << 20) - 24;
constexpr int TB_THREADS = 256;          // one workgroup per transport block: the runs of its CRC24A, four waves for the code blocks
// LTE's 188 block sizes: the smallest one >= bits and the largest one below K; 0 where there is none
inline int turbo_k_next(int64_t bits) {
    if (bits <= 40) return 40;
    if (bits > TURBO_K_MAX) return 0;
    const int64_t step = bits <= 512 ? 8 : bits <= 1024 ? 16 : bits <= 2048 ? 32 : 64;
    return int((bits + step - 1) / step * step);
}
inline int turbo_k_prev(int K) { return K <= 40 ? 0 : K <= 512 ? K - 8 : K <= 1024 ? K - 16 : K <= 2048 ? K - 32 : K - 64; }
inline bool turbo_k_is_lte(int64_t K) { return K >= TURBO_K_MIN && K <= TURBO_K_MAX && turbo_k_next(K) == K; }
struct TbSeg {               // the segmentation of one transport block, in bytes (everything is a multiple of 8 bits)
    int A8, L8;              // payload bytes; 3 with a CRC24B per block, else 0
    int C, Cm;               // code blocks; the first Cm of them have Km8 bytes, the rest Kp8
    int Km8, Kp8, F8;        // F8 filler bytes in front of block 0
};
struct TbRange {             // blocks first .. first + count - 1 of every transport block: dense [n_tb][count][kbytes] packed bits at ws + base
    int first, count, kbytes;
    int64_t base;
};
struct TbSegArgs {           // tb_segment_kernel (payload_in -> ws) and tb_desegment_kernel (ws -> the outputs that are not null)
    TbSeg g;
    int n_ranges;            // <= 3, in block order, tiling 0 .. C
    TbRange range[3];
    int64_t n_tb;
    uint8_t* ws;
    int payload_mode;        // ofdm_bits_mode of payload_in / payload_out: dense [n_tb][A] or [n_tb][A/8]
    const uint8_t* payload_in;
    uint8_t* payload_out;
    uint8_t* tb_ok;          // [n_tb]
    uint8_t* cb_ok;          // [n_tb][C]
    uint32_t* syndrome;      // [n_tb]
};
struct TbConcatArgs {        // group g of every transport block: bits[g] bytes (one bit each) at ws + base[g] + t*bits[g] -> codeword bit off[g] ..
    int n_groups;
    int64_t bits[3], off[3], base[3];
    int64_t n_tb, G, cw_bits;
    const uint8_t* ws;
    uint8_t* cw;             // [n_tb][cw_bits] or [n_tb][cw_bits / 8]; zeros from G on
    int cw_mode;
};
hipError_t launch_tb_segment(const TbSegArgs& a, hipStream_t s);
hipError_t launch_tb_desegment(const TbSegArgs& a, hipStream_t s);
hipError_t launch_tb_concat(const TbConcatArgs& a, hipStream_t s);
hipError_t tb_prepare();                 // loads the three kernels (before a stream capture)
uint32_t crc_long_host(int kind, const uint8_t* bits_packed, int64_t n_bytes);   // the kernels' chunk-and-combine routine on the host

hipError_t launch_rx_demod(const RxDev& rx, const DemodArgs& a, hipStream_t s);
hipError_t launch_rx_sync(const RxDev& rx, const SyncArgs& a, hipStream_t s);
// batch CFO receiver: one wave per frame walks the trial table in order (gate, distance rule, 101st sync) -> FoDecideArgs outputs
hipError_t launch_fo_decide(const RxDev& rx, const FoDecideArgs& a, hipStream_t s);
// batch CFO receiver: LS estimate of every (frame, row) unit, a.n_frames = units, units_per_frame rows per IQ frame.  Reads
// {P*stride+cp, lag, live} from a.tsr (FoDecideArgs::u_tsr); a.rot = the LAST candidate's rotator or null; a.H may be null.
hipError_t launch_fo_finalize(const RxDev& rx, const SyncArgs& a, int units_per_frame, hipStream_t s);
// htime[r] = ifft(H[r]) for n_rows rows of nfft bins (est_chan_time on demand)
hipError_t launch_rx_chan_time(const RxDev& rx, const cf* H, cf* htime, int n_rows, hipStream_t s);
// delay-window denoising of LS channel estimates (rx_chanwin.hip): per row with tsr[3] == 1, H_out = fft(window(ifft(H_in))) on the
// sync bins, the data-bin gains of sync_finalize from it, tail = N/M * the power of the M discarded taps.  One launch,
// ceil(n_rows / SLOTS) workgroups.
struct ChanWinArgs {
    const cf* H_in;          // [n_rows][N]
    const int* tsr;          // [n_rows][4]  {., lag, ., sync found}
    int64_t n_rows;
    int pre, post;           // taps kept: [0, post) and [N - pre, N)
    cf* H_out;               // [n_rows][N]   may be H_in
    cf* gain;                // [n_rows][Kd]  or null
    float* tail;             // [n_rows]      or null
};
hipError_t launch_chan_window(const RxDev& rx, const ChanWinArgs& a, hipStream_t s);
hipError_t launch_chan_noise(const float* tail, int64_t n, double* sigma2, hipStream_t s);   // sigma2[i] = double(tail[i])
hipError_t chan_window_prepare();        // loads the kernels (before a stream capture)
// channel estimate averaged over the sync symbols of a frame (rx_chanavg.hip; contract: include/ofdm_mi355x.h, "channel estimate
// averaged over every sync symbol of a frame").  Two launches: chan_avg_kernel<N>, one work item per (frame, chunk of
// CHANAVG_CHUNK patterns), leaves one partial per item in the workspace and the rotations in rot; chan_avg_finalize_kernel adds a
// frame's partials in chunk order and writes the outputs that are not null.
constexpr int CHANAVG_CHUNK = 16;
inline int64_t chanavg_chunks(int64_t n_pat) { return (n_pat + CHANAVG_CHUNK - 1) / CHANAVG_CHUNK; }
struct ChanAvgArgs {
    const cf* iq;            // frames, frame f at iq + f*frame_stride
    int64_t frame_stride;
    int64_t frame_len;
    int64_t n_frames;
    const int* tsr;          // [n_frames][4]  {t0, lag, ., sync found}
    int n_pat;               // P: patterns considered per frame, min(n_avg, patterns of a frame)
    int n_chunks;            // chanavg_chunks(n_pat)
    cf* part_d;              // workspace [n_frames][n_chunks][N]: the chunk's sum of d_p on the sync bins
    cf* part_a0;             // workspace [n_frames][N]: a_0 on the sync bins (written by chunk 0)
    float* part_q;           // workspace [n_frames][n_chunks]: the chunk's sum of |d_p|^2
    int* part_n;             // workspace [n_frames][n_chunks]: patterns of the chunk that take part
    cf* H_out;               // [n_frames][N]      or null
    cf* gain;                // [n_frames][Kd]     or null
    float* spread;           // [n_frames]         or null
    int* n_used;             // [n_frames]         or null
    cf* rot;                 // [n_frames][n_pat]  or null
};
hipError_t launch_chan_average(const RxDev& rx, const ChanAvgArgs& a, hipStream_t s);
hipError_t launch_chan_spread(const float* spread, int64_t n, double* sigma2, hipStream_t s);   // sigma2[i] = double(spread[i])
hipError_t chan_average_prepare();       // loads the kernels (before a stream capture)
// channel tracked across the sync symbols of a frame (rx_chantrack.hip; contract: include/ofdm_mi355x.h, "channel tracked across
// the sync symbols of a frame").  launch_chan_track_est: chan_track_est_kernel<N>, one work item per (frame, pattern), writes the
// row a_p and the pattern's flag; chan_track_link_kernel, one workgroup per frame, turns the flags into the neighbours {lo, hi}
// of every pattern, the `takes` output and the row tsr of the delay window.  The caller may run launch_chan_window over the
// n_frames * n_pat rows in between.  launch_chan_track_demod: rx_demod_track_kernel<N>, one work item per (frame, run of
// CHANTRACK_RUN consecutive data symbols), then (bits != null) the hard-decision pass over the stored rows.
constexpr int CHANTRACK_RUN = 12;
inline int64_t chantrack_runs(int64_t n_dsym) { return (n_dsym + CHANTRACK_RUN - 1) / CHANTRACK_RUN; }
struct ChanTrackArgs {
    const cf* iq;            // frames, frame f at iq + f*frame_stride
    int64_t frame_stride;
    int64_t frame_len;
    int64_t n_frames;
    const int* tsr;          // [n_frames][4]  {t0, lag, ., sync found}
    int n_pat;               // patterns per frame
    int n_dsym;              // n_pat * D
    int n_runs;              // chantrack_runs(n_dsym)
    int linear;              // 1: OFDM_TRACK_LINEAR, 0: OFDM_TRACK_HOLD
    cf* H_pat;               // [n_frames][n_pat][N]: a_p (the caller's buffer or the workspace)
    int* flag;               // workspace [n_frames][n_pat]: the pattern takes part
    int2* nb;                // workspace [n_frames][n_pat]: {lo, hi or -1}
    int* row_tsr;            // workspace [n_frames][n_pat][4] {0, lag, 0, takes} for launch_chan_window, or null
    int* takes;              // [n_frames][n_pat] or null
    cf* eq;                  // [n_frames][n_dsym][Kd]: the caller's buffer, the workspace (bits alone) or null
    float* csi;              // [n_frames][n_dsym][Kd] or null
    uint8_t* bits;           // hard bits of eq, or null
    int bits_mode;           // ofdm_bits_mode
    int mod;                 // bits per symbol (1, 2, 4, 6)
};
hipError_t launch_chan_track_est(const RxDev& rx, const ChanTrackArgs& a, hipStream_t s);
hipError_t launch_chan_track_demod(const RxDev& rx, const ChanTrackArgs& a, hipStream_t s);
hipError_t chan_track_prepare();         // loads the kernels (before a stream capture)
hipError_t launch_demap(const DemapArgs& a, hipStream_t s);
// segmented soft de-mapper: pass 1 (nearest-point distance sums per slice) and pass 2 (sigma per segment + requested arrays)
hipError_t launch_demap_frames(const SegDemapArgs& a, hipStream_t s);
// pilot tracking stage: the row kernel, then (a.cfo != null) the per-segment offset estimate over a.usum
hipError_t launch_pilot_track(const PilotArgs& a, hipStream_t s);
hipError_t launch_bit_errors(const uint8_t* a, const uint8_t* b, int64_t n, unsigned long long* count, hipStream_t s);
// out[row][i] = mean_SF( in[row][SF + i*dsss] * conj(code[SF]) ), i < n_spread  (SynchEstFOAndDSSS.py:391-399)
// rows visited in order; row r of frame f = f*D + n is divided by sqrt(mean |row f|^2) (SynchronizeAndEstimate.py:431-434)
hipError_t launch_row_renorm(cf* eq, int Kd, int D, int n_frames, const int* tsr, hipStream_t s);
// out = est_data_freq rows minus rows 3, 3+SD, ... (SynchAndChanEst.py:249-255), row-major
hipError_t launch_pack_rows(const cf* edf, int rows, int Kd, int SD, cf* out, hipStream_t s);
hipError_t launch_despread(const cf* in, int in_row_stride, const cf* code, int dsss, int n_spread, int rows, cf* out, hipStream_t s);
hipError_t launch_tx_modulate(const TxDev& tx, const ModArgs& a, hipStream_t s);
hipError_t launch_channel(const ChanArgs& a, hipStream_t s);
hipError_t launch_tx_random_bits(uint64_t seed, uint64_t offset, uint8_t* out, int64_t n, hipStream_t s);
hipError_t launch_tx_map(const uint8_t* bits, int bits_mode, int bps, int64_t n_sym, cf* out, hipStream_t s);
hipError_t launch_tx_grid(const TxDev& tx, const GridArgs& a, hipStream_t s);
hipError_t launch_tx_sync_grid(const TxDev& tx, cf* grid, hipStream_t s);
hipError_t launch_tx_time(const TxDev& tx, const TimeArgs& a, hipStream_t s);
hipError_t launch_tx_mux(const TxDev& tx, const MuxArgs& a, hipStream_t s);
size_t rx_lds_bytes(int nfft);
// RxDev::zcp for a host copy of the Zadoff-Chu sequence zc[S*Ks]: [S][nfft] entries in lane / register-slot order
std::vector<cf> rx_zc_lane_table(int nfft, int Ks, int S, const cf* zc);
// block length of the screened sync search for this numerology (0: the preconditions do not hold, use the sequential search)
int rx_sync_scan_block(const RxDev& rx);
hipError_t launch_probe(const void* in, void* out, int64_t n16, int mode, int sym_in16, int gap16, int sym_out16, int64_t n_sym,
                        hipStream_t s);

}  // namespace ofdm
