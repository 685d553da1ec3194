/* ofdm_mi355x.h -- C ABI of the MI355X-native OFDM TX/RX hot path (libofdm_mi355x.so).
 *
 * Drop-in boundary for tayloreisman16/LTE-GNU-Radio-Code's `ofdm_chain.py` path.  The reference
 * has no native code and no FFI (its blocks are pure Python/NumPy), so every entry point below
 * cites the PYTHON interface it replaces; the GNU Radio blocks in
 * `lte-gnu-radio-code_amd/{utsa_ofdm,RXOFDM,TXOFDM}` bind these symbols with ctypes
 * (INTEGRATION.md shows the stub).  G/ = GNU-Radio-Repositories/ in the reference tree.
 *
 * Conventions
 *   - plain C types only; complex samples are interleaved float32 pairs (numpy complex64,
 *     GNU Radio gr_complex); caller allocates every output; no exceptions cross the boundary.
 *   - every function returns OFDM_OK (0) / a non-negative count, or a negative ofdm_status;
 *     ofdm_last_error() gives the message of the calling thread's last failure.
 *   - `d_` arguments are DEVICE pointers (HBM of the handle's GPU), `h_` arguments are HOST pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the handle's own NON-BLOCKING stream; mind that
 *     the legacy default stream also has handle 0, so it cannot be named here).  Batch entry
 *     points are asynchronous on that stream and allocate nothing.
 *   - a handle owns one HIP stream and its device tables; no global mutable state in the library,
 *     so different block instances (GNU Radio: one thread per block) may run concurrently.
 */
#ifndef OFDM_MI355X_H
#define OFDM_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_ABI_VERSION 1    /* additions that leave every existing declaration as it is keep the version (ofdm_fo_demod_frames) */

typedef enum {
    OFDM_OK = 0,
    OFDM_ERR_INVALID = -1,      /* bad argument / unsupported configuration                        */
    OFDM_ERR_HIP = -2,          /* HIP runtime error (no device, launch failure, ...)              */
    OFDM_ERR_INDEX = -3,        /* the reference would raise IndexError (row >= num_ofdm_symb)     */
    OFDM_ERR_SHAPE = -4,        /* the reference would raise ValueError (reshape / assignment)     */
    OFDM_ERR_NOMEM = -5,
    OFDM_ERR_UNBOUND = -6       /* the reference would raise UnboundLocalError (SynchEstFOAndDSSS.py:392) */
} ofdm_status;

typedef enum { OFDM_MOD_BPSK = 1, OFDM_MOD_QPSK = 2, OFDM_MOD_16QAM = 4, OFDM_MOD_64QAM = 6 } ofdm_modulation;

/* Which generation of the reference RX block supplies the constants (SURVEY.md section 2 notes). */
typedef enum {
    OFDM_COMPAT_UTSA = 0,   /* G/gr-utsa_ofdm/python/SynchAndChanEst.py: ZC root 23, stride 1, gate arg, SNR_lin=10^(snr/20) */
    OFDM_COMPAT_RXOFDM = 1  /* G/gr-RXOFDM/python/synch_and_chan_est.py:54,81,170,184: root 37, stride cp-1, gate 0.4, linear snr */
} ofdm_compat;

typedef enum { OFDM_BITS_NONE = 0, OFDM_BITS_PACKED = 1, OFDM_BITS_UNPACKED = 2 } ofdm_bits_mode;

/* ------------------------------------------------------------------------------------------ RX
 * ctor arguments of utsa_ofdm.SynchAndChanEst (G/gr-utsa_ofdm/python/SynchAndChanEst.py:17-19). */
typedef struct {
    int32_t num_ofdm_symb;     /* rows of est_data_freq kept by the stream block (:88)            */
    int32_t nfft;              /* 64,128,...,4096                                                  */
    int32_t cp_len;
    int32_t num_synch_bins;    /* even, <= nfft                                                    */
    int32_t synch_S;           /* synch_dat[0]                                                     */
    int32_t synch_D;           /* synch_dat[1]                                                     */
    int32_t num_data_bins;     /* even, <= nfft                                                    */
    double snr;                /* the block's `snr` argument (dB-like, see :99,:214)               */
    double scale_factor_gate;  /* :166 (ignored for OFDM_COMPAT_RXOFDM: 0.4)                       */
    int32_t compat;            /* ofdm_compat                                                      */
    int32_t modulation;        /* ofdm_modulation used by the fused / standalone de-mapper         */
    int32_t device;            /* HIP device ordinal                                               */
    int32_t reserved;
} ofdm_rx_cfg;

typedef struct ofdm_rx ofdm_rx;

/* what work() leaves in the block's inspectable attributes (:83-91,:173-175,:260-261) */
typedef struct {
    double time_synch_ref[3];  /* [P*stride+cp, argmax lag, int(max|corr|)]                        */
    int32_t detected;          /* a sync trial was accepted during THIS call                        */
    int32_t trials_run;        /* sync trials evaluated during this call                            */
    int32_t count;             /* number of completed work() calls                                  */
    int32_t corr_obs;
    int64_t n_data_items;      /* n_data_symb * num_data_bins values packed at the head of `out`    */
} ofdm_rx_report;

int ofdm_rx_create(const ofdm_rx_cfg* cfg, ofdm_rx** out);
int ofdm_rx_destroy(ofdm_rx* h);

/* Replaces SynchAndChanEst.work(input_items, output_items) (:135-262), host buffers, including
 * the block's call-to-call state (count / corr_obs gating, persistent est_data_freq rows).
 * `h_in`: n_in complex64 items; `h_out`: n_out complex64 items (GNU Radio sync block: n_out == n_in).
 * Returns n_out (the reference returns len(output_items[0]), :262) or a negative ofdm_status. */
int64_t ofdm_rx_work(ofdm_rx* h, const float* h_in, int64_t n_in, float* h_out, int64_t n_out,
                     ofdm_rx_report* rep);

/* Copies block state to host (complex64 interleaved): what the reference exposes as attributes.
 * `row` selects the corr_obs row the reference wrote: 0 = estimate of the first detection (the one
 * the data equaliser keeps using, :242), 1 = estimate of the latest later-call detection (:171,188).
 * Any pointer may be NULL.  h_chan_freq[nfft]=est_chan_freq_P[row], h_chan_time[nfft]=est_chan_time[row],
 * h_synch_freq[S*Ks]=est_synch_freq[row], h_eq_gain[Ks]=eq_gain (latest), h_data_freq[num_ofdm_symb*Kd]=est_data_freq. */
int ofdm_rx_get_state(ofdm_rx* h, int32_t row, float* h_chan_freq, float* h_chan_time, float* h_synch_freq,
                      float* h_eq_gain, float* h_data_freq);

/* Frame-batched device fast path (benchmarks, multi-GPU shards): every frame is one reference
 * work() buffer processed with FRESH-instance semantics (own sync search from P=0, own channel
 * estimate; :143-248).  Frame f occupies d_iq[f*frame_stride .. +frame_len) (complex64 items).
 * n_pat = floor(floor(frame_len/L)/(S+D)) patterns are demodulated; outputs per frame:
 *   d_eq   [n_pat*D][Kd] complex64 equalised symbols, may be NULL: row p*D + n (p < n_pat, n < D) is the reference's
 *          est_data_freq[p*(S+D) + n], i.e. the data rows of every pattern in order with the rows in between left out.  Pattern p
 *          is read at the reference's pointer ptr_p = t0 + S*L*(p*(S+D) + 1) (:222, t0 = time_synch_ref[0]) and guarded once by
 *          ptr_p + nfft - 1 <= frame_len (:223, else D rows of zeros); for S > 1 that pointer meets the pattern's data symbols at
 *          p = 0 only, and the batch path restates it as it is.
 *   d_bits hard bits of those symbols: packed MSB-first [n_pat*D*Kd*bps/8] bytes or unpacked [..*bps] bytes, may be NULL
 *   d_tsr  [4] int32: time_synch_ref[0..2], detected flag, may be NULL
 * Asynchronous on `stream`.  Returns n_pat*D (data symbols per frame) or a negative ofdm_status. */
int64_t ofdm_rx_demod_frames(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride,
                             int64_t frame_len, float* d_eq, uint8_t* d_bits, int32_t bits_mode,
                             int32_t* d_tsr, void* stream);

/* Per-frame state of the LAST ofdm_rx_demod_frames call, copied to host (synchronises the stream):
 * h_chan_freq[nfft], h_gain[Kd] (equaliser gain incl. lag de-rotation), h_chan_time[nfft]. NULL = skip. */
int ofdm_rx_get_frame_state(ofdm_rx* h, int64_t frame, float* h_chan_freq, float* h_gain, float* h_chan_time);

/* Optional HIP-event timing of the two kernels ofdm_rx_demod_frames launches (bench.py's roofline leg).
 * enable != 0 records events around the sync kernel and the demod kernel on the launch stream (a ring of 32
 * calls, so a timed loop needs no host synchronisation) and resets the ring; ofdm_rx_get_kernel_ms waits for the
 * recorded events and returns the MEAN durations over the calls recorded since (at most the last 32). */
int ofdm_rx_set_profiling(ofdm_rx* h, int32_t enable);
int ofdm_rx_get_kernel_ms(ofdm_rx* h, float* sync_ms, float* demod_ms);

/* Upper bound on sync trials per frame in the batch path (0 = none: scan the whole frame like the
 * reference, :143).  A frame with no sync costs one FFT pair per sample, so hosts may cap it. */
int ofdm_rx_set_max_trials(ofdm_rx* h, int32_t max_trials);

/* Sync search of the batch path and of ofdm_rx_work.  The reference tries the windows P = 0, 1, 2, ... one by one (:143-169);
 * exhaustive != 0 does exactly that (batch: one workgroup per frame; ofdm_rx_work: a trial table in windows, then a finalize
 * launch).  exhaustive == 0 (default) uses the screened search where its preconditions hold
 * (synch_dat[0] == 1, stride 1, num_synch_bins == nfft - 2): the trials between exactly evaluated anchor trials are screened
 * with an O(cp) sliding recurrence of the lag correlations and only flagged trials are evaluated exactly -- the accepted trial,
 * its lag and every output are those of the exhaustive search; ofdm_rx_work then searches its one
 * buffer in parallel segments and accepts and finalizes the first hit in the same launch.  Returns 1 if the screened search is
 * active for this handle afterwards, 0 if the exhaustive one is, or a negative ofdm_status. */
int ofdm_rx_set_sync_search(ofdm_rx* h, int32_t exhaustive);

/* Bytes of device workspace the batch path needs for n_frames (allocated lazily, grown on demand
 * OUTSIDE the asynchronous section: call ofdm_rx_reserve before capturing into a hipGraph). */
int ofdm_rx_reserve(ofdm_rx* h, int64_t n_frames);

/* ------------------------------------------------------------------------------------------ de-map
 * Replaces BitRecovery.work (G/LEGACY/gr-ofdm-rx/python/BitRecovery.py:66-189) on device buffers.
 * d_sym: n complex64; d_hard: n*bps bytes (one bit per byte, order [b0,b1,..] per symbol), may be NULL;
 * d_soft0/d_soft1: n*bps float32 max-log metrics llrp0/llrp1, may be NULL: QPSK literally as :105-125; 16/64-QAM
 * (modulation 4/6) by the same rule per axis -- -0.5/sigma^2 * distance to the nearest PAM level carrying bit value
 * 0 / 1, sigma = 0.7071*mean(dmin) over the buffer (:88,102) -- an extension the reference does not have. */
int ofdm_demap(ofdm_rx* h, const float* d_sym, int64_t n, int32_t modulation, uint8_t* d_hard,
               float* d_soft0, float* d_soft1, void* stream);

/* Segmented soft de-mapper: ofdm_demap's soft outputs for many buffers in one call, each with ITS OWN sigma.  Segment s is
 * seg_len complex64 symbols at d_sym + s*seg_stride (complex items); its outputs are exactly what ofdm_demap defines for that
 * segment alone: sigma_s = 0.7071067811865476 * mean_i dmin(z_i) (nearest-point distance, :88,102), soft0 / soft1 = llrp0 /
 * llrp1 with hf = -0.5/sigma_s^2 (QPSK literally as :105-125, 16/64-QAM by the per-axis PAM rule of ofdm_demap), bit order
 * b0..b(bps-1) per symbol, dense [n_seg][seg_len*bps] float32.  llr = soft0 - soft1 in fp32 from the two values the same call
 * produces: the max-log log(P(b=0)/P(b=1)), positive favours bit 0.  Non-finite or zero-sigma input gives what IEEE arithmetic
 * of the same formulas gives.  Deterministic: sigma is summed per (segment, slice of 2048 symbols) and the partials are added
 * in a fixed order, so a segment's outputs are the same bits alone, in any batch and on every call.  DEVICE pointers;
 * NULL = not wanted. */
typedef struct ofdm_soft_out {
    float*  soft0;    /* [n_seg][seg_len*bps] llrp0, or NULL                  */
    float*  soft1;    /* [n_seg][seg_len*bps] llrp1, or NULL                  */
    float*  llr;      /* [n_seg][seg_len*bps] soft0 - soft1 (fp32), or NULL   */
    double* sigma;    /* [n_seg] sigma_s (a per-segment noise estimate), or NULL */
} ofdm_soft_out;

/* Device workspace of the segmented de-mapper for n_seg segments of seg_len symbols (grows, never shrinks; synchronises the
 * device).  Call it before capturing ofdm_demap_frames / ofdm_rx_demod_frames_soft into a hipGraph. */
int ofdm_rx_reserve_soft(ofdm_rx* h, int64_t n_seg, int64_t seg_len);
/* Asynchronous on `stream` (NULL = the handle's stream): two launches, no host synchronisation and no allocation once
 * ofdm_rx_reserve_soft covers the call (else the workspace grows first, outside a capture).  modulation 2, 4 or 6 (BPSK:
 * OFDM_ERR_INVALID, as ofdm_demap).  n_seg == 0, seg_len == 0 or an `out` without any pointer is a no-op returning OFDM_OK.
 * Argument errors (NULL handle, negative count, seg_stride < seg_len, a batch beyond the kernels' index range) return
 * OFDM_ERR_INVALID without touching the device. */
int ofdm_demap_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t seg_len, int64_t seg_stride,
                      int32_t modulation, const ofdm_soft_out* out, void* stream);
/* ofdm_rx_demod_frames with the same arguments (same d_eq / d_bits / d_tsr bits, same return value n_dsym), then
 * ofdm_demap_frames over d_eq with one segment per frame: seg_len = seg_stride = n_dsym*Kd, modulation = cfg.modulation.
 * A frame's segment holds every row ofdm_rx_demod_frames writes, the zero rows of guard-failed patterns and of frames without
 * a sync included.  soft == NULL or without any pointer: exactly ofdm_rx_demod_frames.  Soft outputs need d_eq (the soft
 * pass reads it); argument errors return OFDM_ERR_INVALID before anything is enqueued. */
int64_t ofdm_rx_demod_frames_soft(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride,
                                  int64_t frame_len, float* d_eq, uint8_t* d_bits, int32_t bits_mode,
                                  int32_t* d_tsr, const ofdm_soft_out* soft, void* stream);

/* ------------------------------------------------------------------------------------------ pilot-aided phase tracking
 * The receive side of ofdm_tx_set_pilots / txOFDM.OFDM_Modulation(fft_size, pilot_locations): an extension, the reference's
 * receivers have no pilot handling.  Convention: the handle's cfg.num_data_bins is the number of OCCUPIED bins K (= the
 * transmitter's num_data_bins + n_pilots), so ofdm_rx_demod_frames runs exactly as without pilots and writes rows z[0..K) in the
 * list order of binsP(K).  Pilots are n_pilots distinct signed bin offsets inside [-K/2..-1, 1..K/2] carrying pilot_re + j
 * pilot_im (the rules of ofdm_tx_set_pilots); Kd' = K - n_pilots data entries remain per row, in list order.
 * For one row, P = the pilots' list indices in ascending order, d_j = the j-th non-pilot list index:
 *   U    = sum_{p in P} z[p] * conj(pilot_value), ascending p, float32
 *   c    = conj(U)/|U| if |U|^2 is finite and > 0, else 1 (zero rows of guard-failed patterns and of frames without a sync
 *          stay zero).  |U|^2 = ur*ur + ui*ui is evaluated in float32 like U itself: a pilot sum whose square overflows float32
 *          (|U| above about 1.8e19) or underflows it to 0 (|U| below about 1e-23; a square in the denormal range, |U| up to 1e-19,
 *          may go either way) is "not usable", as is one with a NaN or an Inf in a pilot entry
 *   data[j] = c * z[d_j]                                  cpe[row] = U/|U| (the measured rotation), 0 for a row without usable U
 *   bits = the hard decision (ofdm_demap's rules) of the STORED float32 data[j], cfg.modulation 2 / 4 / 6 bits per symbol
 * OFDM_PILOT_CPE_SLOPE also removes a phase that is linear in the bin offset k: theta_p = arg(z[p] conj(pilot_value) c),
 *   tau = sum (k_p - kbar) theta_p / sum (k_p - kbar)^2, delta = mean theta - tau kbar,
 *   data[j] = c e^{-j(delta + tau k_{d_j})} z[d_j], slope[row] = tau (radians per bin; 0 for a row without usable U).
 * Per segment: cfo = arg(sum U[s+1] conj(U[s])) / (2 pi L/N) in subcarrier spacings, over consecutive rows s, s+1 of the SAME
 * pattern (they are L = nfft + cp samples apart; rows_per_pattern rows form a pattern), float64 sums, rows without usable U
 * skipped; NaN if no pair exists.  Unambiguous for |cfo| < N/(2L).
 * Deterministic: every sum has an order fixed by the row / the segment's geometry (no atomics), so a segment's outputs are the
 * same bits alone, in any batch, at any alignment and on every call. */
typedef enum { OFDM_PILOT_CPE = 0, OFDM_PILOT_CPE_SLOPE = 1 } ofdm_pilot_mode;
/* Host array, copied into a small device table; n_pilots == 0 clears it.  Synchronises the device. */
int ofdm_rx_set_pilots(ofdm_rx* h, const int32_t* h_locations, int32_t n_pilots, float pilot_re, float pilot_im);
typedef struct ofdm_pilot_out {   /* DEVICE pointers; NULL = not wanted */
    float*   data;       /* [n_seg][rows][Kd'] complex64; required with bits (and by the soft stage)              */
    uint8_t* bits;       /* hard bits of data: packed MSB-first [n_seg][rows][Kd'*bps/8] or one bit per byte        */
    int32_t  bits_mode;  /* ofdm_bits_mode of bits; OFDM_BITS_PACKED needs Kd'*bps % 8 == 0                         */
    float*   cpe;        /* [n_seg][rows] complex64                                                                 */
    float*   slope;      /* [n_seg][rows] float32, OFDM_PILOT_CPE_SLOPE only                                        */
    double*  cfo;        /* [n_seg]                                                                                 */
} ofdm_pilot_out;
/* Device workspace for the cfo output of n_seg segments of `rows` rows (grows, never shrinks; synchronises the device).  Call it
 * before capturing the two calls below into a hipGraph. */
int ofdm_rx_reserve_pilots(ofdm_rx* h, int64_t n_seg, int64_t rows);
/* The stage on any device buffer: segment s = `rows` rows of K complex64 symbols at d_sym + s*seg_stride (complex items;
 * seg_stride >= rows*K), outputs dense per segment.  Asynchronous on `stream` (NULL = the handle's stream): one launch, plus a
 * small one for cfo; no host synchronisation and no allocation once ofdm_rx_reserve_pilots covers the call.  Without pilots set,
 * with mode CPE_SLOPE and fewer than two pilots, and for any other argument error: OFDM_ERR_INVALID before anything is enqueued.
 * n_seg == 0 or an `out` without any pointer is a no-op returning OFDM_OK.  d_sym and the outputs must not overlap. */
int ofdm_pilot_track_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t seg_stride,
                            int32_t rows_per_pattern, int32_t mode, const ofdm_pilot_out* out, void* stream);
/* ofdm_rx_demod_frames with the same arguments and d_bits = NULL (d_eq is required; d_eq and d_tsr get the bits of the plain
 * call), then ofdm_pilot_track_frames over d_eq with one segment per frame (rows = n_dsym, rows_per_pattern = synch_D), then --
 * if `soft` has a pointer -- ofdm_demap_frames over out->data with seg_len = seg_stride = n_dsym*Kd', so that a frame's sigma
 * and LLRs are those of its TRACKED data symbols.  Returns n_dsym. */
int64_t ofdm_rx_demod_frames_pilots(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride,
                                    int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t mode,
                                    const ofdm_pilot_out* out, const ofdm_soft_out* soft, void* stream);

/* ------------------------------------------------------------------------------------------ channel-state-weighted LLRs
 * An extension the reference does not have.  ofdm_demap_frames restates BitRecovery: linear distances and ONE sigma per frame.
 * Behind the one-tap MMSE equaliser the symbol of a bin with channel power a = |H|^2 is shrunk by a/(a + rho), rho = 1/SNR of
 * the equaliser, and carries noise of variance sigma_n^2/a; the max-log LLR of the unbiased symbol is therefore (a/sigma_n^2)
 * times a difference of SQUARED distances, and a faded bin weighs little.  This text is the definition; tests/csi_ref.py
 * restates it in NumPy and the library equals that bit for bit.
 *
 * All arithmetic is float32, every product, sum, difference and quotient rounded on its own (no fused multiply-add), division
 * correctly rounded.  sigma2 is the only double.  Per symbol: z complex64, a = float32 channel power of the symbol's bin,
 * rho float32, w_den = float(sigma2) of the symbol's segment.
 *  1. The symbol is USABLE iff a is finite and a > 0; z.re and z.im are finite and not both zero; s = (a + rho)/a is finite;
 *     u = (z.re*s, z.im*s) is finite.  Zero rows of guard-failed patterns, frames without a sync and bins without an estimate are
 *     therefore erasures.
 *  2. Axis levels are the library's float32 ones: +-0.70710678f for QPSK (bit 0 <-> the positive level), else
 *     l_q = float(2q - (M-1)) * u, q = 0..M-1, M = 4 (u = 0.31622776601683794f) or 8 (u = 0.15430334996209191f), with the TS 36.211
 *     7.1 labels of ofdm_demap: axis bit 0 = (l < 0); 16-QAM bit 1 = (|2q-(M-1)| == 3); 64-QAM bit 1 = (|.| > 4), bit 2 = (|.| == 1 or 7).
 *  3. For axis bit j of coordinate x (u.re or u.im):  d = min_{l: bit = 1} (x-l)*(x-l)  -  min_{l: bit = 0} (x-l)*(x-l),
 *     explicit minima over the levels.
 *  4. Bit order b0..b(bps-1) per symbol as ofdm_demap: b0 = axis bit 0 of re, b1 = axis bit 0 of im, b2 = axis bit 1 of re, ...
 *  5. llr = (a / w_den) * d  if the symbol is usable, w_den is finite and > 0, and the product is finite; else llr = +0.0f.
 *     Positive favours bit 0 (the convention of ofdm_soft_out.llr).  No non-finite value leaves the call.
 *  6. Noise term of a usable symbol: e = a * (mr + mi), mr / mi = min over ALL levels of (u.re-l)*(u.re-l) / (u.im-l)*(u.im-l)
 *     (the squared distance to the nearest point).  A symbol whose e is not finite is left out.
 *  7. OFDM_CSI_NOISE_EST: sigma2 = sum double(e) / n_used per segment, n_used (int64) = the symbols of step 6 that are in the
 *     sum; n_used == 0 gives sigma2 = 0 and every LLR +0.  The order of the sum is fixed by (rows, row_len) alone: one partial
 *     per (segment, slice of 2048 symbols), the partials added in a fixed order, no atomics -- a segment's outputs are the same
 *     bits alone, in any batch, at any alignment and on every call.
 *     OFDM_CSI_NOISE_GIVEN: sigma2 = noise_var for every segment and no estimation pass runs; the sigma2 output, if wanted, is
 *     that value and n_used the number of usable symbols (step 1) of the segment.
 * The estimate of step 7 is decision-directed: at low SNR the nearest point is often the wrong one and sigma2 comes out too
 * SMALL.  Inside one code block that is harmless (max-log decoders are invariant to a common scale of their LLRs); it matters
 * where LLRs of different frames are added (HARQ combining) -- pass a known noise_var there. */
typedef enum { OFDM_CSI_NOISE_EST = 0, OFDM_CSI_NOISE_GIVEN = 1 } ofdm_csi_noise_mode;
typedef enum { OFDM_CSI_ROWS_ALL = 0, OFDM_CSI_ROWS_DATA = 1 } ofdm_csi_layout;
typedef struct ofdm_csi_out {     /* DEVICE pointers; NULL = not wanted */
    float*   llr;      /* [n_seg][rows*row_len*bps] float32, dense */
    double*  sigma2;   /* [n_seg] the noise variance the segment's LLRs were scaled with */
    int64_t* n_used;   /* [n_seg] */
} ofdm_csi_out;
/* Device workspace (partials and the per-(segment, entry) tables) for n_seg segments of `rows` rows of row_len symbols: grows,
 * never shrinks; synchronises the device.  Call it before capturing the calls below into a hipGraph; inside a capture a call
 * that needs more is refused. */
int ofdm_rx_reserve_csi(ofdm_rx* h, int64_t n_seg, int64_t rows, int64_t row_len);
/* d_csi[f*csi_stride + j] = re*re + im*im (float32, each product rounded) of the channel estimate of frame f of the LAST
 * ofdm_rx_demod_frames call on this handle (the est_chan_freq_P row ofdm_rx_get_frame_state returns), in bin-list order:
 * OFDM_CSI_ROWS_ALL: j over binsP(num_data_bins); OFDM_CSI_ROWS_DATA: the Kd' non-pilot entries in list order (needs
 * ofdm_rx_set_pilots, else OFDM_ERR_INVALID).  n_frames beyond that call's count: OFDM_ERR_INVALID.  Asynchronous on `stream`
 * (NULL = the handle's stream), one launch. */
int ofdm_rx_csi_frames(ofdm_rx* h, int64_t n_frames, int32_t layout, float* d_csi, int64_t csi_stride, void* stream);
/* The stage on any device buffer: segment s = `rows` rows of row_len complex64 symbols at d_sym + s*seg_stride (complex items);
 * entry j of every row of segment s has a = d_csi[s*csi_stride + j].  modulation 2, 4 or 6 (BPSK: OFDM_ERR_INVALID).
 * Asynchronous on `stream`: up to four launches, no host synchronisation and no allocation once ofdm_rx_reserve_csi covers
 * the call.  n_seg == 0, rows == 0, row_len == 0 or an `out` without any pointer is a no-op returning OFDM_OK.  Argument
 * errors return OFDM_ERR_INVALID with the reason in ofdm_last_error() before the handle is read: negative counts, seg_stride <
 * rows*row_len, csi_stride < row_len, unknown noise_mode, OFDM_CSI_NOISE_GIVEN with noise_var not finite or <= 0, rho negative
 * or not finite, index range exceeded (n_seg > 2^31, row_len > 2^30, rows*row_len, n_seg*seg_stride or n_seg*csi_stride > 2^40).
 * d_sym, d_csi and the outputs must not overlap. */
int ofdm_demap_csi_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride,
                          const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode,
                          double noise_var, const ofdm_csi_out* out, void* stream);
/* ofdm_rx_demod_frames with the same arguments (same d_eq / d_bits / d_tsr bits, same return value n_dsym), then
 * ofdm_rx_csi_frames(OFDM_CSI_ROWS_ALL) into the workspace and ofdm_demap_csi_frames over d_eq with one segment per frame:
 * rows = n_dsym, row_len = num_data_bins, rho = 1/snr_data of the handle's equaliser, modulation = cfg.modulation.  Needs d_eq.
 * out == NULL or without any pointer: exactly ofdm_rx_demod_frames.
 * Signals with pilots: chain ofdm_rx_demod_frames_pilots -> ofdm_rx_csi_frames(OFDM_CSI_ROWS_DATA) -> ofdm_demap_csi_frames over
 * its out->data (rows = n_dsym, row_len = Kd', rho = 1/snr as above); the tracking stage only rotates, so a is unchanged. */
int64_t ofdm_rx_demod_frames_csi(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                 float* d_eq, uint8_t* d_bits, int32_t bits_mode, int32_t* d_tsr, int32_t noise_mode,
                                 double noise_var, const ofdm_csi_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ receive-diversity combining
 * An extension the reference does not have: maximum-ratio combining (MRC) of B receive branches (antennas) behind the batch
 * receiver, with max-log LLRs of the combined symbol.  Behind the one-tap MMSE equaliser a branch's symbol z of a bin with channel
 * power a = |H|^2 is conj(H) y / (a + rho), so z (a + rho) / sigma_b^2 is the matched-filter output over the branch's noise
 * variance; their sum over the branches divided by A = sum a / sigma_b^2 is the unbiased combined symbol, which carries noise of
 * variance 1/A.  This text is the definition; tests/mrc_ref.py restates it in NumPy and the library equals that bit for bit.
 *
 * All arithmetic is float32, every product, sum, difference and quotient rounded on its own (no fused multiply-add), division
 * correctly rounded.  The noise variances are the only doubles.  Layout, branch-major: branch b of segment s is the unit
 * g = b*n_seg + s: `rows` rows of row_len complex64 symbols at d_sym + g*seg_stride (complex items), channel powers at
 * d_csi + g*csi_stride, noise variance sigma2[g] with w_den = float(sigma2[g]).
 *  1. Per (unit g, entry j), a = d_csi[g*csi_stride + j], rho the float32 equaliser term: c = (a + rho)/w_den, t = a/w_den.
 *     The entry is USABLE iff a is finite and > 0; w_den is finite and > 0; c is finite; t is finite and > 0.
 *  2. Per symbol and branch, z the equalised symbol: p = (z.re*c, z.im*c).  The branch TAKES PART iff its entry is usable;
 *     z.re and z.im are finite and not both zero; p is finite.
 *  3. Over the branches that take part, in the order b = 0, 1, ..., B-1 and starting from +0.0f:  N = sum p (re and im
 *     separately), A = sum t.  A branch that does not take part leaves the sums as they are.
 *  4. u = (N.re/A, N.im/A).  The symbol is USABLE iff at least one branch took part, A is finite and > 0, and u is finite.
 *  5. d per axis bit of u exactly as steps 2-4 of the channel-state-weighted LLR contract above: the same float32 levels and
 *     labels, explicit minima of squared differences, the bit order of ofdm_demap.
 *  6. llr = A * d if the symbol is usable and the product is finite, else +0.0f.  Positive favours bit 0.  No non-finite value
 *     leaves the call.
 *  7. sym = u if the symbol is usable, else 0+0j; weight = A if usable, else +0.0f.
 * A branch without a sync, the zero rows of a guard-failed pattern, a bin without an estimate and a branch whose sigma2 is 0 are
 * therefore erasures of that branch alone: the others carry the symbol.  The result depends on (B, rows, row_len) and the data
 * alone: the same bits in any batch, at either alignment and on every call.
 * Noise: OFDM_MRC_NOISE_GIVEN takes the HOST array h_noise_var[n_branch] (each finite and > 0, else OFDM_ERR_INVALID), read at
 * call time and passed as kernel arguments -- a captured graph keeps them; sigma2[g] = h_noise_var[b].  OFDM_MRC_NOISE_SEG takes
 * the DEVICE array d_sigma2[n_branch*n_seg] indexed by g: the layout ofdm_csi_out.sigma2 has when the channel-state-weighted
 * LLR stage runs over the B*n_seg units as its segments.  OFDM_MRC_NOISE_EST (ofdm_rx_demod_frames_mrc only) estimates them.
 * Estimates are decision-directed and come out too small at low SNR (see above); a branch whose estimate is too small by a
 * larger factor than the others' is weighed too heavily -- pass known variances where they are known. */
#define OFDM_MRC_MAX_BRANCHES 8
typedef enum { OFDM_MRC_NOISE_GIVEN = 0, OFDM_MRC_NOISE_SEG = 1, OFDM_MRC_NOISE_EST = 2 } ofdm_mrc_noise_mode;
typedef struct ofdm_mrc_out {   /* DEVICE pointers; NULL = not wanted */
    float* llr;      /* [n_seg][rows*row_len*bps] */
    float* sym;      /* [n_seg][rows*row_len] complex64 */
    float* weight;   /* [n_seg][rows*row_len] */
} ofdm_mrc_out;
/* Device workspace of the two calls below for n_branch branches of n_seg segments of `rows` rows of row_len symbols (it
 * includes ofdm_rx_reserve_csi over the n_branch*n_seg units): grows, never shrinks; synchronises the device.  Call it before
 * capturing the calls below into a hipGraph; inside a capture a call that needs more is refused. */
int ofdm_rx_reserve_mrc(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len);
/* The stage on any device buffer.  modulation 2, 4 or 6; noise_mode OFDM_MRC_NOISE_GIVEN or OFDM_MRC_NOISE_SEG
 * (OFDM_MRC_NOISE_EST: OFDM_ERR_INVALID).  Asynchronous on `stream`: two launches, no host synchronisation and no allocation
 * once ofdm_rx_reserve_mrc covers the call.  n_seg == 0, rows == 0, row_len == 0 or an `out` without any pointer is a no-op
 * returning OFDM_OK.  Argument errors return OFDM_ERR_INVALID with the reason in ofdm_last_error() before the handle is read:
 * negative counts, n_branch outside 1..8, seg_stride < rows*row_len, csi_stride < row_len, unknown noise_mode, the pointer the
 * mode needs missing, a given variance not finite or <= 0, rho negative or not finite, index range exceeded (n_branch*n_seg >
 * 2^31, row_len > 2^30, rows*row_len, n_branch*n_seg*seg_stride or n_branch*n_seg*csi_stride > 2^40).  d_sym, d_csi, d_sigma2
 * and the outputs must not overlap. */
int ofdm_combine_csi_frames(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len,
                            int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, int32_t modulation,
                            int32_t noise_mode, const double* h_noise_var, const double* d_sigma2,
                            const ofdm_mrc_out* out, void* stream);
/* d_iq holds n_branch*n_frames frames at one frame_stride, frame f of branch b at index b*n_frames + f.  Runs
 * ofdm_rx_demod_frames over all of them (d_eq is required, gets the bits of that call and is left for the caller; d_tsr is
 * [n_branch*n_frames][4]), ofdm_rx_csi_frames(OFDM_CSI_ROWS_ALL) into the workspace, for OFDM_MRC_NOISE_EST the estimation pass
 * of ofdm_demap_csi_frames over the n_branch*n_frames units (sigma2 of a unit is bit for bit what ofdm_rx_demod_frames_csi
 * reports for that frame), then the combiner with rows = n_dsym, row_len = num_data_bins, rho = 1/snr_data of the handle's
 * equaliser and modulation = cfg.modulation.  noise_mode OFDM_MRC_NOISE_GIVEN (h_noise_var[n_branch]) or OFDM_MRC_NOISE_EST.
 * d_sigma2_out [n_branch*n_frames] (may be NULL) receives the variances used.  out == NULL or without any pointer, and no
 * d_sigma2_out: exactly ofdm_rx_demod_frames.  Returns n_dsym or a negative status. */
int64_t ofdm_rx_demod_frames_mrc(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                 int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode,
                                 const double* h_noise_var, const ofdm_mrc_out* out, double* d_sigma2_out, void* stream);

/* ------------------------------------------------------------------------------------------ DFT-spread OFDM
 * An extension the reference does not have: the LTE uplink waveform (SC-FDMA, TS 36.211 5.3.3).  The transmitter sends every row
 * of M modulation symbols through an orthonormal M-point DFT before the resource grid (transform precoding); the receiver
 * undoes it behind the one-tap equaliser (despreading).  M is any 2^a 3^b 5^c in 1 .. 4096 (137 sizes; ofdm_dft_size_ok), both
 * directions carry 1/sqrt(M), twiddles come from a table built in fp64 and rounded once.  Behind the MMSE equaliser the despread
 * symbol is biased and its noise is no longer the per-bin sigma^2/|H|^2: every symbol of a segment shares one gain beta and one
 * post-despread variance nu.  ofdm_demap_csi_frames and ofdm_combine_csi_frames give WRONG weights if fed despread symbols; the
 * LLR rule of this waveform is part of the stage below.  This text is the definition; tests/dft_spread_ref.py restates it in
 * fp64 NumPy.
 *
 * Layout: segment s is `rows` rows of M complex64 at d_sym + s*seg_stride (complex items); entry k of every row of the segment
 * has the channel power a = d_csi[s*csi_stride + k] (float32); rho (float32) is 1/SNR of the equaliser; sigma2 is a double per
 * segment.
 *  1. Entry mask.  Entry k is USABLE iff a is finite and > 0.  z'_k = z_k if the entry is usable and z_k.re, z_k.im are finite,
 *     else z'_k = 0.
 *  2. Inverse transform.  x_i = (1/sqrt(M)) sum_k z'_k e^(+2 pi j i k / M), in float32 and in the library's own operation order
 *     (the bits are those of ofdm_dft_despread_frames with d_csi == NULL on the masked row).  A row whose z' are all 0+0j is an
 *     erasure: sym = +0, llr = +0, bits those of a zero symbol.
 *  3. Per-segment weights, in double: b_k = a/(a + rho) for usable entries and 0 for the others; beta = sum b_k / M;
 *     nu = sum [(b_k - beta)^2 + sigma2 * a/(a + rho)^2] / M, the second term over usable entries only; w = beta^2 / nu.  The
 *     sums run in a fixed order without atomics.  The segment is USABLE iff beta, nu and w are finite and > 0 and float(1/beta)
 *     and float(w) are finite.  beta = float(beta) and weight = float(w), or +0 both where the segment is not usable.
 *  4. Outputs.  u = x * float(1/beta) (float32, each product rounded); sym = u where the segment is usable, the row is no erasure
 *     and u.re, u.im are finite, else +0+0j.  d per axis bit of the stored float32 sym exactly as steps 2-4 of the
 *     channel-state-weighted LLR contract above (levels, labels, explicit minima, bit order).  llr = weight * d if the stored sym is not 0+0j and the product is finite
 *     and not zero, else +0.  bits = ofdm_demap's hard rule on the stored sym.  No non-finite value leaves the call.
 * Noise modes: OFDM_DESPREAD_NOISE_RHO sigma2 = rho, the equaliser's own assumption (nothing else needed);
 * OFDM_DESPREAD_NOISE_GIVEN one host double noise_var, finite and > 0, read at call time (a captured graph keeps it);
 * OFDM_DESPREAD_NOISE_SEG device doubles d_sigma2[n_seg] (a value that is not finite or <= 0 makes nu fail step 3's test or
 * simply shifts it; the segment is then judged by step 3 alone).
 * d_csi == NULL: the plain orthonormal inverse DFT -- every entry usable, beta = weight = 1, the noise mode ignored.
 * sym agrees with the fp64 restatement to max|a-b|/max|b| < 1e-5; beta and weight within one float32 ulp (double sums rounded
 * once); llr and bits are bit-exact functions of the device's own stored sym and weight.  The results depend on (rows, M) and
 * the data alone: the same bits in any batch, at either alignment (8- or 16-byte row bases) and on every call. */
typedef enum { OFDM_DESPREAD_NOISE_RHO = 0, OFDM_DESPREAD_NOISE_GIVEN = 1, OFDM_DESPREAD_NOISE_SEG = 2 } ofdm_despread_noise;
typedef struct ofdm_despread_out {   /* DEVICE pointers; NULL = not wanted */
    float*   sym;      /* [n_seg][rows*M] complex64, dense; may be d_sym itself where seg_stride == rows*M */
    float*   llr;      /* [n_seg][rows*M*bps] float32, dense */
    uint8_t* bits;     /* hard bits of sym: [n_seg][rows*M*bps] one per byte, or /8 bytes packed MSB-first */
    float*   beta;     /* [n_seg] */
    float*   weight;   /* [n_seg] */
} ofdm_despread_out;
/* Host calls, no GPU needed.  ofdm_dft_size_ok: 1 iff M = 2^a 3^b 5^c and 1 <= M <= 4096.  ofdm_dft_plan_info: the passes of
 * the plan for M, how many of them are radix-8 (none: the plans use radix 3, 5, 4 and 2) and the rows a workgroup transforms at
 * once; OFDM_ERR_INVALID for a size that is not ok.  Output pointers may be NULL. */
int ofdm_dft_size_ok(int32_t M);
int ofdm_dft_plan_info(int32_t M, int32_t* n_pass, int32_t* radix8, int32_t* rows_per_group);
struct ofdm_tx;       /* the transmitter handle (typedef ofdm_tx below) */
/* Transform precoder: n_rows contiguous rows of M complex64, out[r] = DFT_M(in[r]) / sqrt(M).  d_out == d_sym is allowed.
 * Asynchronous on `stream`, one launch.  A plan for M that the handle does not hold yet is built first (see
 * ofdm_tx_reserve_spread); inside a capture that is refused.  n_rows == 0: no-op. */
int ofdm_tx_dft_spread(struct ofdm_tx* h, const float* d_sym, int64_t n_rows, int32_t M, float* d_out, void* stream);
/* Builds and caches the plan for M (its twiddle table on the device; a handle keeps up to 8 plans, the least recently used one
 * makes room) and sizes the workspace of ofdm_tx_modulate_frames_spread for n_rows data symbols.  Grows, never shrinks;
 * synchronises the device.  Call it before capturing; inside a capture a call that needs a new plan or a larger workspace is
 * refused before anything is enqueued. */
int ofdm_tx_reserve_spread(struct ofdm_tx* h, int32_t M, int64_t n_rows);
/* The stage calls ofdm_tx_map -> ofdm_tx_dft_spread (M = num_data_bins) -> ofdm_tx_grid -> ofdm_tx_ifft_cp(1, 1) -> ofdm_tx_mux over
 * the handle's workspace: n_frames frames of n_sym symbols, the bits of frame f at d_bits + f * (bits or bytes per frame).
 * Needs n_sym % (S + D) == 0 and frame_stride == n_sym*(nfft + cp), else OFDM_ERR_INVALID.  Pilots set by ofdm_tx_set_pilots pass
 * through the grid untouched (they are not spread).  Returns the symbols written (n_frames * n_sym) or a negative error. */
int64_t ofdm_tx_modulate_frames_spread(struct ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                                       float* d_iq, int64_t frame_stride, void* stream);
/* The despreading stage on any device buffer (layout and steps above).  modulation 2, 4 or 6 (BPSK: OFDM_ERR_INVALID);
 * bits_mode is read when out->bits is wanted.  Asynchronous on `stream`: two launches, no host synchronisation and no
 * allocation once ofdm_rx_reserve_despread covers the call.  Zero counts or an M*rows*n_seg of 0 are a no-op.  Refusals are
 * OFDM_ERR_INVALID with the reason in ofdm_last_error(), before anything is enqueued or any output touched: null handle, M not
 * 2^a 3^b 5^c in 1 .. 4096, negative counts, seg_stride < rows*M, csi_stride < M, unknown noise_mode, OFDM_DESPREAD_NOISE_GIVEN
 * with noise_var not finite or <= 0, OFDM_DESPREAD_NOISE_SEG without d_sigma2, rho negative or not finite, BPSK, bits wanted
 * with OFDM_BITS_NONE or packed bits where M*bps % 8 != 0, `out` NULL or without any pointer, out->sym == d_sym with
 * seg_stride != rows*M, index range exceeded (n_seg > 2^31, rows*M, n_seg*seg_stride or n_seg*csi_stride > 2^40, more than
 * 2^31 - 1 workgroups).  Apart from out->sym == d_sym the buffers must not overlap. */
int ofdm_dft_despread_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int32_t M, int64_t seg_stride,
                             const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode,
                             double noise_var, const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out,
                             void* stream);
/* Plan cache and capture rule as ofdm_tx_reserve_spread; sizes the per-segment table for n_seg segments and the |H|^2 rows of
 * ofdm_rx_demod_frames_despread (n_seg frames). */
int ofdm_rx_reserve_despread(ofdm_rx* h, int32_t M, int64_t n_seg);
/* ofdm_rx_demod_frames (d_eq required, no hard bits of the equalised rows; same d_eq / d_tsr bits and return value n_dsym), then
 * ofdm_rx_csi_frames(OFDM_CSI_ROWS_ALL) into the workspace, then the stage over d_eq with one segment per frame: rows = n_dsym,
 * M = num_data_bins, rho = 1/snr_data of the handle's equaliser, modulation = cfg.modulation.  It runs the handle's ordinary
 * sync and demod and so follows ofdm_rx_set_chan_window and ofdm_rx_set_chan_average like every ofdm_rx_demod_frames_* call.
 * Signals with pilots: chain ofdm_rx_demod_frames_pilots -> ofdm_rx_csi_frames(OFDM_CSI_ROWS_DATA) -> ofdm_dft_despread_frames over
 * its out->data (rows = n_dsym, M = Kd'). */
int64_t ofdm_rx_demod_frames_despread(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                      float* d_eq, int32_t* d_tsr, int32_t noise_mode, double noise_var, const double* d_sigma2,
                                      int32_t bits_mode, const ofdm_despread_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ receive diversity for DFT-spread OFDM
 * An extension the reference does not have: B receive branches (antennas) of a DFT-spread signal.  The branches are combined per
 * bin in the frequency domain FIRST and the combined row is despread afterwards, so that the gain and the noise behind the
 * inverse transform come from the COMBINED channel.  (ofdm_combine_csi_frames followed by ofdm_dft_despread_frames, or despreading
 * per branch and adding, give wrong weights.)  This text is the definition; tests/mrc_despread_ref.py restates it in NumPy.
 *
 * Layout as ofdm_combine_csi_frames, branch-major: branch b of segment s is the unit g = b*n_seg + s: `rows` rows of M complex64
 * equalised symbols at d_sym + g*seg_stride (complex items), channel powers a = |H|^2 at d_csi + g*csi_stride (float32), one
 * noise variance sigma2[g] (double) per unit, rho the equaliser's float32 term.  M is any size ofdm_dft_size_ok accepts, B is
 * 1 .. OFDM_MRC_MAX_BRANCHES.
 *  1.-3. Exactly steps 1-3 of the receive-diversity contract above with row_len = M: c = (a + rho)/w_den and t = a/w_den per (unit,
 *     entry) with the USABLE rule for entries, p = z*c with the TAKES PART rule for a branch of a symbol, N = sum p and A = sum t
 *     from +0 in branch order.  All float32, every operation rounded on its own (no fused multiply-add).
 *  4. MMSE combining per bin, float32: den = A + 1.0f, v = (N.re/den, N.im/den).  The symbol is COMBINED iff at least one branch
 *     took part, A is finite and > 0, and v is finite; otherwise v = 0+0j and A counts as 0 in step 6.  With unit-power symbols
 *     v_k = b_k X_k + noise with b_k = A/(A + 1) and noise variance b_k (1 - b_k).  The "1" is the symbols' power in units of the
 *     noise variances: unlike ofdm_combine_csi_frames, whose u = N/A does not see a common factor of the sigma2, the ABSOLUTE
 *     level of the variances matters here -- variances too small by a factor f act as an equaliser tuned to an SNR f too high.
 *  5. Inverse transform of the row of v: x_i = (1/sqrt(M)) sum_k v_k e^(+2 pi j i k / M), in float32 and in the library's own
 *     operation order (the bits are those of ofdm_dft_despread_frames with d_csi == NULL on that row).  A row whose v are all
 *     0+0j is an erasure.
 *  6. Weights per ROW, in double (a branch may miss a single row -- the zero rows of a guard-failed pattern -- so A may differ
 *     from row to row of a segment).  Over the M entries of the row, with A the float32 value of step 4 widened: b = A/(A + 1.0),
 *     e = 1.0/(A + 1.0); b = 0 and e = 1 for a symbol that is not combined.  beta = sum b / M, eps = sum e / M, w = beta/eps.
 *     (The variance behind the transform is nu = mean(b^2) - beta^2 + mean(b e) = beta eps, so beta^2/nu = beta/eps; eps is summed
 *     on its own and not taken as 1 - beta, which would cancel at high SNR.)  The two sums run in an order fixed by M alone,
 *     without atomics: a row's beta and weight are the same bits wherever the row stands in its segment or the batch.  The row
 *     is USABLE iff it is no erasure; beta, eps and w are finite and > 0; float(1/beta) and float(w) are finite.
 *  7. Outputs.  u = x * float(1/beta) (float32, each product rounded); sym = u where the row is usable and u.re, u.im are finite,
 *     else +0+0j.  llr and bits are functions of the STORED float32 sym and the row's weight = float(w) exactly as step 4 of the
 *     DFT-spread contract above: llr = weight * d if the stored sym is not 0+0j and the product is finite and not zero, else +0;
 *     bits = ofdm_demap's hard rule on the stored sym.  beta = float(beta) and weight, +0 both where the row is not usable.
 *     comb = the v of step 4, before the transform.  No non-finite value leaves the call.
 * Noise: OFDM_MRC_NOISE_GIVEN (HOST array h_noise_var[n_branch], each finite and > 0, read at call time) and OFDM_MRC_NOISE_SEG
 * (DEVICE doubles d_sigma2[n_branch*n_seg] indexed by g; a value that is not finite or <= 0 is an erasure of that unit).
 * OFDM_MRC_NOISE_EST is refused by both calls: the decision-directed estimate assumes constellation points per bin, which a
 * spread signal does not have.  Decision-free sources for the SEG array are ofdm_rx_chan_noise_frames and
 * ofdm_rx_chan_spread_frames (both per frame = per unit of a branch-major batch, in the units of the equalised symbols' noise:
 * variance per bin of a signal of unit power per bin).
 * comb is bit for bit the float32 restatement; sym agrees with fp64 on those float32 v to max|a-b|/max|b| < 1e-5; beta and weight
 * within one float32 ulp (double sums rounded once); llr and bits are bit-exact functions of the device's own stored sym and
 * weight.  The results depend on (B, M) and the row's data alone: the same bits in any batch, at any position of the row, at
 * either alignment of every branch (8- or 16-byte bases) and on every call. */
typedef struct ofdm_mrc_despread_out {   /* DEVICE pointers; NULL = not wanted */
    float*   sym;      /* [n_seg][rows*M] complex64, dense */
    float*   llr;      /* [n_seg][rows*M*bps] float32, dense */
    uint8_t* bits;     /* hard bits of sym: [n_seg][rows*M*bps] one per byte, or /8 bytes packed MSB-first */
    float*   beta;     /* [n_seg][rows] */
    float*   weight;   /* [n_seg][rows] */
    float*   comb;     /* [n_seg][rows*M] complex64, dense: the combined symbols before the transform */
} ofdm_mrc_despread_out;
/* Builds and caches the plan for M (ofdm_rx_reserve_despread's cache and capture rule), sizes the {c, t} table for n_branch*n_seg
 * units and the |H|^2 rows of ofdm_rx_demod_frames_mrc_despread for n_branch*n_seg frames (n_branch*n_seg*num_data_bins floats,
 * which ofdm_combine_despread_frames itself never reads: a caller of the stage alone pays them too, also where the stage grows
 * its workspace on its own).  Grows, never shrinks; synchronises the device.  Call it before capturing; inside a capture a call that needs more is refused before anything is enqueued. */
int ofdm_rx_reserve_mrc_despread(ofdm_rx* h, int32_t M, int32_t n_branch, int64_t n_seg);
/* The stage on any device buffer (layout and steps above).  modulation 2, 4 or 6; bits_mode is read when out->bits is wanted.
 * Asynchronous on `stream`: two launches (the combiner's table, then one fused launch that combines, transforms and writes),
 * no host synchronisation and no allocation once ofdm_rx_reserve_mrc_despread covers the call.  n_seg == 0 or rows == 0 is a
 * no-op.  Refusals are OFDM_ERR_INVALID with the reason in ofdm_last_error(), before anything is enqueued or any output
 * touched: everything ofdm_combine_csi_frames and ofdm_dft_despread_frames refuse for the same argument (null handle, M not
 * 2^a 3^b 5^c in 1 .. 4096, negative counts, n_branch outside 1..8, seg_stride < rows*M, csi_stride < M, BPSK, unknown noise_mode,
 * the pointer the mode needs missing, a given variance not finite or <= 0, rho negative or not finite, bits wanted with
 * OFDM_BITS_NONE or packed bits where M*bps % 8 != 0, `out` NULL or without any pointer, index range exceeded: n_branch*n_seg >
 * 2^31, rows*M, n_branch*n_seg*seg_stride or n_branch*n_seg*csi_stride > 2^40, more than 2^31 - 1 workgroups), and
 * OFDM_MRC_NOISE_EST.  The buffers must not overlap. */
int ofdm_combine_despread_frames(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int32_t M,
                                 int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, int32_t modulation,
                                 int32_t noise_mode, const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                 const ofdm_mrc_despread_out* out, void* stream);
/* d_iq in the layout of ofdm_rx_demod_frames_mrc (frame f of branch b at index b*n_frames + f).  Runs ofdm_rx_demod_frames over
 * the n_branch*n_frames frames (d_eq required; d_eq and d_tsr get the bits of that call), ofdm_rx_csi_frames(OFDM_CSI_ROWS_ALL)
 * into the workspace, then the stage with rows = n_dsym, M = num_data_bins, rho = 1/snr_data of the handle's equaliser and
 * modulation = cfg.modulation.  d_sigma2 (OFDM_MRC_NOISE_SEG) is [n_branch*n_frames].  Every check is made before anything is
 * enqueued.  Returns n_dsym or a negative status. */
int64_t ofdm_rx_demod_frames_mrc_despread(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                          int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode,
                                          const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                          const ofdm_mrc_despread_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ multi-user allocations of DFT-spread OFDM
 * An extension the reference does not have: the multiple access of SC-FDMA.  Several users share a symbol; each occupies its own
 * contiguous run of subcarriers, with its own DFT size, its own modulation and, behind the transform, its own gain beta and LLR
 * weight.  Nothing changes in front of the stage: the channel estimate, the equaliser and ofdm_rx_csi_frames work per bin.  This
 * text is the definition; tests/dft_alloc_ref.py restates it in NumPy (a loop over the allocations around tests/dft_spread_ref.py).
 *
 * An ALLOCATION is (start, M, modulation): entries start .. start+M-1 of a row of row_len entries.  M is any size
 * ofdm_dft_size_ok accepts, modulation is 2, 4 or 6 bits per symbol and is read by the receiver only (the transmitter's mapper
 * keeps the handle's single modulation).  An ALLOCATION SET is a list of up to OFDM_MAX_ALLOCS allocations that do not overlap.
 * The list need not be sorted and may leave gaps; its order is the caller's and fixes the order of the outputs.
 *
 * The contract in one sentence: for every allocation u the stage writes exactly -- bit for bit, in every output, beta and weight
 * included -- what ofdm_dft_despread_frames writes for M = M_u and modulation = mod_u when given a dense copy of columns
 * start_u .. start_u+M_u-1 of every row, the same columns of d_csi, the same rho and the same noise.  Steps 1-4 of the DFT-spread
 * contract above apply per allocation, word for word.  Entries of a row outside every allocation are never read for data.  With
 * OFDM_DESPREAD_NOISE_SEG the one sigma2 of a segment is shared by all its allocations: it is the receiver's noise, not a user's.
 * The transmit precoder likewise replaces allocation u of every row by what ofdm_tx_dft_spread gives on the gathered columns, bit
 * for bit, and writes every entry outside all allocations as +0+0j (nothing is sent there).
 *
 * Outputs are allocation-major and dense: block u of sym is [n_seg][rows*M_u] complex64 at symbol offset
 * n_seg*rows*sum_{v<u} M_v; llr and bits likewise with M_v*bps_v (packed bits: that count / 8, and M_u*bps_u % 8 == 0 for every
 * u); beta and weight are [n_alloc][n_seg].  ofdm_alloc_layout returns these offsets. */
#define OFDM_MAX_ALLOCS 32
/* Host call, no GPU needed: the offsets of the blocks in sym (complex items), llr (floats) and bits (bytes; all 0 with
 * OFDM_BITS_NONE) and totals[3] = the sizes of the three outputs in the same units.  n_alloc in 1 .. OFDM_MAX_ALLOCS, sizes and
 * modulations as above, counts >= 0, packed bits only where every M*bps % 8 == 0: else OFDM_ERR_INVALID.  Output pointers may be
 * NULL. */
int ofdm_alloc_layout(int32_t n_alloc, const int32_t* M, const int32_t* mod, int64_t n_seg, int64_t rows, int32_t bits_mode,
                      int64_t* sym_off, int64_t* llr_off, int64_t* bits_off, int64_t* totals);
/* The allocation set of a handle, from HOST arrays that are copied; n_alloc == 0 clears it.  Synchronises the device, like
 * ofdm_*_set_pilots (call it outside a capture; a graph captured with an earlier set must not be replayed afterwards).  The set
 * owns what its kernels read: its plans, their twiddle tables (built as those of the single-M calls: fp64, rounded once) and the
 * descriptor table on the device.  It does not live in the 8-slot plan cache: no later reserve or single-M call invalidates it
 * and it evicts nothing.  Refused with OFDM_ERR_INVALID and the reason in ofdm_last_error(), the previous set staying in force:
 * null handle, n_alloc outside 0 .. OFDM_MAX_ALLOCS, null arrays with n_alloc > 0, start < 0, an M that is not ok,
 * start + M > 4096, two allocations that overlap, a modulation that is not 2, 4 or 6. */
int ofdm_rx_set_allocations(ofdm_rx* h, int32_t n_alloc, const int32_t* h_start, const int32_t* h_M, const int32_t* h_mod);
int ofdm_tx_set_allocations(struct ofdm_tx* h, int32_t n_alloc, const int32_t* h_start, const int32_t* h_M);
/* Sizes the [n_alloc][n_seg] table of the stage for the set in force and the |H|^2 rows of ofdm_rx_demod_frames_despread_alloc
 * (n_seg frames), and loads the kernels.  Grows, never shrinks; synchronises the device.  Needs a set.  After it the stage
 * enqueues without host synchronisation or allocation and can be captured and replayed; inside a capture a call that needs more
 * is refused before anything is enqueued. */
int ofdm_rx_reserve_despread_alloc(ofdm_rx* h, int64_t n_seg);
/* The stage.  Segment s is `rows` rows of row_len complex64 at d_sym + s*seg_stride; d_csi + s*csi_stride holds row_len channel
 * powers (d_csi == NULL: the plain inverse transforms); rho, the noise modes and `out` as ofdm_dft_despread_frames, the outputs in
 * the allocation-major layout above.  Asynchronous on `stream`.  The number of launches does not grow with n_alloc: one for the
 * table, then at most one per (M <= 2048 or not, modulation) pair present in the set -- one per size class when neither llr nor
 * bits is wanted.  Refused before anything is enqueued or any output touched: everything ofdm_dft_despread_frames refuses for
 * the same argument (per allocation), no allocation set, row_len < max(start + M), seg_stride < rows*row_len, csi_stride <
 * row_len, packed bits with an allocation whose bits do not fill bytes, index ranges (rows*row_len, the per-allocation rows*M_u,
 * n_seg*seg_stride, more than 2^31 - 1 workgroups), out->sym == d_sym (the layouts differ), growth inside a stream capture. */
int ofdm_dft_despread_alloc_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride,
                                   const float* d_csi, int64_t csi_stride, float rho, int32_t noise_mode, double noise_var,
                                   const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out, void* stream);
/* ofdm_rx_demod_frames_despread with the stage above in place of the single transform: ofdm_rx_demod_frames (d_eq required), then
 * ofdm_rx_csi_frames(OFDM_CSI_ROWS_ALL) into the workspace, then the stage with row_len = num_data_bins, one segment per frame
 * and rho from the handle.  Follows ofdm_rx_set_chan_window and ofdm_rx_set_chan_average like every ofdm_rx_demod_frames_* call.
 * Every check is made before anything is enqueued.  Returns n_dsym or a negative status. */
int64_t ofdm_rx_demod_frames_despread_alloc(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                            float* d_eq, int32_t* d_tsr, int32_t noise_mode, double noise_var, const double* d_sigma2,
                                            int32_t bits_mode, const ofdm_despread_out* out, void* stream);
/* Transform precoder over the transmitter's set: n_rows rows of row_len complex64 in, the same layout out, d_out == d_sym
 * allowed.  One launch per size class present (M <= 2048 or not).  Refused: no set, row_len < max(start + M), negative or
 * out-of-range counts, null buffers. */
int ofdm_tx_dft_spread_alloc(struct ofdm_tx* h, const float* d_sym, int64_t n_rows, int64_t row_len, float* d_out, void* stream);
/* Sizes the workspace of ofdm_tx_modulate_frames_alloc for n_rows data symbols (the buffers of ofdm_tx_reserve_spread, without a
 * plan) and loads the kernels.  Grows, never shrinks; synchronises the device. */
int ofdm_tx_reserve_spread_alloc(struct ofdm_tx* h, int64_t n_rows);
/* ofdm_tx_modulate_frames_spread with ofdm_tx_dft_spread_alloc (row_len = num_data_bins) in place of the single transform.  The
 * bits of entries outside every allocation are read and discarded.  Refused if there is no set or it does not fit
 * num_data_bins. */
int64_t ofdm_tx_modulate_frames_alloc(struct ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                                      float* d_iq, int64_t frame_stride, void* stream);

/* ------------------------------------------------------------------------------------------ receive diversity for multi-user allocations of DFT-spread OFDM
 * An extension the reference does not have: the base station's receiver, with B antennas and several users in every symbol.  It
 * is "receive diversity for DFT-spread OFDM" above with the allocation set of "multi-user allocations of DFT-spread OFDM" in
 * place of the single M.  (Combining first with ofdm_combine_csi_frames and despreading with ofdm_dft_despread_alloc_frames gives
 * wrong weights: beta and the noise behind the transform must come from the COMBINED channel of each user's own columns.)  This
 * text is the definition; tests/mrc_despread_alloc_ref.py restates it in NumPy (a loop over the allocations around
 * tests/mrc_despread_ref.py).
 *
 * The contract in one sentence: for every allocation u of the handle's set, block u of every output -- sym, llr, bits, beta,
 * weight and comb -- holds bit for bit what ofdm_combine_despread_frames writes for M = M_u and modulation = mod_u when given a
 * dense copy of columns start_u .. start_u+M_u-1 of every row of every branch, the same columns of every unit's d_csi row, the
 * same rho and the same noise.  Steps 1-7 of the receive-diversity-for-DFT-spread contract apply per allocation, word for word.
 * Entries outside every allocation are never read for data.
 *
 * Inputs, branch-major as ofdm_combine_despread_frames: unit g = b*n_seg + s is `rows` rows of row_len complex64 at
 * d_sym + g*seg_stride (complex items), with row_len channel powers (float32) at d_csi + g*csi_stride.  d_csi is required: the
 * combiner has no meaning without it.  Outputs: sym, comb, llr and bits are allocation-major and dense at the offsets
 * ofdm_alloc_layout returns (comb uses the sym offsets); beta and weight are per row, [n_alloc][n_seg][rows]: row r of segment s
 * of allocation u at (u*n_seg + s)*rows + r.
 * Noise: OFDM_MRC_NOISE_GIVEN (HOST array h_noise_var[n_branch]) and OFDM_MRC_NOISE_SEG (DEVICE doubles d_sigma2[n_branch*n_seg]).
 * A unit's variance is shared by all its allocations: it is the receiver's noise, not a user's.  OFDM_MRC_NOISE_EST is refused.
 * Position independence: a user's bits depend on (B, M_u) and its own columns alone.  They are the same in any batch, at any
 * start, at either alignment of every branch (alignment is decided per row and per branch; it alternates between rows where
 * row_len or start is odd and between branches where n_seg*seg_stride is odd), with any other users in the set, and on every
 * call. */
/* Sizes the {c, t} table of the stage for n_branch*n_seg*row_len entries and the |H|^2 rows of
 * ofdm_rx_demod_frames_mrc_despread_alloc for n_branch*n_seg*num_data_bins floats, and loads the kernels.  Needs no set: the
 * workspace does not depend on it, and the set is not copied into the plan cache.  Grows, never shrinks; synchronises the device.
 * After it the stage enqueues without host synchronisation or allocation and can be captured and replayed; inside a capture a
 * call that needs more is refused before anything is enqueued. */
int ofdm_rx_reserve_mrc_despread_alloc(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t row_len);
/* The stage on any device buffer, over the set ofdm_rx_set_allocations installed.  Asynchronous on `stream`: the combiner's table
 * over the whole rows, then at most one launch per (M <= 2048 or not, modulation) pair present in the set -- one per size class
 * when neither llr nor bits is wanted; the count does not depend on the number of users or branches.  n_seg == 0 or rows == 0
 * is a no-op.  Refusals are OFDM_ERR_INVALID with the reason in ofdm_last_error(), before anything is enqueued or any output
 * touched: everything ofdm_combine_despread_frames refuses, per allocation; everything ofdm_dft_despread_alloc_frames refuses for
 * the same argument (no set, row_len < max(start + M), seg_stride < rows*row_len, csi_stride < row_len, packed bits with an
 * allocation whose row bits do not fill bytes); index ranges (n_branch*n_seg > 2^31, more than 2^31 - 1 workgroups);
 * out->sym or out->comb equal to d_sym (the layouts differ); d_csi NULL; growth inside a stream capture. */
int ofdm_combine_despread_alloc_frames(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len,
                                       int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, int32_t noise_mode,
                                       const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                       const ofdm_mrc_despread_out* out, void* stream);
/* d_iq in the layout of ofdm_rx_demod_frames_mrc (frame f of branch b at index b*n_frames + f).  Runs ofdm_rx_demod_frames over
 * the n_branch*n_frames frames (d_eq required), then ofdm_rx_csi_frames(OFDM_CSI_ROWS_ALL) into the workspace, then the stage with
 * row_len = num_data_bins, one segment per frame and rho from the handle.  Follows ofdm_rx_set_chan_window and
 * ofdm_rx_set_chan_average like every ofdm_rx_demod_frames_* call.  d_sigma2 (OFDM_MRC_NOISE_SEG) is [n_branch*n_frames].  Every
 * check is made before anything is enqueued.  Returns n_dsym or a negative status. */
int64_t ofdm_rx_demod_frames_mrc_despread_alloc(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames,
                                                int64_t frame_stride, int64_t frame_len, float* d_eq, int32_t* d_tsr,
                                                int32_t noise_mode, const double* h_noise_var, const double* d_sigma2,
                                                int32_t bits_mode, const ofdm_mrc_despread_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ delay-window channel-estimate denoising
 * An extension the reference does not have.  The batch receiver's channel estimate is the least-squares (LS) estimate of ONE
 * Zadoff-Chu preamble symbol: as noisy as one received symbol.  A channel is shorter than the cyclic prefix, so nearly all of that
 * noise lies at delays where the channel has no energy: the stage transforms the estimate to the delay domain, keeps a window of
 * taps around tap 0 and transforms back (DFT-based denoising).  This text is the definition; tests/chanwin_ref.py restates it in
 * fp64 NumPy.  The library computes in float32 with an FFT whose operation order is its own: it agrees with the definition to
 * max|a - b| / max|b| < 1e-5 per output row (the bar of every FFT-based output of this library), not bit for bit.
 *
 * Per row (frame) with a sync (tsr[3] == 1), N = nfft, window (pre, post) with pre >= 0, post >= 1 and pre + post <= N:
 *  1. h = ifft_N(H_ls).  H_ls is the frame's est_chan_freq_P row: zero outside the sync bins, with the lag de-rotation already
 *     applied, so the energy sits around tap 0.
 *  2. Keep h[n] for n in [0, post) and [N - pre, N); set the other M = N - pre - post taps to zero.
 *  3. tail = (N / M) * sum over the discarded n of |h[n]|^2: float32, the order of the sum fixed by N alone, so the same bits alone,
 *     in any batch and on every call.  M == 0 gives tail = +0.
 *  4. H' = fft_N(the windowed h) on the sync bins binsP(num_synch_bins), +0 on every other bin.  (num_synch_bins == nfft lists
 *     bin N/2 twice; est_chan_freq_P holds one value there and so does H'.)
 *  5. gain[j], j over binsP(num_data_bins), = conj(H'[k]) / (|H'[k]|^2 + 1/snr_data) * e^{+j 2 pi d k / N} with d = tsr[1]: the
 *     expression ofdm_rx_demod_frames builds its equaliser gains with, taken from H'.
 *  6. A row without a sync is left exactly as it is -- no store to H' or gain -- and gets tail = +0.
 * THE WINDOW IS THE CALLER'S CHOICE.  post must cover the channel's delay spread, pre the timing ambiguity of the sync: the search
 * may lock onto a later path, and the earlier ones then sit at negative delays N - 1, N - 2, ...  On the two-path case of
 * tests/csi_cases.py the search sometimes takes the second path (3 taps late) and a window with pre <= 2 cuts the first path off there
 * and loses blocks that a window with pre >= 3 does not.  (cp/4, 3cp/4) is a reasonable start.
 * WHAT tail IS.  The discarded taps hold noise only, so tail estimates the noise of the LS estimate per bin -- relative to the
 * received preamble power, because the LS estimate is normalised by it: it reads about sigma^2 / (1 + sigma^2) for a signal of
 * unit power in noise of variance sigma^2, plus a leakage term from the bins that are zero in H_ls (DC and the guard bands; about
 * 0.014 at nfft 64, num_synch_bins 62).  It is not an absolute variance, but unlike the decision-directed estimates above it
 * involves no symbol decisions and does not collapse at low SNR; per unit it serves as OFDM_MRC_NOISE_SEG input.  With wide
 * guard bands (num_synch_bins well below nfft) the truncation also biases H' towards the band edges. */
/* The stage on any device buffer: n_rows rows of nfft complex64 at d_H_in, d_tsr [n_rows][4] int32 ({., lag d, ., sync found} as
 * ofdm_rx_demod_frames writes it).  d_H_out [n_rows][nfft] complex64 (d_H_out == d_H_in is allowed), d_gain_out
 * [n_rows][num_data_bins] complex64 and d_tail [n_rows] float32 may be NULL.  One launch, asynchronous on `stream` (NULL = the
 * handle's stream), no allocation.  OFDM_ERR_INVALID with the reason in ofdm_last_error(): pre < 0, post < 1, pre + post > nfft,
 * n_rows negative or above 2^31 - 1, d_H_in, d_tsr or d_H_out missing.  n_rows == 0 is a no-op. */
int ofdm_chan_window_frames(ofdm_rx* h, const float* d_H_in, const int32_t* d_tsr, int64_t n_rows, int32_t pre, int32_t post,
                            float* d_H_out, float* d_gain_out, float* d_tail, void* stream);
/* (0, 0) switches the stage off (the default); any other window must satisfy the rule above.  While it is on,
 * ofdm_rx_demod_frames runs the stage in place on its channel estimates and gains between its sync and its demod launch (timed
 * with the sync leg of ofdm_rx_set_profiling): d_eq, the hard bits, ofdm_rx_get_frame_state and ofdm_rx_csi_frames -- and with
 * them every ofdm_rx_demod_frames_* call -- see the refined estimate.  While it is off that call issues exactly the launches it
 * issued before.  The setting is read when ofdm_rx_demod_frames is called: a captured graph keeps the window it was captured
 * with.  The stream block (ofdm_rx_work) is not affected. */
int ofdm_rx_set_chan_window(ofdm_rx* h, int32_t pre, int32_t post);
/* d_sigma2[f] = double(tail of frame f) of the LAST ofdm_rx_demod_frames call on this handle, f < n_frames: the layout
 * OFDM_MRC_NOISE_SEG takes (frames of a branch-major batch are its units).  One launch, asynchronous on `stream`.
 * OFDM_ERR_INVALID if the window was off in that call or n_frames exceeds its count. */
int ofdm_rx_chan_noise_frames(ofdm_rx* h, int64_t n_frames, double* d_sigma2, void* stream);

/* ------------------------------------------------------------------------------------------ channel estimate averaged over every sync symbol of a frame
 * An extension the reference does not have.  A frame holds n_pat = floor(floor(frame_len / L) / (S + D)) patterns (L = nfft + cp,
 * S, D = synch_dat) and every pattern begins with a sync symbol; the batch receiver takes its LS estimate from the first one
 * alone.  This stage takes one LS estimate per pattern, turns each onto the phase of the first and averages them: the time
 * direction of channel estimation, where the delay window above is the frequency direction.  This text is the definition;
 * tests/chanavg_ref.py restates it in fp64 NumPy.  The library computes in float32 with an FFT whose operation order is its own:
 * it agrees with the definition to max|a - b| / max|b| < 1e-5 per output row, not bit for bit.
 *
 * Preconditions: synch_S == 1.  Every num_synch_bins the handle accepts is supported; num_synch_bins == nfft lists bin N/2
 * twice, and as in the batch receiver's own estimate the bin keeps its last (positive-half) list entry while the power sum E_p
 * counts both entries.  Every other sum over k below runs over the distinct sync bins.
 *
 * Per frame with a sync (tsr[3] == 1), t0 = tsr[0], lag d = tsr[1], N = nfft, SD = S + D, Ks = num_synch_bins.  n_avg >= 1 or -1
 * (all); P = min(n_avg, n_pat) patterns p = 0 .. P - 1 are considered:
 *  1. The window of pattern p starts at w_p = t0 + L * SD * p (64-bit): the CP-stripped sync symbol in front of the pattern's data.
 *  2. It is a candidate iff 0 <= w_p and w_p + N <= frame_len: a sync symbol is never zero-padded.
 *  3. Y_p = fft_N(x[w_p : w_p + N]); y_p = Y_p on binsP(num_synch_bins).
 *  4. E_p = sum |y_p|^2.  The pattern takes part iff E_p is finite and > 0.
 *  5. a_p[k] = sqrt(Ks / E_p) * y_p[k] * e^{+j 2 pi d k / N} * conj(zc[k]) / (1 + 1/snr_ls): for p = 0 the row
 *     ofdm_rx_demod_frames writes without the stage.
 *  Phase alignment.  c_p = sum_k a_p[k] conj(a_0[k]); u_p = c_p / |c_p| if |c_p| is finite and > 0, else the pattern does not
 *  take part; u_0 = 1 + 0j.  (A carrier offset turns every later sync symbol by a common phase; the average stays referred to
 *  pattern 0, the phase the demod kernel's gains assume.)
 *  Mean.  n = the patterns that take part.  Pattern 0 always does for a frame the sync search accepted; if it does not (a
 *  hostile d_tsr in the stand-alone call) the row is treated as a row without a sync.  d_p = conj(u_p) a_p - a_0;
 *  Hbar = a_0 + (sum_p d_p) / n on the sync bins, +0 on every other bin.
 *  Spread.  spread = (sum_p sum_k |d_p[k]|^2 - sum_k |sum_p d_p[k]|^2 / n) / ((n - 1) Ks) for n >= 2, +0 for n < 2: the per-bin
 *  variance of ONE LS estimate about the frame's mean, relative to the received preamble power -- the units of the delay
 *  window's tail without its leakage term, so it serves as OFDM_MRC_NOISE_SEG input.
 *  Gains.  gain[j], j over binsP(num_data_bins), = conj(Hbar[k]) / (|Hbar[k]|^2 + 1/snr_data) * e^{+j 2 pi d k / N}.
 *  Outputs per frame: Hbar [N] complex64, gain [num_data_bins] complex64, spread float32, n_used int32 = n, rot [P] complex64 =
 *  u_p (+0+0j for a pattern that did not take part).  A row without a sync gets no store to Hbar or gain, spread = +0,
 *  n_used = 0 and rot all +0.
 *  Order of the sums.  Patterns are cut into chunks of OFDM_CHANAVG_CHUNK consecutive p.  Inside a chunk the sums over p run in
 *  ascending p from +0 and a pattern that does not take part leaves them as they are; chunk sums are added in ascending chunk
 *  order; sums over bins have a fixed order of their own.  The chunking depends on P and N alone: a frame gives the same bits
 *  alone, in any batch and on every call.
 * The angle of rot[p+1] * conj(rot[p]) divided by 2 pi SD L / N is the frame's carrier offset in subcarrier spacings; the stage
 * does not correct it.  A channel that changes within a frame is what n_avg is for: the average covers the first n_avg patterns. */
#define OFDM_CHANAVG_CHUNK 16
/* The stage on any device IQ buffer: frame f at d_iq + 2 * f * frame_stride floats, d_tsr [n_frames][4] int32 as
 * ofdm_rx_demod_frames writes it.  d_H_out [n_frames][nfft] complex64, d_gain_out [n_frames][num_data_bins] complex64, d_spread
 * [n_frames] float32, d_n_used [n_frames] int32 and d_rot [n_frames][P] complex64 may each be NULL, but not all of them.  Two
 * launches, asynchronous on `stream` (NULL = the handle's stream).  The chunk partials live in a workspace on the handle
 * (ofdm_rx_reserve_chan_average); a call that needs a larger one grows it, which synchronises and is refused inside a stream
 * capture.  OFDM_ERR_INVALID with the reason in ofdm_last_error(): null handle, synch_S != 1, n_avg of 0 or below -1, negative
 * counts, n_frames above 2^31 - 1, frame_stride < frame_len, d_iq or d_tsr missing, no output wanted.  n_frames == 0 is a no-op. */
int ofdm_chan_average_frames(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             const int32_t* d_tsr, int32_t n_avg, float* d_H_out, float* d_gain_out, float* d_spread,
                             int32_t* d_n_used, float* d_rot, void* stream);
/* 0 switches the stage off (the default); n_avg >= 1 or -1 (all patterns) switches it on, below -1 is OFDM_ERR_INVALID and so is
 * switching it on with synch_S != 1.  While it is on, ofdm_rx_demod_frames runs the stage in place on its channel estimates and
 * gains between its sync launch and the delay window (timed with the sync leg of ofdm_rx_set_profiling): d_eq, the hard bits,
 * ofdm_rx_get_frame_state, ofdm_rx_csi_frames, the delay window -- and with them every ofdm_rx_demod_frames_* call -- see the
 * averaged estimate.  While it is off that call issues exactly the launches it issued before.  The setting is read when
 * ofdm_rx_demod_frames is called: a captured graph keeps the setting it was captured with.  The stream block (ofdm_rx_work), the
 * CFO receiver and the tracker are not affected. */
int ofdm_rx_set_chan_average(ofdm_rx* h, int32_t n_avg);
/* Workspace for the chunk partials of n_frames frames of frame_len samples (all patterns), outside a stream capture; never
 * shrinks.  With ofdm_rx_reserve before it, a first averaged ofdm_rx_demod_frames inside a capture has nothing left to set up. */
int ofdm_rx_reserve_chan_average(ofdm_rx* h, int64_t n_frames, int64_t frame_len);
/* d_sigma2[f] = double(spread of frame f) of the LAST ofdm_rx_demod_frames call on this handle, f < n_frames: the layout
 * OFDM_MRC_NOISE_SEG takes.  One launch, asynchronous on `stream`.  OFDM_ERR_INVALID if the stage was off in that call or
 * n_frames exceeds its count. */
int ofdm_rx_chan_spread_frames(ofdm_rx* h, int64_t n_frames, double* d_sigma2, void* stream);

/* ------------------------------------------------------------------------------------------ channel tracked across the sync symbols of a frame
 * An extension the reference does not have.  The batch receiver equalises every data symbol of a frame with ONE channel estimate;
 * the delay window and the average above refine that one estimate and assume with it that the channel stands still for the whole
 * frame.  This stage drops the assumption: it takes one LS estimate per sync symbol and equalises every data symbol with an
 * estimate interpolated in time between the sync symbols around it.  This text is the definition; tests/chantrack_ref.py restates
 * it in fp64 NumPy.  The library computes in float32 with an FFT whose operation order is its own: it agrees with the definition
 * to max|a - b| / max|b| < 1e-5 per output row, not bit for bit.
 *
 * Precondition: synch_S == 1.  Every num_synch_bins / num_data_bins pair the handle accepts is supported; num_synch_bins == nfft
 * lists bin N/2 twice, with the rule the averaging section states (and so does num_data_bins == nfft: P_s counts both entries
 * and both list entries of the output row hold the bin's value).
 *
 * N = nfft, L = N + cp, SD = S + D, Ks = num_synch_bins, Kd = num_data_bins.  Per frame with a sync (tsr[3] == 1), t0 = tsr[0],
 * lag d = tsr[1], n_pat = floor(floor(frame_len / L) / SD) patterns:
 *  1. Per-pattern estimates.  For every p < n_pat, a_p is formed exactly as in steps 1-5 of the averaging section: the window
 *     starts at w_p = t0 + L * SD * p, is a candidate iff 0 <= w_p and w_p + N <= frame_len (never zero-padded), E_p is summed
 *     over the sync-bin list, the pattern TAKES PART iff E_p is finite and > 0, and
 *     a_p[k] = sqrt(Ks / E_p) * y_p[k] * e^{+j 2 pi d k / N} * conj(zc[k]) / (1 + 1/snr_ls) on the sync bins, +0 elsewhere.
 *     There is NO phase alignment: the estimates keep their own phase, and following it is the point of the stage.  If pattern 0
 *     does not take part the frame is treated as a frame without a sync.
 *  2. Optional delay window.  With a window (pre, post) != (0, 0), every a_p that takes part is replaced by H' of steps 1-4 of
 *     the delay-window section applied to that row; (0, 0) means off; the rule for valid windows is that section's.
 *  3. Neighbours and weight.  Data symbol m (0 <= m < D) of pattern p has the symbol index s = p * SD + S + m.  lo = the largest
 *     q <= p that takes part (pattern 0 does); hi = the smallest q > p that takes part, if there is one.
 *     OFDM_TRACK_LINEAR: w = float32(s - lo * SD) / float32((hi - lo) * SD), H = a_lo + w (a_hi - a_lo); without a hi H = a_lo
 *     (no extrapolation past the last sync symbol).  OFDM_TRACK_HOLD: H = a_lo always.
 *  4. Demodulation, with the windows and the guard of ofdm_rx_demod_frames: ptr_p = t0 + L * (p * SD + 1); pattern p is
 *     demodulated iff ptr_p + N - 1 <= frame_len, otherwise its D rows are zeros.  Symbol m starts at ptr_p + L * m, samples
 *     outside [0, frame_len) read as zero like fft(x, N); Y = fft_N; P_s = sum |Y[k]|^2 over the list binsP(Kd);
 *     z_j = Y[k] * sqrt(Kd / P_s) * conj(H[k]) / (|H[k]|^2 + 1/snr_data) * e^{+j 2 pi d k / N}, j over binsP(Kd) in list order.
 *     A non-finite or zero P_s gives what IEEE arithmetic of these formulas gives.
 *  5. Outputs per frame, each optional but not all:
 *       eq    [n_pat*D][Kd] complex64
 *       bits  the hard decision, by the rules of ofdm_demap, of the STORED float32 eq values, zero rows included; modulation =
 *             cfg.modulation; packed MSB-first [n_pat*D*Kd*bps/8] bytes or one bit per byte
 *       csi   [n_pat*D][Kd] float32 = re*re + im*im of H[k] (each product rounded) for EVERY data symbol of the frame, whether
 *             its pattern is demodulated or not: ofdm_demap_csi_frames with one ROW per segment (n_seg = n_frames*n_pat*D,
 *             rows = 1, csi_stride = Kd) weighs every symbol with its own channel power
 *       H_pat [n_pat][N] complex64 = a_p after step 2, +0 rows for patterns that do not take part
 *       takes [n_pat] int32, 1 or 0
 *     A frame without a sync gets zero rows in eq, the bits of zeros, +0 in csi and H_pat and 0 in takes.
 *  6. Every symbol is computed on its own in a fixed order: a frame gives the same bits alone, in any batch, at any buffer
 *     alignment and on every call. */
typedef enum { OFDM_TRACK_HOLD = 0, OFDM_TRACK_LINEAR = 1 } ofdm_track_mode;
typedef struct ofdm_track_out {      /* DEVICE pointers; NULL = not wanted */
    float*   eq;
    uint8_t* bits;
    float*   csi;
    float*   H_pat;
    int32_t* takes;
} ofdm_track_out;
/* The stage on any device IQ buffer: frame f at d_iq + 2 * f * frame_stride floats, d_tsr [n_frames][4] int32 as
 * ofdm_rx_demod_frames writes it.  Asynchronous on `stream` (NULL = the handle's stream): the estimate launch, a small launch
 * that links every pattern to its neighbours, the delay-window launch over the n_frames * n_pat rows if a window is given, the
 * demod launch if eq, bits or csi is wanted and a hard-decision launch over the stored rows if bits is.  The flags, the
 * neighbours and -- for a call that does not take H_pat -- the rows a_p live in a workspace on the handle
 * (ofdm_rx_reserve_chan_track); a call that needs a larger one grows it, which synchronises and is refused inside a stream
 * capture, before anything is enqueued.  bits without eq keeps the equalised rows in a second workspace that grows on demand
 * only, outside a capture.  Returns n_pat*D or a negative status.  OFDM_ERR_INVALID with the reason in
 * ofdm_last_error(), before anything is enqueued: null handle, synch_S != 1, an unknown mode, a window that is neither (0, 0)
 * nor valid, an unknown bits_mode, bits wanted with OFDM_BITS_NONE (or packed bits the numerology cannot pack), negative counts,
 * frame_stride < frame_len, a batch beyond the kernels' index range, d_iq or d_tsr missing, an `out` without any pointer.
 * n_frames == 0 is a no-op that returns the row count. */
int64_t ofdm_chan_track_frames(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                               const int32_t* d_tsr, int32_t mode, int32_t pre, int32_t post, int32_t bits_mode,
                               const ofdm_track_out* out, void* stream);
/* The sync search of ofdm_rx_demod_frames (the same d_tsr bits; d_tsr may be NULL), then the stage with the window of
 * ofdm_rx_set_chan_window.  The call runs the handle's sync launch ONLY: the averaging setting (ofdm_rx_set_chan_average) is
 * not applied here -- it is the opposite assumption -- and the handle's per-frame state (ofdm_rx_get_frame_state,
 * ofdm_rx_csi_frames) stays as the sync launch wrote it, without the window.  The window and the mode are read when the call is
 * made: a captured graph keeps them.  Refusals as above. */
int64_t ofdm_rx_demod_frames_track(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                   int32_t mode, int32_t bits_mode, int32_t* d_tsr, const ofdm_track_out* out, void* stream);
/* Workspace of the stage for n_frames frames of frame_len samples (n_frames * n_pat rows of nfft complex64, the flags, the
 * neighbours and the row tsr of the window launch: what a call without H_pat needs; a call that takes H_pat allocates no rows
 * of its own), outside a stream capture; never shrinks; loads the kernels.  With
 * ofdm_rx_reserve before it, a first ofdm_rx_demod_frames_track inside a capture has nothing left to set up. */
int ofdm_rx_reserve_chan_track(ofdm_rx* h, int64_t n_frames, int64_t frame_len);

/* ------------------------------------------------------------------------------------------ TX
 * Replaces MultiAntennaSystem.multi_ant_binary_map + multi_ant_symb_gen (single antenna)
 * (G/LEGACY/gr-ofdm-rx/python/txrx_mod/MultiAntennaSystem.py:113-218) and SynchSignal (:13-30). */
typedef struct {
    int32_t nfft, cp_len, num_synch_bins, num_data_bins, synch_S, synch_D;
    int32_t modulation;        /* ofdm_modulation */
    int32_t zc_root;           /* 23 (SynchSignal.py:23) */
    int32_t device;
    int32_t reserved;
} ofdm_tx_cfg;

typedef struct ofdm_tx ofdm_tx;

int ofdm_tx_create(const ofdm_tx_cfg* cfg, ofdm_tx** out);
int ofdm_tx_destroy(ofdm_tx* h);

/* bits -> time-domain IQ.  Each frame has n_sym symbols laid out back to back (symbol s is a sync
 * symbol iff s % (S+D) < S); frame f is written at d_iq[f*frame_stride ..] (n_sym*(nfft+cp) items).
 * d_bits: per frame n_data_sym*Kd*bps bits, one per byte (bits_mode UNPACKED) or MSB-first packed. */
int ofdm_tx_modulate_frames(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames,
                            int32_t n_sym, float* d_iq, int64_t frame_stride, void* stream);

/* ---- decomposed transmitter stages.  The reference names these blocks only in a flowgraph --
 * txOFDM_random_bit_source -> txOFDM_ConstellationModulation(modulation) -> txOFDM_OFDM_Modulation(fft_size, pilot_locations)
 * -> txOFDM_IFFT(fft_size) -> txOFDM_CyclicPrefix(fft_size, cp_size) -> txOFDM_SynchDataMux(fft_size, cp_size, prime_no,
 * synch_every, synch_length)  (G/LEGACY/gr-ofdm-tx/grc/RXtransmit_6.grc:701-975, connections :1819-1854) -- and holds no
 * code for them.  Each stage is the corresponding slice of MultiAntennaSystem.multi_ant_binary_map / multi_ant_symb_gen
 * (:150-218) on device buffers; chained they equal ofdm_tx_modulate_frames bit for bit (the kernels share their device
 * functions).  The handle's cfg supplies the numerology: modulation (map), nfft / num_data_bins (grid), cp_len (CP),
 * num_synch_bins / zc_root / synch_S / synch_D (mux: S sync symbols before every D = synch_every data symbols). */
/* random_bit_source: n_bits bits, one per byte, of a counter-based stream: bit k = bit (k%32) of word (k/32)%4 of
 * Philox4x32-10(counter = k/128, key = seed); the window [offset, offset+n_bits) is produced (a stream block advances offset). */
int ofdm_tx_random_bits(ofdm_tx* h, uint64_t seed, uint64_t offset, uint8_t* d_bits, int64_t n_bits, void* stream);
/* ConstellationModulation: n_symbols * bps bits (MSB first per symbol; bits_mode as above) -> n_symbols complex64 (:150-178). */
int ofdm_tx_map(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_symbols, float* d_sym, void* stream);
/* pilot_locations of OFDM_Modulation: signed bin offsets (e.g. -21,-7,7,21) inside the occupied span
 * binsP(num_data_bins + n_pilots); those bins carry pilot_re + j pilot_im, the data symbols fill the other occupied bins in
 * list order.  n_pilots = 0 (default) gives the reference grid (:182-183).  Host array, copied; synchronises the device. */
int ofdm_tx_set_pilots(ofdm_tx* h, const int32_t* h_locations, int32_t n_pilots, float pilot_re, float pilot_im);
/* OFDM_Modulation: d_sym [n_rows][num_data_bins] -> d_grid [n_rows][nfft] (unused bins and DC zero) (:135-183). */
int ofdm_tx_grid(ofdm_tx* h, const float* d_sym, int64_t n_rows, float* d_grid, void* stream);
/* IFFT (do_ifft=1, add_cp=0): [n_rows][nfft] grid rows -> [n_rows][nfft] time samples, numpy.fft.ifft scaling (:199).
 * CyclicPrefix (0,1): [n_rows][nfft] time samples -> [n_rows][nfft+cp] CP-extended symbols, power-normalised as :200-218.
 * (1,1): both in one launch. */
int ofdm_tx_ifft_cp(ofdm_tx* h, const float* d_in, int64_t n_rows, int32_t do_ifft, int32_t add_cp, float* d_out, void* stream);
/* SynchDataMux: d_data [n_data_sym][nfft+cp] -> d_out: synch_S Zadoff-Chu sync symbols in front of every synch_D data symbols
 * (a trailing partial pattern keeps its sync symbols).  Returns the number of OUTPUT symbols
 * (n/D*(S+D) + (n%D ? S + n%D : 0)) or a negative ofdm_status; d_out must hold that many symbols. */
int64_t ofdm_tx_mux(ofdm_tx* h, const float* d_data, int64_t n_data_sym, float* d_out, void* stream);
/* the sync symbol(s) the mux inserts: h_sync_time [synch_S][nfft+cp] complex64 */
int ofdm_tx_get_sync_symbol(ofdm_tx* h, float* h_sync_time);

/* Loop-back channel (MultiAntennaSystem.py:221-260): y = x (*) taps (taps used as given; the
 * reference normalises to unit norm first, :86) + complex AWGN of variance noise_var (Philox
 * counter-based, reproducible from `seed`).  Per frame: in_len input samples, out_len outputs
 * (out_len <= in_len + n_taps - 1, the rest of the convolution tail is dropped).
 * d_taps: [n_taps] complex64, or [n_frames][n_taps] when per_frame_taps != 0.
 * Frame f reads d_in + f * in_stride and writes out_len samples at d_out + f * out_stride (strides in complex samples,
 * in_stride >= in_len, out_stride >= out_len; nothing else of d_out is written).  1 <= n_taps, 0 <= n_frames <= 65535;
 * n_frames = 0 or out_len = 0 is OK and does nothing.
 *
 * The noise is a contract: a sample's noise depends only on (seed, frame index f within the call, sample index n within the
 * frame) -- not on addresses, strides, out_len or the launch.  With the pair index p = n / 2 and the four words
 *     w[0..3] = Philox4x32-10(counter = (p & 0xFFFFFFFF, p >> 32, f, 0), key = (seed & 0xFFFFFFFF, seed >> 32)),
 * sample 2p takes (w[0], w[1]) and sample 2p + 1 takes (w[2], w[3]) as (radius word, angle word).  A word becomes
 *     u = (float(w) + 0.5f) * 2^-32      in float32 (u in (0, 1]; the conversion rounds to nearest even),
 * and the noise of the sample is  sigma * sqrt(-2 ln u_radius) * exp(2 pi j u_angle),  sigma = sqrtf(noise_var / 2) in float32.
 * The device evaluates log, sqrt, sin and cos with its float32 hardware instructions: against the same expression in double
 * it was measured within 8e-7 sigma (tests/channel_ref.py restates this text; tests/test_gpu_channel_edges.py holds every
 * sample against it).  noise_var = 0 adds nothing. */
int ofdm_channel_apply(ofdm_tx* h, const float* d_in, int64_t n_frames, int64_t in_stride, int64_t in_len,
                       const float* d_taps, int32_t n_taps, int32_t per_frame_taps, float noise_var,
                       uint64_t seed, float* d_out, int64_t out_stride, int64_t out_len, void* stream);

/* ------------------------------------------------------------------------------------------ channel code (LTE TBCC)
 * The tail-biting convolutional code of 3GPP TS 36.212 5.1.3.1 on the frame-batched path: an encoder in front of
 * ofdm_tx_modulate_frames and a decoder behind the LLRs of ofdm_demap_frames / ofdm_rx_demod_frames_soft /
 * ofdm_rx_demod_frames_pilots.  An extension: the reference has no channel code, so this text is the contract.  The calls of
 * this block use the plain interleaving below at rate 1/3; the sub-block interleaver and the circular-buffer rate matching of
 * 5.1.4.2 are the ofdm_*_rm_* calls of the next block, which leave these calls as they are.
 * Code block: K information bits c[0..K), K a multiple of 8 with 24 <= K <= 2048; indices are taken mod K (tail-biting: the
 * register starts in the state of the last six bits).
 * Encoder:  d0[k] = c[k]^c[k-2]^c[k-3]^c[k-5]^c[k-6]   (generator 133 octal)
 *           d1[k] = c[k]^c[k-1]^c[k-2]^c[k-3]^c[k-6]   (171)
 *           d2[k] = c[k]^c[k-1]^c[k-2]^c[k-4]^c[k-6]   (165)          e[3k+j] = dj[k]: 3K coded bits.
 * Segments: a segment is one frame's bit stream of seg_bits bits (receiver: n_dsym*Kd*bps, with pilots n_dsym*Kd'*bps;
 * transmitter: the n_data_sym*Kd*bps bits ofdm_tx_modulate_frames takes per frame).  It carries blocks_per_seg <=
 * floor(seg_bits/(3K)) blocks back to back from bit 0; the encoder writes the rest of the segment as zeros (filler), the
 * decoder ignores it.
 * Decoder: wrap-around Viterbi, non-iterative, fully determined; all arithmetic IEEE float32 in the order written.
 *   state s = sum_{i=1..6} c[k-i] 2^(6-i); input b takes s to s' = (b<<5)|(s>>1); the predecessors of s' are p0 = (s'<<1)&63 and
 *   p1 = p0|1; output bit j of the transition p -> s' is parity((((s'>>5)<<6) | p) & Gj), G = 0133, 0171, 0165 (bit 6 = input).
 *   An LLR that is not finite counts as 0; positive favours bit 0 (the convention of ofdm_soft_out.llr).
 *   W = 96, T = K + 2W steps; step t uses the LLRs l0, l1, l2 of information index (t - W) mod K; all 64 start metrics are 0.
 *   Per state s': bm = (sg0*l0 + sg1*l1) + sg2*l2, sgj = +1 where output bit j of the p0 branch is 0, -1 where it is 1 (the p1
 *   branch has all three bits flipped -- every generator taps delay 6 -- so its metric is exactly -bm);
 *   cand0 = pm[p0] + bm, cand1 = pm[p1] - bm, decision = (cand1 > cand0) (a tie takes p0), pm'[s'] = the chosen candidate.
 *   No renormalisation: finite LLRs whose sums overflow float32 are outside the contract.
 *   After step T-1 the end state is the one with the largest metric, the lowest index on a tie.  Traceback t = T-1 .. 0:
 *   bit[t] = s_{t+1} >> 5, s_t = ((s_{t+1} << 1) & 63) | decision[t][s_{t+1}].
 *   Outputs per block: the bits of steps W .. W+K-1; metric = the end state's path metric; tb_ok = 1 iff s_W == s_{W+K} (a
 *   consistency diagnostic, not an error detector).
 * Deterministic: a block's outputs depend on its own 3K LLRs only -- the same bits alone, in any batch, at any stride and on
 * every call (no atomics). */
/* floor(seg_bits / (3K)): the blocks a segment can carry.  Host arithmetic; OFDM_ERR_INVALID for a bad K or seg_bits < 0. */
int64_t ofdm_tbcc_blocks(int64_t seg_bits, int32_t K);
/* d_info: dense [n_seg][blocks_per_seg][K] information bits, d_coded: [n_seg][seg_bits] coded bits + filler; each side packed
 * MSB-first or one bit per byte (ofdm_bits_mode; packed coded output needs seg_bits % 8 == 0).  Asynchronous on `stream`
 * (NULL = the handle's stream), one launch, no allocation.  n_seg == 0 or seg_bits == 0 is a no-op; argument errors return
 * OFDM_ERR_INVALID before anything is enqueued. */
int ofdm_tx_tbcc_encode_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                               int32_t K, uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream);
typedef struct ofdm_tbcc_out {   /* DEVICE pointers; NULL = not wanted */
    uint8_t* bits;       /* dense [n_seg][blocks_per_seg][K] decoded bits: packed MSB-first (K/8 bytes per block) or one per byte */
    int32_t  bits_mode;  /* ofdm_bits_mode of bits                                                                             */
    float*   metric;     /* [n_seg][blocks_per_seg] float32                                                                    */
    int32_t* tb_ok;      /* [n_seg][blocks_per_seg]                                                                            */
} ofdm_tbcc_out;
/* Prepares the handle's device for decoding up to n_blocks blocks of K bits per call: the decoder keeps its survivors in LDS and
 * needs no device workspace, so this checks the geometry and loads the kernels.  Call it before capturing ofdm_tbcc_decode_frames
 * or ofdm_tbcc_decode_rm_frames into a hipGraph. */
int ofdm_rx_reserve_tbcc(ofdm_rx* h, int64_t n_blocks, int32_t K);
/* Block (s, b) reads the 3K float32 LLRs at d_llr + s*seg_stride + b*3K (seg_stride in floats, >= blocks_per_seg*3K), so the
 * call works on any LLR buffer.  Asynchronous on `stream` (NULL = the handle's stream): one launch, no host synchronisation and
 * no allocation.  n_seg == 0, blocks_per_seg == 0 or an `out` without any pointer is a no-op returning OFDM_OK.  Argument errors
 * (NULL handle, bad K, seg_stride too short, a negative count, a batch beyond the kernel's index range) return OFDM_ERR_INVALID
 * before anything is enqueued and without touching the device. */
int ofdm_tbcc_decode_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, int32_t K,
                            const ofdm_tbcc_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ rate matching (LTE TBCC)
 * The sub-block interleaver and the circular buffer of TS 36.212 5.1.4.2 around the code above: E rate-matched bits per block
 * in place of the 3K of e[3k+j] (puncturing for E < 3K, repetition for E > 3K), on the transmit side as an encoder of its own and
 * on the receive side as a de-matching stage and as a decoder that de-matches while it loads.  An extension like the code
 * itself: this text is the contract.
 * K as above (D = K); 1 <= E <= 48K (at most 16 copies of a coded bit; PBCH's 1920 / 120 is exactly 16).  R = ceil(K / 32),
 * ND = 32R - K.
 * Sub-block interleaver: each stream dj, prefixed with ND NULLs, is written row by row into an R x 32 matrix; column c of the
 *   permuted matrix is column P[c] of it, P = <1,17,9,25,5,21,13,29,3,19,11,27,7,23,15,31,0,16,8,24,4,20,12,28,2,18,10,26,6,22,14,30>
 *   (P[c] is the 5-bit reversal of (c + 16) mod 32); the permuted matrix read column by column is vj, 32R entries.
 * Circular buffer: w = v0 | v1 | v2; e_k, k = 0 .. E-1, walks w cyclically from index 0 and skips the NULLs (k0 = 0: the
 *   convolutionally coded channels have no other start).
 * Closed form: nullmask has bit c set iff P[c] < ND.  Coded bit dj[i] has y = ND + i, row = y >> 5, c = P^-1[y & 31] and the
 *   rank  q = j K + c R + row - popcount(nullmask & ((2 << c) - 1)),  0 <= q < 3K;  e_k = the coded bit of rank k mod 3K.
 *   The other way: cum(c) = c R - popcount(nullmask & ((1 << c) - 1)); inside stream j, c is the largest column with
 *   cum(c) <= rank, row = rank - cum(c) + [P[c] < ND], i = 32 row + P[c] - ND.  E = 3K is a permutation of the 3K coded bits.
 * Segments: as above with E in place of 3K -- block b has its coded bits at segment bit b*E and its LLRs at
 *   d_llr + s*seg_stride + b*E; blocks_per_seg*E <= seg_bits (encoder), seg_stride >= blocks_per_seg*E (receive side); filler
 *   zeros follow the last block.  E need not be a multiple of 8: packed blocks may start inside a byte.
 * De-matching, IEEE float32 in this order: v(x) = x if x is finite, else 0.  For rank q: L = +0 if q >= E (punctured), else
 *   L = v(l[q]) and then L = L + v(l[q + m 3K]) for m = 1, 2, .. while the index is < E, in increasing m.  The decoder uses
 *   v(L) -- a sum that overflowed counts as 0, as any input that is not finite does -- and is the decoder above from there on.
 * Deterministic: a block's outputs depend on its own E LLRs only (no atomics). */
/* floor(seg_bits / E): the blocks a segment can carry.  Host arithmetic; OFDM_ERR_INVALID for a bad K, E or seg_bits < 0. */
int64_t ofdm_tbcc_rm_blocks(int64_t seg_bits, int32_t K, int32_t E);
/* ofdm_tx_tbcc_encode_frames with E rate-matched bits per block; the same layouts, rules and errors (seg_bits >= blocks_per_seg*E). */
int ofdm_tx_tbcc_encode_rm_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                                  int32_t K, int32_t E, uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream);
/* De-matching alone: d_out[s*out_stride + b*3K + 3i + j] = L of dj[i] (out_stride in floats, >= blocks_per_seg*3K), the layout
 * ofdm_tbcc_decode_frames reads.  L is stored as summed (an overflowed sum as +-inf, a single -0 as -0).  Asynchronous, one
 * launch, no allocation; n_seg == 0 or blocks_per_seg == 0 is a no-op; argument errors as below. */
int ofdm_tbcc_rate_dematch_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                                  int32_t K, int32_t E, float* d_out, int64_t out_stride, void* stream);
/* ofdm_tbcc_decode_frames on rate-matched LLRs, de-matched while they are loaded: one launch and no 3K-float intermediate; the
 * outputs are those of ofdm_tbcc_rate_dematch_frames followed by ofdm_tbcc_decode_frames, bit for bit.  The same rules as
 * ofdm_tbcc_decode_frames (ofdm_rx_reserve_tbcc prepares this call too); OFDM_ERR_INVALID before anything is enqueued for a NULL
 * handle, a bad K, E outside 1 .. 48K, seg_stride < blocks_per_seg*E, a negative count or a batch beyond the index range. */
int ofdm_tbcc_decode_rm_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                               int32_t K, int32_t E, const ofdm_tbcc_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ CRC and scrambling (LTE)
 * The bit-level stages around the code above, TS 36.212 5.1.1 and TS 36.211 7.2, which close the chain on the device:
 *   transmit: payload -> ofdm_tx_crc_attach_frames -> ofdm_tx_tbcc_encode(_rm)_frames -> ofdm_tx_scramble_frames ->
 *             ofdm_tx_modulate_frames;
 *   receive:  LLRs -> ofdm_descramble_llr_frames -> ofdm_tbcc_decode(_rm)_frames -> ofdm_crc_check_frames -> one ok byte and
 *             one syndrome word per block.
 * An extension like the code itself: this text is the contract.
 * CRC: generators gCRC24A = 0x1864CFB, gCRC24B = 0x1800063 (L = 24), gCRC16 = 0x11021 (L = 16), gCRC8 = 0x19B (L = 8), bit L on
 *   top.  Systematic: with the payload a_0 .. a_{A-1} and the parity p_0 .. p_{L-1}, the polynomial a_0 D^{A+L-1} + .. + a_{A-1} D^L
 *   + p_0 D^{L-1} + .. + p_{L-1} is divisible by g; the register starts at zero, nothing is reflected, there is no final XOR.
 *   A block is the A payload bits followed by L parity bits, K = A + L; A is a multiple of 8 with 8 <= A <= 2040 and K <= 2048.
 *   The parity read as an L-bit integer (p_0 the most significant bit) is XORed with a mask of L bits -- for PDCCH the RNTI
 *   (x_rnti,0 = MSB, 5.3.3.2), for PBCH the antenna mask.  The mask is the scalar `mask`, or with d_mask != NULL one uint32 per
 *   block on the device (the scalar is then not used).  A scalar mask in use with bits at or above L is OFDM_ERR_INVALID; in a
 *   device mask those bits are ignored.
 *   Bit layouts are those of the TBCC calls: OFDM_BITS_PACKED is MSB-first, OFDM_BITS_UNPACKED is one bit per byte of which only
 *   bit 0 is read; written bytes are 0 or 1.  Blocks are dense: [n_blocks][K] or [n_blocks][K/8], what
 *   ofdm_tx_tbcc_encode(_rm)_frames reads and the decoders write.
 * Scrambling: c(n) = x1(n + 1600) ^ x2(n + 1600), x1(n + 31) = x1(n + 3) ^ x1(n) with x1(0) = 1 and x1(1 .. 30) = 0,
 *   x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n) with x2(i) = bit i of c_init, i < 31.  One sequence per segment, from
 *   the segment's bit 0; c_init of segment s is d_cinit[s] on the device (bit 31 is ignored, 0 is allowed), so that no per-call
 *   host work depends on it.  0 <= seg_bits < 2^31 - 1600.
 * All device calls: asynchronous on `stream` (NULL = the handle's stream), one launch, no allocation, deterministic (no
 * atomics).  Argument errors return OFDM_ERR_INVALID before anything is enqueued; zero counts are a no-op returning OFDM_OK. */
typedef enum ofdm_crc_kind { OFDM_CRC24A = 0, OFDM_CRC24B = 1, OFDM_CRC16 = 2, OFDM_CRC8 = 3 } ofdm_crc_kind;
/* L of a kind: 24 / 24 / 16 / 8.  Host arithmetic; OFDM_ERR_INVALID for an unknown kind. */
int32_t ofdm_crc_bits(int32_t kind);
/* *crc = the parity of the A payload bits at host_bits_packed (MSB-first), unmasked.  Host arithmetic through the kernels' own
 * remainder routine; no device. */
int ofdm_crc_compute(int32_t kind, const uint8_t* host_bits_packed, int32_t A, uint32_t* crc);
/* d_payload dense [n_blocks][A] (or [A/8]) -> d_info dense [n_blocks][K] (or [K/8]): the payload, then parity ^ mask. */
int ofdm_tx_crc_attach_frames(ofdm_tx* h, const uint8_t* d_payload, int32_t payload_mode, int64_t n_blocks, int32_t A,
                              int32_t kind, uint32_t mask, const uint32_t* d_mask, uint8_t* d_info, int32_t info_mode, void* stream);
typedef struct ofdm_crc_out {    /* DEVICE pointers; NULL = not wanted */
    uint8_t*  ok;            /* [n_blocks] 1 iff syndrome == the block's mask                                                   */
    uint32_t* syndrome;      /* [n_blocks] CRC(first A bits) ^ received parity: a host that does not know the RNTI reads it here */
    uint8_t*  payload;       /* the first A bits of each block, dense [n_blocks][A] or [n_blocks][A/8]                          */
    int32_t   payload_mode;  /* ofdm_bits_mode of payload                                                                       */
} ofdm_crc_out;
/* d_info dense [n_blocks][K] (or [K/8]) as the decoders write it.  An `out` without any pointer is a no-op. */
int ofdm_crc_check_frames(ofdm_rx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_blocks, int32_t A, int32_t kind,
                          uint32_t mask, const uint32_t* d_mask, const ofdm_crc_out* out, void* stream);
/* host_out[i] = c(first + i), i < n, one bit per byte, for this c_init.  Host arithmetic through the kernels' own jump tables
 * (random access: no stepping from 0); OFDM_ERR_INVALID for a negative count or first + n > 2^31 - 1600. */
int ofdm_gold_bits(uint32_t c_init, int64_t first, int64_t n, uint8_t* host_out);
/* d_out bit = d_in bit ^ c, segment s = seg_bits bits at byte s*seg_bytes of both buffers, seg_bytes = seg_bits (one bit per
 * byte; written bytes are 0 or 1) or seg_bits / 8 (packed, needs seg_bits % 8 == 0): the coded output of
 * ofdm_tx_tbcc_encode_frames.  d_out == d_in is allowed. */
int ofdm_tx_scramble_frames(ofdm_tx* h, const uint8_t* d_in, int32_t mode, int64_t n_seg, int64_t seg_bits,
                            const uint32_t* d_cinit, uint8_t* d_out, void* stream);
/* d_out[s*out_stride + n] = the bit pattern of d_llr[s*seg_stride + n] with its sign bit XORed by c(n), n < seg_bits (strides in
 * floats, >= seg_bits): NaN payloads, +-inf, +-0 and subnormals keep every other bit, and descrambling twice is the identity.
 * Floats between seg_bits and the stride are not touched.  d_out == d_llr is allowed with out_stride == seg_stride. */
int ofdm_descramble_llr_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int64_t seg_bits,
                               const uint32_t* d_cinit, float* d_out, int64_t out_stride, void* stream);
/* Load the kernels of this block on the handle's device: call before capturing one of its calls into a hipGraph. */
int ofdm_tx_reserve_bitproc(ofdm_tx* h);
int ofdm_rx_reserve_bitproc(ofdm_rx* h);

/* ------------------------------------------------------------------------------------------ channel code (LTE turbo)
 * The rate-1/3 turbo code of TS 36.212 5.1.3.2 -- two 8-state constituent encoders around a QPP interleaver, with trellis
 * termination -- on the frame-batched path: the data channel's code next to the TBCC above, with an iterative max-log-MAP
 * decoder.  An extension like the TBCC: the reference has no channel code, so this text is the contract.  Code-block
 * segmentation and the table of 3GPP (f1, f2) pairs are not part of it; rate matching (5.1.4.1) is the block behind this one.
 * Code block: K information bits c[0..K), K a multiple of 8 with 40 <= K <= 6144 (LTE's 188 sizes are a subset).
 * Interleaver: pi(i) = (f1 i + f2 i^2) mod K with 0 <= f1, f2 < K, handed over by the caller.  A call whose (K, f1, f2) is not a
 *   permutation of 0 .. K-1 returns OFDM_ERR_INVALID before anything is enqueued (O(K) host work per call).
 * Constituent encoder: feedback 1 + D^2 + D^3, parity 1 + D + D^3; state s = 4 r1 + 2 r2 + r3 with r1 the most recent, start
 *   state 0.  Input u gives a = u ^ r2 ^ r3, parity z = a ^ r1 ^ r3, next(s, u) = 4 a + (s >> 1).  Encoder 1 runs over c[k] and
 *   gives z[k]; encoder 2 runs over c[pi(i)] and gives z'[i].  Termination, three steps per encoder: u = r2 ^ r3 (so a = 0),
 *   transmitted x = u and z = r1 ^ r3; x_K .. x_{K+2}, z_K .. z_{K+2} from encoder 1, x'_K .. , z'_K .. from encoder 2.
 * Streams of K + 4 bits (5.1.3.2.2):   k < K: d0 = c[k], d1 = z[k], d2 = z'[k];
 *   k = K:   x_K, z_K, x_{K+1};   K+1: z_{K+1}, x_{K+2}, z_{K+2};   K+2: x'_K, z'_K, x'_{K+1};   K+3: z'_{K+1}, x'_{K+2}, z'_{K+2}.
 *   Coded order as in the TBCC calls, e[3k+j] = dj[k]: 3K + 12 bits per block, the 12 tail values at 3K .. 3K+11 as
 *   x_K z_K x_{K+1} z_{K+1} x_{K+2} z_{K+2} followed by the same six primed.
 * Segments: the TBCC rules with 3K + 12 in place of 3K -- blocks back to back from bit 0 of the segment, filler zeros behind
 *   them (written by the encoder, ignored by the decoder).  3K + 12 is no multiple of 8: packed blocks may start inside a byte.
 * Decoder: max-log-MAP, n_iter full iterations (1 <= n_iter <= 16), fully determined; every operation is one IEEE float32
 *   operation in the order written.  Positive LLRs favour bit 0; an input LLR that is not finite counts as 0; sigma(0) = +1,
 *   sigma(1) = -1.  max(a, b) is the larger value; which zero a max of +0 and -0 returns is not specified (no comparison,
 *   decision or non-zero value depends on it).
 *   SISO(ls, la, lp, t[0..6)) -> (post, ext), metrics twice the log-domain ones:
 *     x_k = ls_k + la_k;  gamma_k(u, z) = sigma(u) x_k + sigma(z) lp_k  (exact products, one add).
 *     Forward: A_0 = (0, -inf, .., -inf); k = 0 .. K-1: m(s') = max over the two branches (s, u) -> s' of A_k(s) + gamma_k(u, z);
 *       A_{k+1}(s') = m(s') - m(0) if (k+1) mod 8 == 0, else m(s').
 *     Tail: from state s follow s_0 = s, s_{j+1} = s_j >> 1; with the bits of s_j, g_j = sigma(r2^r3) t[2j] + sigma(r1^r3) t[2j+1];
 *       b(s) = (g_0 + g_1) + g_2;  B_K(s) = b(s) - b(0).
 *     Backward, k = K-1 .. 0: t_u(s) = (A_k(s) + gamma_k(u, z)) + B_{k+1}(next(s, u));  M_u = max_s t_u(s);
 *       post_k = 0.5 (M_0 - M_1);  ext_k = 0.75 (post_k - x_k);  n(s) = max_u (gamma_k(u, z) + B_{k+1}(next(s, u)));
 *       B_k(s) = n(s) - n(0) if k mod 8 == 0, else n(s).
 *     State 0 is always reachable, so every subtrahend is finite and finite inputs give no NaN; finite LLRs whose sums overflow
 *     are outside the contract.
 *   With ls[k] = l[3k], lp1[k] = l[3k+1], lp2[k] = l[3k+2], tail 1 = l[3K .. 3K+5], tail 2 = l[3K+6 .. 3K+11] of the block's
 *   3K + 12 LLRs l (each made 0 where it is not finite):  la1 = 0;  per iteration  (., e1) = SISO(ls, la1, lp1, tail 1);
 *   ls2[i] = ls[pi(i)], la2[i] = e1[pi(i)];  (post2, e2) = SISO(ls2, la2, lp2, tail 2);  la1[pi(i)] = e2[i].
 *   Outputs per block: llr[pi(i)] = post2[i] of the last iteration; bit[k] = (llr[k] < 0), so that +0 and -0 both decide 0.
 * Deterministic: a block's outputs depend on its own 3K + 12 LLRs only -- the same bits and llr alone, in any batch, at any
 * stride and on every call (no atomics). */
/* floor(seg_bits / (3K + 12)): the blocks a segment can carry.  Host arithmetic; OFDM_ERR_INVALID for a bad K or seg_bits < 0. */
int64_t ofdm_turbo_blocks(int64_t seg_bits, int32_t K);
/* OFDM_OK iff K is valid, 0 <= f1, f2 < K and pi is a permutation of 0 .. K-1.  Host arithmetic, O(K). */
int ofdm_turbo_qpp_check(int32_t K, int32_t f1, int32_t f2);
/* The layouts, filler, no-op and error rules of ofdm_tx_tbcc_encode_frames with 3K + 12 coded bits per block
 * (seg_bits >= blocks_per_seg*(3K+12)); a triple that is no permutation is OFDM_ERR_INVALID.  One launch, no allocation. */
int ofdm_tx_turbo_encode_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                                int32_t K, int32_t f1, int32_t f2, uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits,
                                void* stream);
typedef struct ofdm_turbo_out {  /* DEVICE pointers; NULL = not wanted */
    uint8_t* bits;       /* dense [n_seg][blocks_per_seg][K] decoded bits: packed MSB-first (K/8 bytes per block) or one per byte */
    int32_t  bits_mode;  /* ofdm_bits_mode of bits                                                                             */
    float*   llr;        /* dense [n_seg][blocks_per_seg][K] float32 a-posteriori LLRs                                         */
} ofdm_turbo_out;
/* Sizes the handle's device workspace for decoding up to n_blocks blocks of K bits per call and loads the kernel.  Workspace:
 * 4 n_blocks K bytes of extrinsic values plus 256 ceil(n_blocks / 8) ceil(K / 32) bytes of forward metrics (one checkpoint of
 * 8 states x 8 blocks every 32 trellis steps); it only grows.  Growing waits for the device and allocates, so call this before
 * capturing ofdm_turbo_decode_frames into a hipGraph: inside a capture a call that would have to grow returns OFDM_ERR_INVALID. */
int ofdm_rx_reserve_turbo(ofdm_rx* h, int64_t n_blocks, int32_t K);
/* Block (s, b) reads the 3K + 12 float32 LLRs at d_llr + s*seg_stride + b*(3K+12) (seg_stride in floats, >=
 * blocks_per_seg*(3K+12)).  Asynchronous on `stream` (NULL = the handle's stream): one launch, no host synchronisation and, once
 * reserved, no allocation.  The workspace belongs to the handle: calls on one handle must not overlap on the device (one stream,
 * or ordered by events).  n_seg == 0, blocks_per_seg == 0 or an `out` without any pointer is a no-op returning OFDM_OK.
 * Argument errors (NULL handle, bad K, a triple that is no permutation, n_iter outside 1 .. 16, seg_stride too short, a negative
 * count, a batch beyond the kernel's index range) return OFDM_ERR_INVALID before anything is enqueued. */
int ofdm_turbo_decode_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, int32_t K,
                             int32_t f1, int32_t f2, int32_t n_iter, const ofdm_turbo_out* out, void* stream);
/* Early termination by CRC: a second decoder entry point for code blocks that end in a CRC (every code block of a transport
 * block does).  After every full iteration from min_iter on, the CRC of each block's hard decisions is checked; a block that
 * passes stops there.  It changes no arithmetic: with bit_n[k] and llr_n[k] the outputs of ofdm_turbo_decode_frames at
 * n_iter = n on the same 3K + 12 LLRs,
 *   block b stops at the smallest n in min_iter .. max_iter for which bit_n[0] D^(K-1) + .. + bit_n[K-1] is divisible by the
 *   generator of crc_kind -- the arithmetic of the CRC block above: all four kinds, zero mask, all K bits, so that leading zeros
 *   (filler) do not matter -- and at max_iter if there is no such n;
 *   bits and llr are bit_n and llr_n (floats by bit pattern), iters = n, crc_ok = 1 iff the remainder was zero at n.
 * False passes are part of the contract: a wrong decision whose remainder is zero stops the block, and a block of all-zero or
 * all-NaN LLRs decides all zeros and stops at min_iter with crc_ok = 1.  1 <= min_iter <= max_iter <= 16; stat_stride is 0 or
 * >= blocks_per_seg.  The layout, no-op (an `out` without any of its four pointers) and error rules are those of
 * ofdm_turbo_decode_frames, an unknown crc_kind included: OFDM_ERR_INVALID before anything is enqueued, and likewise inside a
 * capture for a call that would have to grow the workspace.  One launch, no host synchronisation, no allocation once reserved.
 * Deterministic: a block's outputs depend on its own LLRs only, in any batch, at any stride, next to any neighbours (a wave of 8
 * blocks runs as long as its slowest block; the others are frozen, not re-decoded). */
typedef struct ofdm_turbo_es_out {   /* DEVICE pointers; NULL = not wanted */
    uint8_t* bits;  int32_t bits_mode;  float* llr;      /* as ofdm_turbo_out */
    uint8_t* iters;        /* iterations the block ran, min_iter .. max_iter                      */
    uint8_t* crc_ok;       /* 1 iff the remainder was zero after that iteration                   */
    int64_t  stat_stride;  /* iters / crc_ok of block (s, b) at s*stat_stride + b; 0 = blocks_per_seg */
} ofdm_turbo_es_out;
/* ofdm_rx_reserve_turbo for this entry point: the same workspace (one per handle, it only grows) with a second array of
 * 4 n_blocks K bytes, the a-posteriori values of each block's latest checked iteration. */
int ofdm_rx_reserve_turbo_es(ofdm_rx* h, int64_t n_blocks, int32_t K);
int ofdm_turbo_decode_es_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                                int32_t K, int32_t f1, int32_t f2, int32_t crc_kind, int32_t min_iter, int32_t max_iter,
                                const ofdm_turbo_es_out* out, void* stream);

/* ------------------------------------------------------------------------------------------ rate matching (LTE turbo)
 * The three sub-block interleavers, the circular buffer with its limit Ncb and the redundancy versions of TS 36.212 5.1.4.1
 * around the code above: E rate-matched bits per block in place of the 3K + 12 of e[3i+j], on the transmit side as an encoder
 * of its own and on the receive side as a de-matching stage that can add a retransmission into an existing soft buffer (HARQ
 * chase or incremental-redundancy combining).  An extension like the code itself: this text is the contract.
 * Geometry: K, f1, f2 as above; D = K + 4; the three streams dj[i], i < D, are exactly the coded order e[3i + j] above (the 12
 *   tail values already sit there as d0 .. d2 of i = K .. K+3).  R = ceil(D / 32), Kpi = 32R, ND = Kpi - D (K is a multiple of 8,
 *   so ND is 4, 12, 20 or 28), Kw = 3 Kpi.
 * Sub-block interleaver: P[c] is the 5-bit reversal of c, <0,16,8,24,4,20,12,28,2,18,10,26,6,22,14,30,1,17,..,31> (not the
 *   TBCC's P).  d0 and d1: the stream, prefixed with ND NULLs, is written row by row into an R x 32 matrix; column c of the
 *   permuted matrix is column P[c] of it; read column by column it is v0 resp. v1.  d2: with y = ND NULLs followed by d2,
 *   v2[k] = y[pi2(k)], pi2(k) = (P[floor(k / R)] + 32 (k mod R) + 1) mod Kpi.
 * Circular buffer: w[k] = v0[k], w[Kpi + 2k] = v1[k], w[Kpi + 2k + 1] = v2[k], k < Kpi.
 * Selection: buffer length Ncb with Kpi <= Ncb <= Kw (an argument of 0 means Kw), redundancy version rv in 0 .. 3,
 *   k0 = R (2 ceil(Ncb / (8R)) rv + 2); e_k, k < E, are the entries of w[(k0 + j) mod Ncb], j = 0, 1, 2, .., that are not NULL,
 *   in order.  Navail = the entries of w[0 .. Ncb) that are not NULL (3K + 12 at Ncb = Kw); 1 <= E <= 16 Navail, so that a coded
 *   bit is sent at most 16 times.
 * rv per call or per segment: the scalar rv, or with d_rv != NULL one int32 per segment on the device of which the low two bits
 *   are read (the scalar is then not used; a batch holds transport blocks at different HARQ rounds).
 * Closed form: the NULLs of v0 and v1 are row 0 of the columns with P[c] < ND, those of v2 row 0 of the columns with
 *   P[c] < ND - 1 and its last entry (pi2 = 0).  d0[i] and d1[i] sit at column P[y & 31], row y >> 5 of their stream with
 *   y = ND + i, d2[i] at the same place for y - 1.  The rank of a place -- the entries in front of it that are not NULL -- is a
 *   popcount over the 32-bit mask of those columns plus the interlacing; the first transmission of a coded bit is
 *   n0 = (rank - rank(k0)) mod Navail and its copies follow every Navail bits.
 * Segments: the TBCC rate-matching rules with E -- block b has its bits at segment bit b*E and its LLRs at
 *   d_llr + s*seg_stride + b*E; blocks_per_seg*E <= seg_bits (encoder), seg_stride >= blocks_per_seg*E (receive side); filler
 *   zeros follow the last block.  E need not be a multiple of 8: packed blocks may start inside a byte.
 * De-matching, IEEE float32 in this order: v(x) = x if x is finite, else 0.  For coded bit dj[i] with n0 the index of its
 *   first transmission in e: it has none if its place in w is >= Ncb or if n0 >= E, and then L = +0; otherwise L = v(l[n0]) and
 *   then L = L + v(l[n0 + m Navail]) for m = 1, 2, .. while the index is < E, in increasing m.  accumulate == 0:
 *   out[3i + j] = L, stored as summed (an overflowed sum as +-inf, a single -0 as -0).  accumulate != 0: out[3i + j] = old + L
 *   with old the float already there, read as is: one float32 addition after L is complete.  The first transmission of a block
 *   uses accumulate == 0 or a zeroed buffer.  The output is what ofdm_turbo_decode_frames reads, 3K + 12 floats per block; that
 *   decoder counts inputs that are not finite as 0.  The de-matched buffer IS the HARQ soft buffer, so there is no decoder
 *   variant that de-matches while it loads.
 * Deterministic: a block's outputs depend on its own E LLRs only, plus its old soft values when accumulating (no atomics). */
/* floor(seg_bits / E): the blocks a segment can carry.  Host arithmetic; OFDM_ERR_INVALID for a bad K, E outside
 * 1 .. 16 (3K + 12) or seg_bits < 0. */
int64_t ofdm_turbo_rm_blocks(int64_t seg_bits, int32_t K, int32_t E);
/* *k0 and *n_avail (either may be NULL) of (K, Ncb, rv).  Host arithmetic through the kernels' own geometry routine; no device. */
int ofdm_turbo_rm_info(int32_t K, int32_t Ncb, int32_t rv, int32_t* k0, int32_t* n_avail);
/* ofdm_tx_turbo_encode_frames with E rate-matched bits per block: the same layouts, filler, no-op and error rules
 * (seg_bits >= blocks_per_seg*E), and OFDM_ERR_INVALID for E or Ncb out of range or a scalar rv outside 0 .. 3 while it is in
 * use.  One launch, no allocation. */
int ofdm_tx_turbo_encode_rm_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                                   int32_t K, int32_t f1, int32_t f2, int32_t E, int32_t Ncb, int32_t rv, const int32_t* d_rv,
                                   uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream);
/* d_out[s*out_stride + b*(3K+12) + 3i + j] = L of dj[i], or old + L (out_stride in floats, >= blocks_per_seg*(3K+12)).
 * Asynchronous on `stream` (NULL = the handle's stream), one launch, no allocation, no host synchronisation; n_seg == 0 or
 * blocks_per_seg == 0 is a no-op.  OFDM_ERR_INVALID before anything is enqueued for a NULL handle, a bad K, E or Ncb out of
 * range, a scalar rv outside 0 .. 3 while in use, a stride that is too short, a negative count or a batch beyond the index
 * range. */
int ofdm_turbo_rate_dematch_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                                   int32_t K, int32_t E, int32_t Ncb, int32_t rv, const int32_t* d_rv, int32_t accumulate,
                                   float* d_out, int64_t out_stride, void* stream);
/* Load the kernels of this block on the handle's device: call before capturing one of its calls into a hipGraph. */
int ofdm_tx_reserve_turbo_rm(ofdm_tx* h);
int ofdm_rx_reserve_turbo_rm(ofdm_rx* h);

/* ------------------------------------------------------------------------------------------ transport block (LTE turbo)
 * The layer that makes the three blocks above usable on a real payload: transport-block CRC (TS 36.212 5.1.1), code-block
 * segmentation with a CRC per code block (5.1.2), the two rate-matching sizes of a transport block (5.1.4.1.2) and code-block
 * concatenation (5.1.5), around the encode / de-match / decode calls above, which it uses as they are.  An extension like the
 * code itself: this text is the contract.
 * Valid K here: LTE's 188 sizes -- 40 .. 512 in steps of 8, 528 .. 1024 in steps of 16, 1056 .. 2048 in steps of 32,
 *   2112 .. 6144 in steps of 64.
 * Segmentation of a transport block of A bits, A a multiple of 8 with 8 <= A <= 2^20 - 24, at the maximum code block size Z, one
 *   of the valid K (an argument of 0 means 6144; smaller values exist so that every branch can be reached with small blocks):
 *   B = A + 24: the payload, then its CRC24A with a zero mask, in the arithmetic of the CRC block above (p0 first).
 *   B <= Z: L = 0, C = 1, B' = B.  Otherwise L = 24, C = ceil(B / (Z - 24)), B' = B + 24 C.
 *   K+ = the smallest valid K with C K >= B'.  C = 1: C+ = 1, C- = 0, K- = 0.  Otherwise K- = the largest valid K below K+,
 *   dK = K+ - K-, C- = floor((C K+ - B') / dK), C+ = C - C-; at K+ = 40, where there is no K-, dK = 8 and K- = 0, and a case with
 *   C- > 0 there is OFDM_ERR_INVALID.  F = C+ K+ + C- K- - B'.
 *   Blocks r < C- have K- bits, the others K+.  Block 0 starts with F zeros; then each block carries its K_r - L bits of the
 *   B-bit sequence in order, and with L = 24 the CRC24B (zero mask) of its first K_r - 24 bits, the filler zeros included,
 *   follows.  A, B', F and every K are multiples of 8, so every packed block and every slice is byte aligned.
 * Filler bits -- a DEVIATION from TS 36.212: they are encoded and rate-matched as ordinary zeros and not marked <NULL> as
 *   5.1.3.2.1 and 5.1.4.1.1 ask, on the transmit and on the receive side alike, so the two sides of this library agree with
 *   each other and, for F > 0, with nobody else.  F is reported: a host that needs conformance refuses F > 0.  The transport
 *   block sizes of TS 36.213 are believed to give F = 0 throughout; that is a belief, it has not been checked here.
 * Rate matching: G coded bits per transport block in units of q = N_L Q_m >= 1, G % q == 0.  G' = G / q, gamma = G' mod C;
 *   E_r = q floor(G' / C) (E0) for r <= C - gamma - 1, else q ceil(G' / C) (E1).  Every E_r has to lie in 1 .. 16 Navail of its
 *   block.  Soft-buffer limit N_IR (0 = none): Ncb_r = min(floor(N_IR / C), Kw_r), OFDM_ERR_INVALID if that is below Kpi_r.
 * Groups: the boundaries C- and C - gamma cut 0 .. C into at most three contiguous runs of blocks with one (K, E) each, in block
 *   order; ofdm_tb_geom names them.  Workspaces and the soft buffer are laid out by them.
 * Interleavers: the caller supplies one (f1, f2) for K- and one for K+ (the table of 3GPP pairs is not part of this library);
 *   each one that has blocks is held to the rule of ofdm_turbo_qpp_check, the other is not looked at.
 * Codeword: the blocks' E_r bits back to back, r = 0 .. C-1, G bits; transport block t at bit t*cw_bits of the buffer
 *   (cw_bits >= G, zeros from G on; packed codewords need cw_bits % 8 == 0).  On the receive side its LLRs at
 *   d_llr + t*llr_stride (floats, llr_stride >= G).
 * HARQ soft buffer: per transport block sum_r (3 K_r + 12) floats in block order -- what the de-matcher writes and the decoder
 *   reads -- at d_soft + t*soft_stride (soft_stride >= that sum).  It belongs to the caller and goes in and out; `accumulate`
 *   has the de-matcher's meaning, and rv / d_rv (one value per transport block) the rate matcher's.
 * Results: the A payload bits, tb_ok = (CRC24A of the re-joined first A bits == the 24 bits behind them), that difference as
 *   `syndrome`, and cb_ok[t][r] = the same for block r's CRC24B (1 with L = 0).  Deterministic, no atomics. */
typedef struct ofdm_tb_geom {
    int32_t A, Z, B, L, C, K_plus, K_minus, C_plus, C_minus, F, n_groups;
    int32_t G, q, gamma, E0, E1, Ncb_minus, Ncb_plus;   /* Ncb resolved (Kw without a limit), 0 for a K without blocks; all 0 at G == 0 */
    struct { int32_t first, count, K, E; int64_t cw_bit_offset, soft_offset; } group[3];
    int64_t soft_floats;       /* sum_r (3 K_r + 12)                                                                 */
} ofdm_tb_geom;
/* The smallest valid K >= bits (40 for every bits <= 40), or OFDM_ERR_INVALID above 6144.  Host arithmetic. */
int32_t ofdm_turbo_k_next(int32_t bits);
/* Everything above for one transport block.  G == 0: the segmentation alone (q and N_IR are not looked at; the groups are the
 * runs of one K, with E = 0 and cw_bit_offset = 0).  Host arithmetic; OFDM_ERR_INVALID for anything out of range. */
int ofdm_tb_geometry(int32_t A, int32_t Z, int64_t G, int32_t q, int64_t N_IR, ofdm_tb_geom* out);
/* ofdm_crc_compute without its length limit: n_bits a multiple of 8 with 8 <= n_bits <= 2^30.  Host arithmetic through the
 * kernels' own chunk-and-combine routine (256 runs, each multiplied by x^(bits behind it) mod g, XORed); no device. */
int ofdm_crc_compute_long(int32_t kind, const uint8_t* host_bits_packed, int64_t n_bits, uint32_t* crc);
/* d_payload dense [n_tb][A] (or [A/8]) -> d_cw [n_tb][cw_bits] (or [cw_bits/8]).  Asynchronous on `stream` (NULL = the handle's
 * stream): the segment kernel, one rate-matching encoder launch per group, the concatenation kernel; no host synchronisation
 * and, once reserved, no allocation.  The workspace belongs to the handle: calls on one handle must not overlap on the device.
 * n_tb == 0 is a no-op.  Argument errors (NULL handle, anything ofdm_tb_geometry refuses, G == 0, a pair that is no permutation,
 * bad modes, a scalar rv outside 0 .. 3 while in use, cw_bits < G, a batch beyond the kernels' index range) return
 * OFDM_ERR_INVALID before anything is enqueued, and so does, inside a capture, a call that would have to grow the workspace. */
int ofdm_tx_tb_encode_frames(ofdm_tx* h, const uint8_t* d_payload, int32_t payload_mode, int64_t n_tb, int32_t A, int32_t Z,
                             int64_t G, int32_t q, int64_t N_IR, int32_t f1_minus, int32_t f2_minus, int32_t f1_plus,
                             int32_t f2_plus, int32_t rv, const int32_t* d_rv, uint8_t* d_cw, int32_t cw_mode, int64_t cw_bits,
                             void* stream);
typedef struct ofdm_tb_out {     /* DEVICE pointers; NULL = not wanted */
    uint8_t*  payload;       /* dense [n_tb][A] or [n_tb][A/8]                                                  */
    int32_t   payload_mode;  /* ofdm_bits_mode of payload                                                       */
    uint8_t*  tb_ok;         /* [n_tb]                                                                          */
    uint8_t*  cb_ok;         /* [n_tb][C]                                                                       */
    uint32_t* syndrome;      /* [n_tb] CRC24A of the re-joined payload ^ the received parity                    */
} ofdm_tb_out;
/* One de-matching launch per group straight out of d_llr into d_soft, one decoder launch per K on d_soft in place, the
 * desegment kernel.  The rules of the encode call; additionally n_iter in 1 .. 16, llr_stride >= G, soft_stride >= soft_floats,
 * and `out` == NULL is an argument error (an `out` without any pointer de-matches and stops there: the soft buffer is an
 * output of its own).  The decoder's workspace is the one of ofdm_rx_reserve_turbo. */
int ofdm_tb_decode_frames(ofdm_rx* h, const float* d_llr, int64_t n_tb, int64_t llr_stride, int32_t A, int32_t Z, int64_t G,
                          int32_t q, int64_t N_IR, int32_t f1_minus, int32_t f2_minus, int32_t f1_plus, int32_t f2_plus,
                          int32_t rv, const int32_t* d_rv, int32_t n_iter, int32_t accumulate, float* d_soft, int64_t soft_stride,
                          const ofdm_tb_out* out, void* stream);
/* Size the handle's workspace for n_tb transport blocks of this geometry per call (transmit: the packed code blocks and G bytes
 * of encoder output per transport block; receive: the packed decoded blocks, and the turbo decoder's workspace for both K) and
 * load the kernels; the workspaces only grow.  Growing waits for the device, so call these before capturing into a hipGraph. */
int ofdm_tx_reserve_tb(ofdm_tx* h, int64_t n_tb, int32_t A, int32_t Z, int64_t G, int32_t q);
int ofdm_rx_reserve_tb(ofdm_rx* h, int64_t n_tb, int32_t A, int32_t Z);
/* ofdm_tb_decode_frames with early termination: the same sequence, the decoder launches through ofdm_turbo_decode_es_frames
 * with crc_kind = OFDM_CRC24B when L = 24 and OFDM_CRC24A when C = 1 (the block then ends in the transport block's own CRC).
 * cb_iters[t][r] = the iterations block r ran.  payload, tb_ok, cb_ok and syndrome are those of ofdm_tb_decode_frames run with
 * each block at its own n; the soft buffer is written by the de-matcher only.  cb_iters alone makes the call decode.
 * ofdm_rx_reserve_tb_es is ofdm_rx_reserve_tb with the decoder workspace of ofdm_rx_reserve_turbo_es. */
typedef struct ofdm_tb_es_out {  /* DEVICE pointers; NULL = not wanted */
    uint8_t*  payload;  int32_t payload_mode;  uint8_t* tb_ok;  uint8_t* cb_ok;  uint32_t* syndrome;   /* as ofdm_tb_out */
    uint8_t*  cb_iters;      /* [n_tb][C]                                                                       */
} ofdm_tb_es_out;
int ofdm_tb_decode_es_frames(ofdm_rx* h, const float* d_llr, int64_t n_tb, int64_t llr_stride, int32_t A, int32_t Z, int64_t G,
                             int32_t q, int64_t N_IR, int32_t f1_minus, int32_t f2_minus, int32_t f1_plus, int32_t f2_plus,
                             int32_t rv, const int32_t* d_rv, int32_t min_iter, int32_t max_iter, int32_t accumulate,
                             float* d_soft, int64_t soft_stride, const ofdm_tb_es_out* out, void* stream);
int ofdm_rx_reserve_tb_es(ofdm_rx* h, int64_t n_tb, int32_t A, int32_t Z);

/* ------------------------------------------------------- CFO-search receiver */
/* Replaces OFDMReceiver.SynchEstAndFO (G/LEGACY/gr-ofdm-rx/python/SynchEstAndFO.py:28-369): the
 * gr-RXOFDM receiver (root-37 ZC, stride cp-1, gate 0.4, linear SNR) plus a brute-force carrier
 * offset search -- every sync trial is evaluated once per candidate rotator (:258-282) -- and a
 * table of up to OFDM_FO_MAX_SYNC syncs per work() call, each followed by ONE equalised data
 * symbol (:332-358).  The candidate rotators are handed over as a table so that the caller decides
 * how `cfo` (:192) is formed (under the file's Python-2 semantics 1/fs is an integer division and
 * every rotator is 1). */
#define OFDM_FO_MAX_SYNC 100          /* rows of time_synch_ref / est_chan_freq_P / est_data_freq (:197,202-206) */
typedef struct ofdm_fo ofdm_fo;
typedef struct ofdm_fo_cfg {
    int32_t num_ofdm_symb;     /* :37  only sizes the output: corr_size = num_ofdm_symb / (S+D) rows (:362)      */
    int32_t nfft;
    int32_t cp_len;
    int32_t num_synch_bins;
    int32_t synch_S, synch_D;
    int32_t num_data_bins;
    int32_t n_fo;              /* len(fo_range) >= 1                                                           */
    double snr;                /* self.SNR (:150), linear                                                      */
    const float* rotators;     /* host, [n_fo][nfft] complex64 interleaved: self.cfo (:192); copied.  NULL with
                                * n_fo == 1: no rotation at all = work() of gr-RXOFDM's synch_and_chan_est
                                * (gr-RXOFDM/python/synch_and_chan_est.py:136-266), short data slices zero-padded (:228-230) */
    int32_t device;
    int32_t dsss;              /* 0: SynchEstAndFO.  >= 1: SynchEstFOAndDSSS with spreading factor self.DSSS     */
    const float* spread_code;  /* host, [dsss] complex64 interleaved: self.SC (SynchEstFOAndDSSS.py:253-262); copied */
} ofdm_fo_cfg;

typedef struct ofdm_fo_report {
    int32_t n_sync;            /* cor_obs + 1 before the end-of-call reset (:369)                               */
    int32_t count;
    int32_t dmax_tmp_ind;      /* candidate index of the LAST trial evaluated (:283), -1 if none ever was         */
    int32_t trials_run;
    int64_t n_data_items;      /* corr_size * num_data_bins values packed at the head of `out` (when count > 0) */
} ofdm_fo_report;

int ofdm_fo_create(const ofdm_fo_cfg* cfg, ofdm_fo** out);
int ofdm_fo_destroy(ofdm_fo* h);
/* SynchEstAndFO.work (:232-369), host buffers; returns n_out or a negative ofdm_status
 * (OFDM_ERR_INDEX: a 101st sync, :294-296; OFDM_ERR_SHAPE: short data slice :338-339 / reshape :364). */
int64_t ofdm_fo_work(ofdm_fo* h, const float* h_in, int64_t n_in, float* h_out, int64_t n_out, ofdm_fo_report* rep);
/* Block attributes, any pointer may be NULL: h_tsr[100][3] doubles (time_synch_ref), complex64 interleaved
 * h_chan_freq[100][nfft], h_chan_time[100][nfft], h_synch_freq[100][S*Ks], h_data_freq[100][Kd], h_eq_gain[Ks]. */
int ofdm_fo_get_state(ofdm_fo* h, double* h_tsr, float* h_chan_freq, float* h_chan_time, float* h_synch_freq,
                      float* h_data_freq, float* h_eq_gain);
/* DSSS variant (cfg.dsss >= 1; SynchEstFOAndDSSS.py:28-413, grc/OFDMReceiver_SynchEstFOAndDSSS.block.yml): after the
 * equaliser every row is despread -- est_data_freq_d[P][i] = mean_SF(est_data_freq[P][SF + i*DSSS] * conj(SC[SF])),
 * i < floor(Kd/DSSS) (:391-399) -- and ofdm_fo_work emits the first corr_size despread rows on EVERY call (:405-407).
 * OFDM_ERR_UNBOUND: row 0 of an earlier call fails the data guard before any row passed (:392).
 * h_data_freq_d[100][floor(Kd/DSSS)] complex64 interleaved. */
int ofdm_fo_get_despread(ofdm_fo* h, float* h_data_freq_d);

/* Frame-batched device path of the same receiver (additive: ofdm_fo_work and the handle's stream state are untouched).
 * Every frame is the FIRST work() call of a FRESH SynchEstAndFO / SynchEstFOAndDSSS / table-mode instance on that frame's
 * samples d_iq[f*frame_stride .. +frame_len) (complex64 items).  All pointers below are DEVICE pointers; NULL = not wanted.
 * R = OFDM_FO_MAX_SYNC rows per frame; row r < n_sync is the r-th accepted sync, rows >= n_sync are written as zeros.
 * On a fresh first call a trial is evaluated only if S*L + P*stride + N + cp < frame_len (:249), so the data window of every
 * accepted sync is complete: the reference's ValueError (short slice, :338), UnboundLocalError (DSSS :392) and NameError
 * (undefined dmax_tmp_ind) cannot occur.  The one per-frame error is a 101st sync (IndexError, :294-296): that frame gets
 * status OFDM_ERR_INDEX and unspecified other outputs; the other frames and the call's return value are unaffected. */
typedef struct ofdm_fo_batch_out {
    int32_t* status;       /* REQUIRED [n_frames]: n_sync (0..R) or OFDM_ERR_INDEX                                        */
    int32_t* tsr;          /* [n_frames][R][3] time_synch_ref {P*stride+cp, lag, int(max|corr|)}                          */
    int32_t* fo_idx;       /* [n_frames] dmax_tmp_ind: best candidate of the LAST trial evaluated (:283), -1 if none       */
    float* data_freq;      /* [n_frames][R][Kd] complex64 est_data_freq: one equalised data symbol per sync (:332-358)      */
    uint8_t* bits;         /* hard QPSK bits of those rows: [n_frames][R][Kd*2] bytes (UNPACKED) or [..][Kd/4] (PACKED)   */
    int32_t bits_mode;     /* ofdm_bits_mode of `bits` (PACKED needs num_data_bins % 4 == 0)                               */
    float* data_freq_d;    /* cfg.dsss > 0 only: [n_frames][R][floor(Kd/DSSS)] complex64 est_data_freq_d (DS:391-399)      */
    float* chan_freq;      /* [n_frames][R][nfft] complex64 est_chan_freq_P                                                */
    float* chan_time;      /* [n_frames][R][nfft] complex64 est_chan_time                                                  */
    float* synch_freq;     /* [n_frames][R][S*Ks] complex64 est_synch_freq                                                 */
} ofdm_fo_batch_out;

/* Device workspace of ofdm_fo_demod_frames for batches of up to n_frames frames of frame_len samples (grows, never shrinks;
 * synchronises the device).  Call it before capturing a batch call into a hipGraph. */
int ofdm_fo_reserve(ofdm_fo* h, int64_t n_frames, int64_t frame_len);
/* Asynchronous on `stream` (NULL = the handle's stream): four launches -- trial table of every frame, per-frame decision
 * (gate, distance rule, 101st sync), LS estimate per accepted sync, one data symbol per sync (+ despreading) -- with no host
 * synchronisation and no allocation once ofdm_fo_reserve covers the call (else the workspace grows first, outside a capture).
 * Returns R (rows per frame) or a negative ofdm_status; argument errors (NULL handle, NULL status, data_freq_d without dsss,
 * frame_stride < frame_len, a batch beyond the kernels' index range) return OFDM_ERR_INVALID without touching the device. */
int64_t ofdm_fo_demod_frames(ofdm_fo* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             const ofdm_fo_batch_out* out, void* stream);

/* ------------------------------------------------ regression-tracking receiver */
/* Device primitives behind OFDMReceiver.SynchronizeAndEstimate (G/LEGACY/gr-ofdm-rx/python/SynchronizeAndEstimate.py:25-442).
 * The block's control flow is a strictly sequential pointer tracker (each window position depends on the outcome of the
 * previous one, from the sixth sync on through a least-squares line, :230-350); that scalar logic stays in the host-side
 * block mirror, which calls these entry points for every array computation: the strided acquisition search and the
 * per-sync trial (:236-276), the LS estimate (:344-378) and the data stage (:397-440).  [1,3]-type patterns with ONE sync
 * symbol per pattern only (the reference's reshape at :351 does not work for more). */
typedef struct ofdm_trk ofdm_trk;
typedef struct ofdm_trk_cfg {
    int32_t nfft, cp_len;
    int32_t num_synch_bins;    /* nfft - 2 (:122)                                                               */
    int32_t num_data_bins;
    int32_t synch_D;           /* data symbols per pattern (3)                                                   */
    int32_t rows_sync;         /* lmax_s: rows of est_chan_freq_p / est_synch_freq / est_chan_impulse (:143)     */
    int32_t rows_data;         /* lmax_d: rows of est_data_freq (:144)                                           */
    int32_t zc_root;           /* 23 (:125)                                                                      */
    double snr;                /* linear (:349,377,425)                                                          */
    int32_t device;
    int32_t reserved;
} ofdm_trk_cfg;
int ofdm_trk_create(const ofdm_trk_cfg* cfg, ofdm_trk** out);
int ofdm_trk_destroy(ofdm_trk* h);
/* work() buffer -> HBM; kept until the next load */
int ofdm_trk_load(ofdm_trk* h, const float* h_in, int64_t n_in);
/* `count` windows at first_ptr + i*step: h_peak[i] = max_d |del_mat[d]|, h_lag[i] = argmax d in 0..cp (:236-274).
 * The caller vouches that every window lies inside the buffer (:240). */
int ofdm_trk_trials(ofdm_trk* h, int64_t first_ptr, int32_t step, int32_t count, float* h_peak, int32_t* h_lag);
/* LS estimate of the window at window_ptr into row `row` (:344-378): est_chan_freq_p, est_chan_impulse, est_synch_freq
 * with the phase column lag_sync, and the data equaliser of that row de-rotated by lag_data (:421, may be -1).
 * row >= rows_sync -> OFDM_ERR_INDEX (the reference raises IndexError at :358). */
int ofdm_trk_accept(ofdm_trk* h, int32_t row, int64_t window_ptr, int32_t lag_sync, int32_t lag_data);
/* Data stage (:397-440) for syncs 0..n_sync-1: h_ptr[p] = time_synch_ref[p][0]; h_guard[p] != 0 iff :401 holds.  Rows
 * p*D+n of est_data_freq are equalised and renormalised in loop order; h_last[Kd] receives the last row processed (what
 * lands in out[0:Kd], :438-440), *last_row its index or -1.  A row past rows_data -> OFDM_ERR_INDEX; short and even empty
 * data slices are zero-padded like np.fft.fft(x, N) does. */
int ofdm_trk_demod(ofdm_trk* h, int32_t n_sync, const int64_t* h_ptr, const uint8_t* h_guard, float* h_last, int32_t* last_row);
/* complex64 interleaved, any pointer may be NULL: h_chan_freq[rows_sync][nfft], h_chan_impulse[rows_sync][nfft],
 * h_synch_freq[rows_sync][Ks], h_data_freq[rows_data][Kd] */
int ofdm_trk_get_state(ofdm_trk* h, float* h_chan_freq, float* h_chan_impulse, float* h_synch_freq, float* h_data_freq);

/* ------------------------------------------------------------------------------------------ misc */
/* *d_count += number of differing bits of two device byte strings (packed bit-streams): the BER numerator without moving
 * the streams -- with frames sharded over GPUs the ranks then exchange 8 bytes instead of their bits.  The
 * reference's idiom is bitwise_xor(a, b).sum() (TEST/GNU_RADIO_OFFLINE/pls_aio.py:131).  d_count is a DEVICE uint64 the
 * caller zeroes; asynchronous on `stream` (NULL: the default stream).  n_bytes <= 2^40. */
int ofdm_count_bit_errors(int32_t device, const uint8_t* d_a, const uint8_t* d_b, int64_t n_bytes, uint64_t* d_count, void* stream);

/* Measurement aid for bench.py: mode 0 = float4 device copy of `bytes` (achievable HBM rate of this chip, same run);
 * mode 1 = the demod kernel's access pattern without arithmetic (per symbol: skip gap_bytes, read sym_in_bytes, write
 * sym_out_bytes).  Asynchronous on `stream`. */
int ofdm_bandwidth_probe(int32_t device, const void* d_in, void* d_out, int64_t bytes, int32_t mode, int32_t sym_in_bytes,
                         int32_t gap_bytes, int32_t sym_out_bytes, int64_t n_sym, void* stream);
/* Frame partition of the N-GPU path: frames are independent (each is one reference work() buffer: own sync, own estimate,
 * SynchAndChanEst.py:135-262 keeps no state between the buffers the batch entry takes), so rank `rank` of `world` owns the
 * contiguous frames [*first, *first + *count) and calls ofdm_rx_demod_frames on them with its own handle on its own device; the
 * only exchange is the caller's all-gather of the packed bits.  The same rule as ofdm_mi355x.dist.shard_frames and bench.py, for
 * hosts that are not Python.  n_frames_total must be a multiple of world (an all-gather needs equal counts: pad the batch), else
 * OFDM_ERR_INVALID.  Host arithmetic only: no device is touched. */
int ofdm_shard_frames(int64_t n_frames_total, int32_t world, int32_t rank, int64_t* first, int64_t* count);
int ofdm_abi_version(void);
const char* ofdm_last_error(void);
/* plain device memory helpers so hosts without torch can drive the batch path */
int ofdm_device_malloc(int32_t device, void** d_ptr, int64_t bytes);
int ofdm_device_free(int32_t device, void* d_ptr);
int ofdm_memcpy_h2d(int32_t device, void* d_dst, const void* h_src, int64_t bytes);
int ofdm_memcpy_d2h(int32_t device, void* h_dst, const void* d_src, int64_t bytes);
int ofdm_device_synchronize(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_H */
