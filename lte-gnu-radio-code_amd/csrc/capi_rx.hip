// capi_rx.hip -- the receiver handle: create / destroy / setters / state, the frame-batched ofdm_rx_demod_frames, ofdm_demap and the
// stream block ofdm_rx_work with the reference's control flow (SynchAndChanEst.work, gr-utsa_ofdm/python/SynchAndChanEst.py:135-262).
#include "capi_internal.hpp"

namespace {
constexpr int SEG_STATE_0[2] = {0x7fffffff, 0};   // d_seg_state before a search: {first hit, segments done}
}

extern "C" {

int ofdm_rx_destroy(ofdm_rx* h) {
    if (!h) return OFDM_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->pin_tsr) (void)hipHostFree(h->pin_tsr);
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    free_dev(&h->tb_ws, &h->d_pack, &h->d_tw, &h->d_zc, &h->d_in, &h->d_edf, &h->s_tsr, &h->s_H, &h->s_htime, &h->s_esf, &h->s_eqg, &h->s_gain,
             &h->s_ysc, &h->d_trial_m, &h->d_trial_d, &h->d_partial, &h->f_tsr, &h->f_H, &h->f_gain, &h->f_htime, &h->d_scan_g,
             &h->d_seg_state, &h->d_work, &h->f_seg_partial, &h->p_idx, &h->p_k, &h->p_src, &h->f_usum, &h->t_ws, &h->c_part_e,
             &h->c_part_n, &h->c_tab, &h->c_a, &h->m_tab, &h->m_sigma2, &h->f_tail, &h->f_spread, &h->a_part_d, &h->a_part_a0, &h->a_part_q, &h->a_part_n,
             &h->k_H, &h->k_flag, &h->k_nb, &h->k_rtsr, &h->k_eq, &h->ds_tab, &h->ds_a, &h->md_tab, &h->md_a);
    dft_plans_free(h->dft);
    dft_alloc_free(h->alloc);
    free_dev(&h->da_tab, &h->da_a, &h->ma_tab, &h->ma_a);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->ev_up) (void)hipEventDestroy(h->ev_up);
    if (h->ev_s1) (void)hipEventDestroy(h->ev_s1);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return OFDM_OK;
}

int ofdm_rx_set_profiling(ofdm_rx* h, int32_t enable) {
    if (!h) return fail(OFDM_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (enable && !h->ev[0])
        for (auto& e : h->ev) HIP_TRY(hipEventCreate(&e));
    h->profiling = enable != 0;
    h->prof_calls = 0;
    return OFDM_OK;
}

int ofdm_rx_get_kernel_ms(ofdm_rx* h, float* sync_ms, float* demod_ms) {
    if (!h || !h->ev[0] || h->prof_calls == 0) return fail(OFDM_ERR_INVALID, "profiling was not enabled / no call recorded");
    HIP_TRY(hipSetDevice(h->cfg.device));
    // mean over the calls recorded since ofdm_rx_set_profiling (at most the last PROF_RING of them)
    const int64_t n = h->prof_calls < ofdm_rx::PROF_RING ? h->prof_calls : ofdm_rx::PROF_RING;
    double ssum = 0, dsum = 0;
    for (int64_t c = h->prof_calls - n; c < h->prof_calls; ++c) {
        hipEvent_t* e = h->ev + 3 * (c % ofdm_rx::PROF_RING);
        HIP_TRY(hipEventSynchronize(e[2]));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, e[0], e[1]));
        HIP_TRY(hipEventElapsedTime(&b, e[1], e[2]));
        ssum += a;
        dsum += b;
    }
    if (sync_ms) *sync_ms = float(ssum / double(n));
    if (demod_ms) *demod_ms = float(dsum / double(n));
    return OFDM_OK;
}

#ifdef OFDM_EXPERIMENTS
// Bench-only build (tools/experiments/ofdm_experiments.h): kernel tuning variants and the s_memtime-stamped diagnostic.
// Not part of the product ABI and not compiled into libofdm_mi355x.so.
int ofdm_exp_set_variant(ofdm_rx* h, int32_t variant) {
    if (!h || variant < 0) return fail(OFDM_ERR_INVALID, "bad argument");
    h->variant = variant;
    return OFDM_OK;
}

int ofdm_exp_set_stamp_buffer(ofdm_rx* h, void* d_stamps) {
    if (!h) return fail(OFDM_ERR_INVALID, "null handle");
    h->d_stamps = static_cast<unsigned*>(d_stamps);
    return OFDM_OK;
}
#endif

int ofdm_rx_set_sync_search(ofdm_rx* h, int32_t exhaustive) {
    if (!h) return fail(OFDM_ERR_INVALID, "null handle");
    h->scan_block = exhaustive ? 0 : rx_sync_scan_block(h->dev);
    if (h->scan_block > 0 && !h->d_scan_g) h->scan_block = 0;
    return h->scan_block > 0 ? 1 : 0;
}

int ofdm_rx_set_max_trials(ofdm_rx* h, int32_t max_trials) {
    if (!h || max_trials < 0) return fail(OFDM_ERR_INVALID, "bad argument");
    h->max_trials = max_trials;
    return OFDM_OK;
}

int ofdm_rx_create(const ofdm_rx_cfg* c, ofdm_rx** out) {
    if (!c || !out) return fail(OFDM_ERR_INVALID, "ofdm_rx_create: null argument");
    *out = nullptr;
    if (int bad = check_nfft(c->nfft)) return bad;
    if (c->cp_len < 0 || c->cp_len >= c->nfft) return fail(OFDM_ERR_INVALID, "cp_len=%d out of range", c->cp_len);
    if (int bad = check_bins(c->nfft, c->num_synch_bins, c->num_data_bins)) return bad;
    if (int bad = check_pattern(c->synch_S, c->synch_D, c->num_ofdm_symb)) return bad;
    if (c->modulation != 1 && c->modulation != 2 && c->modulation != 4 && c->modulation != 6)
        return fail(OFDM_ERR_INVALID, "modulation must be 1, 2, 4 or 6 bits per symbol");
    if (c->compat == OFDM_COMPAT_RXOFDM && c->cp_len < 2)
        return fail(OFDM_ERR_INVALID, "gr-RXOFDM search stride is cp_len-1: cp_len must be >= 2");
    if (c->compat != OFDM_COMPAT_UTSA && c->compat != OFDM_COMPAT_RXOFDM) return fail(OFDM_ERR_INVALID, "bad compat");

    HIP_TRY(hipSetDevice(c->device));
    ofdm_rx* h = new (std::nothrow) ofdm_rx();
    if (!h) return fail(OFDM_ERR_NOMEM, "out of host memory");
    h->cfg = *c;
    const int N = c->nfft, Ks = c->num_synch_bins, Kd = c->num_data_bins, S = c->synch_S;
    const int MM = S * Ks;
    RxDev& d = h->dev;
    const int root = fill_rxdev(*c, d);

    int rc = OFDM_OK;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        rc = fail(OFDM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if (rc == OFDM_OK && (hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
                          hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming) != hipSuccess ||
                          hipEventCreateWithFlags(&h->ev_s1, hipEventDisableTiming) != hipSuccess))
        rc = fail(OFDM_ERR_HIP, "second stream / events of the stream block");
    // utsa: parity of MM decides the ZC form (:56); gr-RXOFDM: parity of num_synch_bins (synch_and_chan_est.py:56-61)
    auto zc = make_zc(MM, root, c->compat == OFDM_COMPAT_UTSA ? MM : Ks);
    const size_t rows = size_t(c->num_ofdm_symb);
    if (rc == OFDM_OK) rc = upload_rx_tables(d, &h->d_tw, &h->d_zc, zc);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->d_edf, rows * Kd);
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_pack, rows * Kd);
    if (rc == OFDM_OK && (hipHostMalloc(reinterpret_cast<void**>(&h->pin_tsr), 4 * sizeof(int), hipHostMallocMapped) != hipSuccess ||
                          hipHostMalloc(reinterpret_cast<void**>(&h->pin_in), ofdm_rx::PIN_IN_BYTES, hipHostMallocMapped) != hipSuccess ||
                          hipHostMalloc(reinterpret_cast<void**>(&h->pin_out), ofdm_rx::PIN_OUT_BYTES, hipHostMallocMapped) != hipSuccess ||
                          hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pin_tsr_dev), h->pin_tsr, 0) != hipSuccess ||
                          hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pin_in_dev), h->pin_in, 0) != hipSuccess ||
                          hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pin_out_dev), h->pin_out, 0) != hipSuccess))
        rc = fail(OFDM_ERR_NOMEM, "pinned host allocation failed");
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_tsr, 4);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_H, size_t(2) * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_htime, size_t(2) * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_esf, size_t(2) * MM);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_eqg, size_t(Ks));
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_gain, size_t(Kd));
    if (rc == OFDM_OK) rc = dev_alloc(&h->s_ysc, size_t(MM));
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_trial_m, size_t(ofdm_rx::TRIAL_CAP));
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_trial_d, size_t(ofdm_rx::TRIAL_CAP));
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_partial, size_t(DEMAP_PARTIALS));
    // work queue of the batch demod launch: two words, zero between launches (the kernel re-arms them itself)
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->d_work, 2, "work queue init failed");
    h->scan_block = rx_sync_scan_block(d);
    if (rc == OFDM_OK && h->scan_block > 0) {
        rc = upload(&h->d_scan_g, make_scan_table(N, Ks, zc), "scan table upload failed");
        if (rc == OFDM_OK) rc = upload(&h->d_seg_state, SEG_STATE_0, 2, "segment state upload failed");
        h->seg_armed = rc == OFDM_OK;
    }
    if (rc != OFDM_OK) return create_failed(h, rc, ofdm_rx_destroy);
#ifdef OFDM_EXPERIMENTS
    if (const char* ev = std::getenv("OFDM_EXP_VARIANT")) h->variant = std::atoi(ev);   // run a whole test suite on one variant
#endif
    if (const char* q = std::getenv("OFDM_MI355X_DEMOD_QUEUE")) h->use_queue = std::atoi(q) != 0;   // 0: one chunk per workgroup (A/B)
    *out = h;
    return OFDM_OK;
}

int ofdm_rx_reserve(ofdm_rx* h, int64_t n_frames) {
    if (!h || n_frames < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve: bad argument");
    if (n_frames <= h->cap_frames) return OFDM_OK;
    h->last_frames = 0;                  // the rows of f_H go with the old buffer: none until the next ofdm_rx_demod_frames
    h->tail_frames = -1;                 // ... and so do the tail powers
    h->spread_frames = -1;               // ... and the spreads
    return regrow(h, {{&h->cap_frames, n_frames}}, ws_buf(&h->f_tsr, size_t(n_frames) * 4),
                  ws_buf(&h->f_H, size_t(n_frames) * h->dev.nfft), ws_buf(&h->f_gain, size_t(n_frames) * h->dev.Kd),
                  ws_buf(&h->f_htime, size_t(n_frames) * h->dev.nfft), ws_buf(&h->f_tail, size_t(n_frames)),
                  ws_buf(&h->f_spread, size_t(n_frames)));
}

}  // extern "C"

int rx_sync_leg(ofdm_rx* h, const cf* iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len, hipStream_t s) {
    SyncArgs sa{};
    sa.iq = iq;
    sa.frame_stride = frame_stride;
    sa.frame_len = frame_len;
    sa.n_frames = int(n_frames);
    sa.mode = 0;
    sa.p_begin = 0;
    sa.p_count = h->max_trials;
    sa.force_accept = 0;
    sa.tsr = h->f_tsr;
    sa.H = h->f_H;
    sa.H_for_gain = nullptr;
    sa.gain = h->f_gain;
    sa.htime = nullptr;                  // est_chan_time is computed on demand (ofdm_rx_get_frame_state)
    sa.scan_block = h->scan_block;       // screened search where its preconditions hold (same outcome as the exhaustive one)
    sa.scan_g = h->d_scan_g;
#ifdef OFDM_EXPERIMENTS
    sa.stamps = h->d_stamps;
#endif
    HIP_TRY(launch_rx_sync(h->dev, sa, s));
    h->last_frames = n_frames;           // rows of f_H this call wrote (ofdm_rx_csi_frames)
    h->tail_frames = -1;
    h->spread_frames = -1;
    return OFDM_OK;
}

extern "C" {

int64_t ofdm_rx_demod_frames(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride,
                             int64_t frame_len, float* d_eq, uint8_t* d_bits, int32_t bits_mode, int32_t* d_tsr,
                             void* stream) {
    if (!h || !d_iq || n_frames < 0 || frame_len < 0 || frame_stride < frame_len)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames: bad argument");
    const RxDev& d = h->dev;
    const int SD = d.S + d.D;
    const int64_t n_unique = frame_len / d.L;
    const int64_t n_pat = n_unique / SD;
    const int64_t n_dsym = n_pat * d.D;
    const char* bad = demod_bad_args(d, n_frames, n_dsym, d_bits, bits_mode);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s", bad);
    if (n_frames == 0) return n_dsym;
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (n_frames > h->cap_frames) {
        int rc = ofdm_rx_reserve(h, n_frames);
        if (rc != OFDM_OK) return rc;
    }
    hipStream_t s = pick_stream(h, stream);

    const cf* iq = reinterpret_cast<const cf*>(d_iq);
    hipEvent_t* pev = h->ev + 3 * (h->prof_calls % ofdm_rx::PROF_RING);
    if (h->profiling) HIP_TRY(hipEventRecord(pev[0], s));
    if (const int rc = rx_sync_leg(h, iq, n_frames, frame_stride, frame_len, s)) return rc;
    if (h->avg_n != 0) {                 // the estimate averaged over the frame's sync symbols, in place (capi_chanavg.hip)
        const int rc = chan_average_in_place(h, iq, n_frames, frame_stride, frame_len, s);
        if (rc != OFDM_OK) return rc;
    }
    if (h->win_post > 0) {               // delay-window denoising, in place on the rows the sync launch just wrote (capi_chanwin.hip)
        ChanWinArgs wa{};
        wa.H_in = h->f_H;
        wa.tsr = h->f_tsr;
        wa.n_rows = n_frames;
        wa.pre = h->win_pre;
        wa.post = h->win_post;
        wa.H_out = h->f_H;
        wa.gain = h->f_gain;
        wa.tail = h->f_tail;
        HIP_TRY(launch_chan_window(d, wa, s));
        h->tail_frames = n_frames;
    }
    if (h->profiling) HIP_TRY(hipEventRecord(pev[1], s));

    if (n_dsym > 0 && (d_eq || d_bits)) {
        DemodArgs da{};
        da.iq = iq;
        da.frame_stride = frame_stride;
        da.frame_len = frame_len;
        da.n_frames = int(n_frames);
        da.tsr = h->f_tsr;
        da.gain = h->f_gain;
        da.eq = reinterpret_cast<cf*>(d_eq);
        da.bits = d_bits;
        da.bits_mode = bits_mode;
        da.mod = d.bps;
        da.n_dsym = int(n_dsym);
        da.spc = 0;                 // launcher picks the chunking (multiples of its slots per workgroup)
        da.chunks_per_frame = 0;
        da.row_stride_pat = d.D;
        da.rows_per_frame = int(n_dsym);
        da.zero_skipped = 1;
        da.variant = h->variant;
        da.stamps = h->d_stamps;
        da.work = h->use_queue ? h->d_work : nullptr;
        HIP_TRY(launch_rx_demod(d, da, s));
    }
    if (h->profiling) {
        HIP_TRY(hipEventRecord(pev[2], s));
        h->prof_calls += 1;
    }
    if (d_tsr) HIP_TRY(hipMemcpyAsync(d_tsr, h->f_tsr, size_t(n_frames) * 4 * sizeof(int), hipMemcpyDeviceToDevice, s));
    return n_dsym;
}

int ofdm_rx_get_frame_state(ofdm_rx* h, int64_t frame, float* h_chan_freq, float* h_gain, float* h_chan_time) {
    if (!h || frame < 0 || frame >= h->cap_frames) return fail(OFDM_ERR_INVALID, "ofdm_rx_get_frame_state: bad frame");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    const int N = h->dev.nfft, Kd = h->dev.Kd;
    if (h_chan_freq) HIP_TRY(hipMemcpy(h_chan_freq, h->f_H + frame * N, size_t(N) * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_gain) HIP_TRY(hipMemcpy(h_gain, h->f_gain + frame * Kd, size_t(Kd) * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_chan_time) {                   // ifft of the frame's est_chan_freq_P row, now (SynchAndChanEst.py:202,212)
        HIP_TRY(launch_rx_chan_time(h->dev, h->f_H + frame * N, h->f_htime + frame * N, 1, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(h_chan_time, h->f_htime + frame * N, size_t(N) * sizeof(cf), hipMemcpyDeviceToHost));
    }
    return OFDM_OK;
}

int ofdm_rx_get_state(ofdm_rx* h, int32_t row, float* h_chan_freq, float* h_chan_time, float* h_synch_freq,
                      float* h_eq_gain, float* h_data_freq) {
    if (!h || row < 0 || row > 1) return fail(OFDM_ERR_INVALID, "ofdm_rx_get_state: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int N = h->dev.nfft, Kd = h->dev.Kd, Ks = h->dev.Ks, MM = h->dev.MM;
    if (h_chan_freq) HIP_TRY(hipMemcpy(h_chan_freq, h->s_H + size_t(row) * N, size_t(N) * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_chan_time) HIP_TRY(hipMemcpy(h_chan_time, h->s_htime + size_t(row) * N, size_t(N) * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_synch_freq) HIP_TRY(hipMemcpy(h_synch_freq, h->s_esf + size_t(row) * MM, size_t(MM) * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_eq_gain) HIP_TRY(hipMemcpy(h_eq_gain, h->s_eqg, size_t(Ks) * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_data_freq)
        HIP_TRY(hipMemcpy(h_data_freq, h->d_edf, size_t(h->cfg.num_ofdm_symb) * Kd * sizeof(cf), hipMemcpyDeviceToHost));
    return OFDM_OK;
}

// ---- stream block (SynchAndChanEst.work): the pieces its three search paths share
}  // extern "C"
namespace {
hipError_t upload_in(ofdm_rx* h, const float* h_in, int64_t from, int64_t to, hipStream_t s) {
    return hipMemcpyAsync(h->d_in + from, h_in + 2 * from, size_t(to - from) * sizeof(cf), hipMemcpyHostToDevice, s);
}

int deleted_rows(int rows, int SD) {                                         // :249 (literal 3)
    int n_del = 0;
    for (int r = 3; r < rows; r += SD) ++n_del;
    return n_del;
}

// Finalising search of one buffer: the LS estimate, gains and est_chan_time of the accepted trial go to state row `row` (:171-218).
// The caller adds the trial range: segments on the screened paths, the one forced trial on the exhaustive one.
SyncArgs final_args(const ofdm_rx* h, const cf* iq, int64_t n_in, int row) {
    const RxDev& d = h->dev;
    SyncArgs fa{};
    fa.iq = iq;
    fa.frame_stride = n_in;
    fa.frame_len = n_in;
    fa.n_frames = 1;
    fa.mode = 0;
    fa.tsr = h->s_tsr;
    fa.H = h->s_H + size_t(row) * d.nfft;
    fa.H_for_gain = (row == 0) ? nullptr : h->s_H;                           // :242 always row 0
    fa.gain = h->s_gain;
    fa.htime = h->s_htime + size_t(row) * d.nfft;
    fa.esf = h->s_esf + size_t(row) * d.MM;
    fa.eqg = h->s_eqg;
    fa.yscratch = h->s_ysc;
    return fa;
}

// Screened search (same outcome as trial-by-trial, see rx_sync_scan_kernel): search, accept and finalize in ONE launch
// straight into the state rows the accepted trial would get; a miss leaves the state as it was.  The trial range is
// searched in parallel segments (a continuing stream finds its next sync ~3 symbols into the buffer, :168).
void add_segments(SyncArgs& fa, const ofdm_rx* h, int64_t p0, int64_t p_valid) {
    fa.p_begin = int(p0);
    fa.p_count = int(p_valid);
    fa.keep_on_miss = 1;
    fa.scan_block = h->scan_block;
    fa.scan_g = h->d_scan_g;
    fa.seg_len = h->scan_block;                                              // one screening block per workgroup
    fa.n_seg = int((p_valid - p0 + fa.seg_len - 1) / fa.seg_len);
    fa.seg_state = h->d_seg_state;
}

// Loop B of the stream block on the device: n_dsym data symbols into est_data_freq, a skipped pattern keeps its old rows (:223)
DemodArgs loop_b_args(const ofdm_rx* h, const cf* iq, int64_t n_in, int64_t n_dsym) {
    DemodArgs da{};
    da.iq = iq;
    da.frame_stride = n_in;
    da.frame_len = n_in;
    da.n_frames = 1;
    da.tsr = h->s_tsr;
    da.gain = h->s_gain;
    da.eq = h->d_edf;
    da.mod = h->dev.bps;
    da.n_dsym = int(n_dsym);
    da.row_stride_pat = h->dev.S + h->dev.D;
    da.rows_per_frame = h->cfg.num_ofdm_symb;
    da.zero_skipped = 0;
    da.variant = h->variant;
    return da;
}

struct Found {
    int detected = 0, trials_run = 0;
};

// The four words a screened search left {tsr0, lag, int(peak), accepted} become block state; trials p0 .. p_valid-1 were searched.
void take_search_result(ofdm_rx* h, const int* t4, int64_t p0, int64_t p_valid, Found& f) {
    if (t4[3]) {
        h->corr_obs += 1;                                                    // :171
        h->tsr[0] = t4[0];                                                   // :173-175
        h->tsr[1] = t4[1];
        h->tsr[2] = t4[2];
        f.detected = 1;
        f.trials_run = int((int64_t(t4[0]) - h->dev.cp) / h->dev.stride - p0 + 1);
    } else {
        f.trials_run = int(p_valid - p0);
    }
}

void fill_report(const ofdm_rx* h, ofdm_rx_report* rep, const Found& f, int64_t n_data_items) {
    if (!rep) return;
    rep->time_synch_ref[0] = h->tsr[0];
    rep->time_synch_ref[1] = h->tsr[1];
    rep->time_synch_ref[2] = h->tsr[2];
    rep->detected = f.detected;
    rep->trials_run = f.trials_run;
    rep->count = h->count;
    rep->corr_obs = h->corr_obs;
    rep->n_data_items = n_data_items;
}

// ---- one-synchronisation path.  Nothing the host decides between the search and the output depends on the search's
// result when (a) every data row any pattern could need exists (no IndexError whatever tsr0 turns out to be), (b) the
// reshape of :255 and the output size are fine (both known up front): then the search, Loop B (its guard :223 is
// evaluated on the device against the tsr the search leaves there), the row deletion and both copies are queued
// back to back and the host waits ONCE.  Round 2 waited after the search, after Loop B and after the copy-out and
// repacked the rows on the host: 0.37-0.40 ms per 240-symbol buffer, 0.09-0.10 ms per 4-symbol buffer.
bool one_sync_ok(const ofdm_rx* h, int64_t n_unique, int64_t n_data_symb, int64_t kept, int64_t n_out) {
    const RxDev& d = h->dev;
    const int SD = d.S + d.D;
    const int64_t n_pat_all = (n_unique + SD - 1) / SD;
    const bool rows_ok = n_pat_all == 0 || (n_pat_all - 1) * SD + d.D - 1 < h->cfg.num_ofdm_symb;
    const bool shape_ok = kept == n_data_symb && (h->count == 0 || n_data_symb * d.Kd <= n_out);
    return rows_ok && shape_ok && h->seg_armed;
}

int64_t work_one_sync(ofdm_rx* h, const float* h_in, int64_t n_in, float* h_out, int64_t n_out, ofdm_rx_report* rep, int64_t p0,
                      int64_t p_valid, int row, int64_t n_data_symb) {
    const RxDev& d = h->dev;
    const int N = d.nfft, L = d.L, S = d.S, D = d.D, Kd = d.Kd, SD = S + D;
    hipStream_t s = h->stream;
    const size_t out_bytes = size_t(n_data_symb) * Kd * sizeof(cf);
    const bool in_place_in = size_t(n_in) * sizeof(cf) <= ofdm_rx::PIN_IN_BYTES;
    const bool in_place_out = out_bytes <= ofdm_rx::PIN_OUT_BYTES;
    const cf* iq_dev = in_place_in ? h->pin_in_dev : h->d_in;
    SyncArgs fa = final_args(h, iq_dev, n_in, row);
    add_segments(fa, h, p0, p_valid);
    fa.tsr_host = h->pin_tsr_dev;
    h->seg_armed = false;
    // samples the first SYNC_STAGE_SEGS segments can touch: their last trial's windows and screening edges
    const int64_t head = p0 + int64_t(SYNC_STAGE_SEGS) * fa.seg_len + int64_t(S) * L + N + d.cp + 64;
    if (in_place_in) {
        std::memcpy(h->pin_in, h_in, size_t(n_in) * sizeof(cf));
        fa.seg_final = 1;
        HIP_TRY(launch_rx_sync(d, fa, s));
    } else if (fa.n_seg > 2 * SYNC_STAGE_SEGS && head < n_in / 2) {
        HIP_TRY(upload_in(h, h_in, 0, head, s));
        HIP_TRY(hipEventRecord(h->ev_up, s));
        HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_up, 0));
        fa.seg_base = 0;
        fa.seg_launch = SYNC_STAGE_SEGS;
        fa.seg_final = 2;                                // a hit in the first stage is finalized under the upload too
        HIP_TRY(launch_rx_sync(d, fa, h->stream2));
        HIP_TRY(hipEventRecord(h->ev_s1, h->stream2));
        HIP_TRY(upload_in(h, h_in, head, n_in, s));      // (pageable source: the host is held here while stage 1 runs)
        HIP_TRY(hipStreamWaitEvent(s, h->ev_s1, 0));
        fa.seg_base = SYNC_STAGE_SEGS;
        fa.seg_launch = fa.n_seg - SYNC_STAGE_SEGS;
        fa.seg_final = 1;
        HIP_TRY(launch_rx_sync(d, fa, s));
    } else {
        HIP_TRY(upload_in(h, h_in, 0, n_in, s));
        fa.seg_final = 1;
        HIP_TRY(launch_rx_sync(d, fa, s));
    }
    const int64_t n_dsym_all = (n_in / L + SD - 1) / SD * D;                 // the device applies the guard per pattern
    if (n_dsym_all > 0) HIP_TRY(launch_rx_demod(d, loop_b_args(h, iq_dev, n_in, n_dsym_all), s));
    if (h->count > 0) {                                                      // :257
        HIP_TRY(launch_pack_rows(h->d_edf, h->cfg.num_ofdm_symb, Kd, SD, in_place_out ? h->pin_out_dev : h->d_pack, s));
        if (!in_place_out) HIP_TRY(hipMemcpyAsync(h_out, h->d_pack, out_bytes, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));                                        // the one wait of this call
    if (h->count > 0 && in_place_out) std::memcpy(h_out, h->pin_out, out_bytes);
    h->seg_armed = true;
    Found f;
    take_search_result(h, h->pin_tsr, p0, p_valid, f);
    h->count += 1;                                                           // :260
    h->corr_obs = 0;                                                         // :261
    fill_report(h, rep, f, n_data_symb * Kd);
    return n_out;                                                            // :262
}
}  // namespace
extern "C" {

int64_t ofdm_rx_work(ofdm_rx* h, const float* h_in, int64_t n_in, float* h_out, int64_t n_out, ofdm_rx_report* rep) {
    if (!h || (!h_in && n_in > 0) || (!h_out && n_out > 0) || n_in < 0 || n_out < 0)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_work: bad argument");
    const RxDev& d = h->dev;
    const int N = d.nfft, L = d.L, S = d.S, D = d.D, Kd = d.Kd, SD = S + D, rows = h->cfg.num_ofdm_symb;
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    int rc = grow_input(&h->d_in, &h->in_cap, n_in, s);
    if (rc != OFDM_OK) return rc;

    const int64_t n_unique = n_in / L;                                       // :140
    const int64_t n_data_symb = int64_t(double(n_unique) * (double(D) / double(SD)));   // :141 int(n * (D/(S+D)))
    const int64_t kept = rows - deleted_rows(rows, SD);                      // rows the output keeps (:249-255)

    // ---------------- Loop A: sliding sync search, first accepted trial wins (:143-219)
    Found f;
    const int64_t p_valid = valid_trials(d, n_in);
    int64_t p0 = 0;
    if (h->corr_obs != -1) {
        // After the first call a trial can only be accepted if P*stride + cp - tsr0 > 2cp + N (:168): earlier trials
        // are evaluated by the reference but can never win, so they are skipped (identical outcome).
        const int64_t need = int64_t(h->tsr[0]) + d.cp + N;                  // P*stride > need
        p0 = need >= 0 ? need / d.stride + 1 : 0;
    }
    // The screened search is used where its preconditions hold.  The row past the estimate arrays (the reference's
    // IndexError) is left to the exhaustive path, which raises it.
    const bool screened = h->scan_block > 0 && p0 < p_valid && p_valid < (int64_t(1) << 30) && h->corr_obs + 1 < rows;
    const int next_row = h->corr_obs + 1 > 1 ? 1 : h->corr_obs + 1;
    // The upload is issued where the search is set up: the one-synchronisation path sends the head of the buffer first and
    // runs the first stage of the search under the rest of it.
    if (screened && one_sync_ok(h, n_unique, n_data_symb, kept, n_out))
        return work_one_sync(h, h_in, n_in, h_out, n_out, rep, p0, p_valid, next_row, n_data_symb);
    if (n_in > 0) HIP_TRY(upload_in(h, h_in, 0, n_in, s));

    if (screened) {   // ---- screened search, host decisions (Loop B, packing) after it
        SyncArgs fa = final_args(h, h->d_in, n_in, next_row);
        add_segments(fa, h, p0, p_valid);
        if (!h->seg_armed) {                                       // an earlier search did not run to its end: start clean
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(hipMemcpy(h->d_seg_state, SEG_STATE_0, sizeof SEG_STATE_0, hipMemcpyHostToDevice));
        }
        h->seg_armed = false;
        fa.seg_final = 1;
        HIP_TRY(launch_rx_sync(d, fa, s));
        int t4[4];
        HIP_TRY(hipMemcpyAsync(t4, h->s_tsr, sizeof(t4), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->seg_armed = true;
        take_search_result(h, t4, p0, p_valid, f);
        p0 = p_valid;
    }

    // ---- exhaustive search, window by window: the host applies the gate and the distance rule to every trial
    int win = 128;
    std::vector<float> tm(ofdm_rx::TRIAL_CAP);
    std::vector<int> td(ofdm_rx::TRIAL_CAP);
    while (p0 < p_valid && !f.detected) {
        const int cnt = int(std::min<int64_t>(win, p_valid - p0));
        HIP_TRY(launch_rx_sync(d, trial_window_args(h->d_in, n_in, p0, cnt, h->d_trial_m, h->d_trial_d), s));
        HIP_TRY(hipMemcpyAsync(tm.data(), h->d_trial_m, size_t(cnt) * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(td.data(), h->d_trial_d, size_t(cnt) * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int w = 0; w < cnt; ++w) {
            const int64_t P = p0 + w;
            ++f.trials_run;
            if (!(tm[w] > d.gate_mm)) continue;                                              // :166
            const double pos = double(P * d.stride + d.cp);
            if (!(h->corr_obs == -1 || pos - h->tsr[0] > double(2 * d.cp + N))) continue;    // :168-169
            // finalize this trial on the device: LS estimate, gains, est_chan_time (:171-218)
            h->corr_obs += 1;                                                                // :171
            if (h->corr_obs >= rows)
                return fail(OFDM_ERR_INDEX, "est_chan_freq_P has %d rows, corr_obs=%d (the reference raises IndexError)", rows,
                            h->corr_obs);
            SyncArgs fa = final_args(h, h->d_in, n_in, h->corr_obs > 1 ? 1 : h->corr_obs);
            fa.p_begin = int(P);
            fa.p_count = 1;
            fa.force_accept = 1;
            HIP_TRY(launch_rx_sync(d, fa, s));
            int t4[4];
            HIP_TRY(hipMemcpyAsync(t4, h->s_tsr, sizeof(t4), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            h->tsr[0] = t4[0];                                                               // :173-175
            h->tsr[1] = t4[1];
            h->tsr[2] = t4[2];
            f.detected = 1;
            break;                                                                           // :219
        }
        p0 += cnt;
        if (win < ofdm_rx::TRIAL_CAP) win *= 2;
    }
    fill_report(h, rep, f, n_data_symb * Kd);   // valid even if the call fails below, like the attributes the reference has already updated

    // ---------------- Loop B: data demod (:221-248)
    // The reference works symbol by symbol and raises IndexError from the first row that does not exist (:248) AFTER having
    // written every earlier row; the same rows are written here before the error is returned.  A window that starts past the
    // buffer is not an error: np.fft.fft(x, nfft) zero-pads even an empty slice (:230), the row becomes 0 * inf = NaN there
    // and here alike.
    const int64_t tsr0 = int64_t(h->tsr[0]);
    const int64_t n_pat_loop = (n_unique + SD - 1) / SD;                     // range(n_unique)[::S+D]
    int64_t n_dsym_run = 0;                                                  // data symbols the reference gets through
    int loop_b_err = OFDM_OK;
    char loop_b_msg[160] = "";
    for (int64_t p = 0; p < n_pat_loop && loop_b_err == OFDM_OK; ++p) {
        const int64_t ptr = tsr0 + int64_t(S) * L * (p * SD + 1);            // :222
        if (!(ptr + N - 1 <= n_in)) continue;                                // :223 (monotonic: later patterns fail too)
        for (int n = 0; n < D; ++n) {
            if (p * SD + n >= rows) {
                loop_b_err = OFDM_ERR_INDEX;
                snprintf(loop_b_msg, sizeof loop_b_msg, "est_data_freq has %d rows, pattern %lld needs row %lld (the reference raises IndexError)",
                         rows, (long long)p, (long long)(p * SD + n));
                break;
            }
            n_dsym_run = p * D + n + 1;
        }
    }
    if (n_dsym_run > 0) HIP_TRY(launch_rx_demod(d, loop_b_args(h, h->d_in, n_in, n_dsym_run), s));
    if (loop_b_err != OFDM_OK) {
        HIP_TRY(hipStreamSynchronize(s));
        return fail(loop_b_err, "%s", loop_b_msg);
    }

    // ---------------- output packing (:249-262)
    if (kept * Kd != n_data_symb * Kd)                                       // :255 reshape
        return fail(OFDM_ERR_SHAPE, "cannot reshape %lld kept rows x %d bins into (1, %lld) (the reference raises ValueError)",
                    (long long)kept, Kd, (long long)(n_data_symb * Kd));
    if (h->count > 0) {                                                      // :257
        if (n_data_symb * Kd > n_out)
            return fail(OFDM_ERR_SHAPE, "output buffer holds %lld items, need %lld (the reference raises ValueError)",
                        (long long)n_out, (long long)(n_data_symb * Kd));
        std::vector<cf> host(size_t(rows) * Kd);
        HIP_TRY(hipMemcpyAsync(host.data(), h->d_edf, host.size() * sizeof(cf), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        cf* o = reinterpret_cast<cf*>(h_out);
        int64_t w = 0;
        for (int r = 0; r < rows; ++r) {
            if (r >= 3 && (r - 3) % SD == 0) continue;
            std::memcpy(o + w * Kd, host.data() + size_t(r) * Kd, size_t(Kd) * sizeof(cf));
            ++w;
        }
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    h->count += 1;                                                           // :260
    h->corr_obs = 0;                                                         // :261
    fill_report(h, rep, f, n_data_symb * Kd);
    return n_out;                                                            // :262
}

int ofdm_demap(ofdm_rx* h, const float* d_sym, int64_t n, int32_t modulation, uint8_t* d_hard, float* d_soft0,
               float* d_soft1, void* stream) {
    if (!h || (!d_sym && n > 0) || n < 0) return fail(OFDM_ERR_INVALID, "ofdm_demap: bad argument");
    if (modulation != 1 && modulation != 2 && modulation != 4 && modulation != 6)
        return fail(OFDM_ERR_INVALID, "modulation must be 1, 2, 4 or 6 bits per symbol");
    if ((d_soft0 || d_soft1) && modulation == 1)
        return fail(OFDM_ERR_INVALID, "soft metrics: QPSK (BitRecovery.py) and its 16/64-QAM extension only");
    HIP_TRY(hipSetDevice(h->cfg.device));
    DemapArgs a{};
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n = n;
    a.mod = modulation;
    a.hard = d_hard;
    a.soft0 = d_soft0;
    a.soft1 = d_soft1;
    a.partial = h->d_partial;
    HIP_TRY(launch_demap(a, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
