// capi_trk.hip -- the regression-tracking receiver (SynchronizeAndEstimate.py): handle and the device primitives its Python
// control flow calls (load, trial windows, accept, demod).
#include "capi_internal.hpp"

extern "C" {

int ofdm_trk_destroy(ofdm_trk* h) {
    if (!h) return OFDM_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_dev(&h->d_tw, &h->d_zc, &h->d_in, &h->t_tsr, &h->t_H, &h->t_imp, &h->t_esf, &h->t_gain, &h->t_edf, &h->s_ysc, &h->d_trial_m,
             &h->d_trial_d);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return OFDM_OK;
}

int ofdm_trk_create(const ofdm_trk_cfg* c, ofdm_trk** out) {
    if (!c || !out) return fail(OFDM_ERR_INVALID, "ofdm_trk_create: null argument");
    *out = nullptr;
    if (int bad = check_nfft(c->nfft)) return bad;
    if (c->cp_len < 1 || c->cp_len >= c->nfft) return fail(OFDM_ERR_INVALID, "cp_len=%d out of range", c->cp_len);
    if (int bad = check_bins(c->nfft, c->num_synch_bins, c->num_data_bins)) return bad;
    if (c->synch_D < 1 || c->rows_sync < 1 || c->rows_data < 0) return fail(OFDM_ERR_INVALID, "bad pattern / row counts");
    if (!(c->snr > 0.0)) return fail(OFDM_ERR_INVALID, "snr must be > 0 (linear)");

    HIP_TRY(hipSetDevice(c->device));
    ofdm_trk* h = new (std::nothrow) ofdm_trk();
    if (!h) return fail(OFDM_ERR_NOMEM, "out of host memory");
    h->cfg = *c;
    RxDev& d = h->dev;
    const int N = c->nfft, Ks = c->num_synch_bins, Kd = c->num_data_bins;
    d.nfft = N;
    d.cp = c->cp_len;
    d.L = N + c->cp_len;
    d.Ks = Ks;
    d.Kd = Kd;
    d.S = 1;
    d.D = c->synch_D;
    d.MM = Ks;
    d.bps = 2;
    d.stride = 1;
    d.gate_mm = 0.f;
    d.inv_ls = float(1.0 / (1.0 + 1.0 / c->snr));                     // SynchronizeAndEstimate.py:349
    d.inv_snr_data = float(1.0 / c->snr);                              // :425
    d.inv_snr_eqsync = float(1.0 / c->snr);                            // :377
    const size_t RS = size_t(c->rows_sync), RD = size_t(c->rows_data > 0 ? c->rows_data : 1);

    int rc = OFDM_OK;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) rc = fail(OFDM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    auto zc = make_zc(Ks, c->zc_root, Ks);                             // :123-130 parity of MM = Ks
    if (rc == OFDM_OK) rc = upload_rx_tables(d, &h->d_tw, &h->d_zc, zc);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_tsr, RS * 4);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_H, RS * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_imp, RS * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_esf, RS * Ks);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_gain, RS * Kd);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_edf, RD * Kd);
    if (rc == OFDM_OK) rc = dev_alloc(&h->s_ysc, size_t(Ks));
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_trial_m, size_t(ofdm_trk::TRIAL_CAP));
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_trial_d, size_t(ofdm_trk::TRIAL_CAP));
    if (rc != OFDM_OK) return create_failed(h, rc, ofdm_trk_destroy);
    *out = h;
    return OFDM_OK;
}

int ofdm_trk_load(ofdm_trk* h, const float* h_in, int64_t n_in) {
    if (!h || (!h_in && n_in > 0) || n_in < 0) return fail(OFDM_ERR_INVALID, "ofdm_trk_load: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int rc = grow_input(&h->d_in, &h->in_cap, n_in, h->stream);
    if (rc != OFDM_OK) return rc;
    if (n_in > 0) HIP_TRY(hipMemcpyAsync(h->d_in, h_in, size_t(n_in) * sizeof(cf), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // the caller's buffer is only valid during work()
    h->n_in = n_in;
    return OFDM_OK;
}

int ofdm_trk_trials(ofdm_trk* h, int64_t first_ptr, int32_t step, int32_t count, float* h_peak, int32_t* h_lag) {
    if (!h || !h_peak || !h_lag || count < 0 || step < 1 || first_ptr < 0)
        return fail(OFDM_ERR_INVALID, "ofdm_trk_trials: bad argument");
    if (count == 0) return OFDM_OK;
    const RxDev& d0 = h->dev;
    if (first_ptr + int64_t(count - 1) * step + d0.nfft > h->n_in)
        return fail(OFDM_ERR_INVALID, "window %lld..+%d reaches past the loaded buffer (%lld samples)",
                    (long long)(first_ptr + int64_t(count - 1) * step), d0.nfft, (long long)h->n_in);
    HIP_TRY(hipSetDevice(h->cfg.device));
    RxDev d = d0;
    d.stride = step;
    for (int32_t done = 0; done < count; done += ofdm_trk::TRIAL_CAP) {
        const int cnt = std::min<int>(ofdm_trk::TRIAL_CAP, count - done);
        SyncArgs sa = trial_window_args(h->d_in, h->n_in, done, cnt, h->d_trial_m, h->d_trial_d);
        sa.off_delta = int(first_ptr) - d.cp;                         // window start = first_ptr + P*step
        sa.host_valid = 1;
        HIP_TRY(launch_rx_sync(d, sa, h->stream));
        HIP_TRY(hipMemcpyAsync(h_peak + done, h->d_trial_m, size_t(cnt) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(h_lag + done, h->d_trial_d, size_t(cnt) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return OFDM_OK;
}

int ofdm_trk_accept(ofdm_trk* h, int32_t row, int64_t window_ptr, int32_t lag_sync, int32_t lag_data) {
    if (!h || row < 0 || window_ptr < 0) return fail(OFDM_ERR_INVALID, "ofdm_trk_accept: bad argument");
    const RxDev& d = h->dev;
    if (row >= h->cfg.rows_sync)
        return fail(OFDM_ERR_INDEX, "est_chan_freq_p has %d rows, corr_obs=%d (the reference raises IndexError)", h->cfg.rows_sync, row);
    if (lag_sync < 0 || lag_sync > d.cp || window_ptr + d.nfft > h->n_in) return fail(OFDM_ERR_INVALID, "ofdm_trk_accept: lag / window out of range");
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int N = d.nfft;
    SyncArgs fa{};
    fa.iq = h->d_in;
    fa.frame_stride = h->n_in;
    fa.frame_len = h->n_in;
    fa.n_frames = 1;
    fa.mode = 0;
    fa.p_begin = 0;
    fa.p_count = 1;
    fa.force_accept = 1;
    fa.host_valid = 1;
    fa.off_delta = int(window_ptr) - d.cp;
    fa.force_dhat_p1 = lag_sync + 1;
    fa.gain_lag_set = 1;
    fa.gain_lag = lag_data;
    fa.tsr = h->t_tsr + size_t(row) * 4;
    fa.H = h->t_H + size_t(row) * N;
    fa.gain = h->t_gain + size_t(row) * d.Kd;
    fa.htime = h->t_imp + size_t(row) * N;
    fa.esf = h->t_esf + size_t(row) * d.MM;
    fa.yscratch = h->s_ysc;
    HIP_TRY(launch_rx_sync(d, fa, h->stream));
    return OFDM_OK;
}

int ofdm_trk_demod(ofdm_trk* h, int32_t n_sync, const int64_t* h_ptr, const uint8_t* h_guard, float* h_last, int32_t* last_row) {
    if (!h || n_sync < 0 || (n_sync > 0 && (!h_ptr || !h_guard))) return fail(OFDM_ERR_INVALID, "ofdm_trk_demod: bad argument");
    if (last_row) *last_row = -1;
    if (n_sync == 0) return OFDM_OK;
    if (n_sync > h->cfg.rows_sync) return fail(OFDM_ERR_INDEX, "%d syncs, %d rows", n_sync, h->cfg.rows_sync);
    const RxDev& d = h->dev;
    const int D = d.D, Kd = d.Kd;
    HIP_TRY(hipSetDevice(h->cfg.device));
    std::vector<int> tsr(size_t(n_sync) * 4, 0);
    int last = -1;
    for (int p = 0; p < n_sync; ++p) {
        if (h_guard[p] && (h_ptr[p] < 0 || h_ptr[p] > INT32_MAX - int64_t(d.S + D) * d.L))
            // a guarded window that starts before the buffer: the reference's slice would wrap / be empty and the block
            // mirror raises IndexError for it; never hand a negative start to the kernel
            return fail(OFDM_ERR_INDEX, "sync %d: window pointer %lld outside the buffer", p, (long long)h_ptr[p]);
        tsr[size_t(p) * 4 + 0] = h_guard[p] ? int(h_ptr[p]) : 0;
        tsr[size_t(p) * 4 + 3] = h_guard[p] ? 1 : 0;
        if (!h_guard[p]) continue;
        if (p * D + D - 1 >= h->cfg.rows_data)
            return fail(OFDM_ERR_INDEX, "est_data_freq has %d rows, sync %d needs row %d (the reference raises IndexError)",
                        h->cfg.rows_data, p, p * D + D - 1);
        last = p * D + D - 1;
    }
    HIP_TRY(hipMemcpyAsync(h->t_tsr, tsr.data(), tsr.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    DemodArgs da{};
    da.iq = h->d_in;
    da.frame_stride = 0;
    da.frame_len = h->n_in;
    da.n_frames = n_sync;
    da.tsr = h->t_tsr;
    da.gain = h->t_gain;
    da.eq = h->t_edf;
    da.bits = nullptr;
    da.bits_mode = 0;
    da.mod = 2;
    da.n_dsym = D;
    da.spc = 0;
    da.chunks_per_frame = 0;
    da.row_stride_pat = D;
    da.rows_per_frame = D;
    da.zero_skipped = 0;
    da.host_guard = 1;
    HIP_TRY(launch_rx_demod(d, da, h->stream));
    HIP_TRY(launch_row_renorm(h->t_edf, Kd, D, n_sync, h->t_tsr, h->stream));
    if (h_last && last >= 0)
        HIP_TRY(hipMemcpyAsync(h_last, h->t_edf + size_t(last) * Kd, size_t(Kd) * sizeof(cf), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));          // tsr (host vector) must stay alive until the copy has run
    if (last_row) *last_row = last;
    return OFDM_OK;
}

int ofdm_trk_get_state(ofdm_trk* h, float* h_chan_freq, float* h_chan_impulse, float* h_synch_freq, float* h_data_freq) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_trk_get_state: null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const RxDev& d = h->dev;
    const size_t RS = size_t(h->cfg.rows_sync), RD = size_t(h->cfg.rows_data);
    if (h_chan_freq) HIP_TRY(hipMemcpy(h_chan_freq, h->t_H, RS * d.nfft * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_chan_impulse) HIP_TRY(hipMemcpy(h_chan_impulse, h->t_imp, RS * d.nfft * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_synch_freq) HIP_TRY(hipMemcpy(h_synch_freq, h->t_esf, RS * d.Ks * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_data_freq && RD > 0) HIP_TRY(hipMemcpy(h_data_freq, h->t_edf, RD * d.Kd * sizeof(cf), hipMemcpyDeviceToHost));
    return OFDM_OK;
}

}  // extern "C"
