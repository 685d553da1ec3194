// capi_fo.hip -- the CFO-search receiver (SynchEstAndFO.py / SynchEstFOAndDSSS.py): handle, the stream block ofdm_fo_work and the
// frame-batched ofdm_fo_demod_frames.
#include "capi_internal.hpp"

extern "C" {

int ofdm_fo_destroy(ofdm_fo* h) {
    if (!h) return OFDM_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_dev(&h->d_tw, &h->d_zc, &h->d_rot, &h->d_in, &h->t_tsr, &h->t_H, &h->t_htime, &h->t_esf, &h->t_gain, &h->t_edf, &h->d_code,
             &h->t_edfd, &h->s_eqg, &h->s_ysc, &h->d_trial_m, &h->d_trial_d, &h->b_tm, &h->b_td, &h->b_tsr, &h->b_fo, &h->b_gain,
             &h->b_edf);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return OFDM_OK;
}

int ofdm_fo_create(const ofdm_fo_cfg* c, ofdm_fo** out) {
    if (!c || !out) return fail(OFDM_ERR_INVALID, "ofdm_fo_create: null argument");
    *out = nullptr;
    if (int bad = check_nfft(c->nfft)) return bad;
    if (c->cp_len < 2 || c->cp_len >= c->nfft) return fail(OFDM_ERR_INVALID, "cp_len=%d out of range (stride is cp_len-1)", c->cp_len);
    if (int bad = check_bins(c->nfft, c->num_synch_bins, c->num_data_bins)) return bad;
    if (int bad = check_pattern(c->synch_S, c->synch_D, c->num_ofdm_symb)) return bad;
    if (c->n_fo < 1 || (!c->rotators && c->n_fo != 1))
        return fail(OFDM_ERR_INVALID, "fo_range must hold at least one candidate (rotators may be NULL only with n_fo == 1)");
    if (!(c->snr > 0.0)) return fail(OFDM_ERR_INVALID, "snr must be > 0 (linear)");
    if (c->dsss < 0 || c->dsss > c->num_data_bins || (c->dsss > 0 && !c->spread_code))
        return fail(OFDM_ERR_INVALID, "dsss=%d must be 0 or in [1, num_data_bins] with a spreading code", c->dsss);

    HIP_TRY(hipSetDevice(c->device));
    ofdm_fo* h = new (std::nothrow) ofdm_fo();
    if (!h) return fail(OFDM_ERR_NOMEM, "out of host memory");
    h->cfg = *c;
    h->cfg.rotators = nullptr;            // the caller's tables are copied below, never kept
    h->cfg.spread_code = nullptr;
    h->n_spread = c->dsss > 0 ? c->num_data_bins / c->dsss : 0;
    ofdm_rx_cfg rc_cfg{};
    rc_cfg.num_ofdm_symb = c->num_ofdm_symb;
    rc_cfg.nfft = c->nfft;
    rc_cfg.cp_len = c->cp_len;
    rc_cfg.num_synch_bins = c->num_synch_bins;
    rc_cfg.synch_S = c->synch_S;
    rc_cfg.synch_D = c->synch_D;
    rc_cfg.num_data_bins = c->num_data_bins;
    rc_cfg.snr = c->snr;
    rc_cfg.compat = OFDM_COMPAT_RXOFDM;   // same constants: root 37 (FO:167), stride cp-1 (:196), gate 0.4 (:288), linear SNR
    rc_cfg.modulation = 2;
    RxDev& d = h->dev;
    const int root = fill_rxdev(rc_cfg, d);
    const int N = d.nfft, Ks = d.Ks, Kd = d.Kd, MM = d.MM;
    constexpr size_t R = OFDM_FO_MAX_SYNC;

    int rc = OFDM_OK;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) rc = fail(OFDM_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    auto zc = make_zc(MM, root, Ks);                                  // FO:168-176: parity of num_synch_bins
    if (rc == OFDM_OK) rc = upload_rx_tables(d, &h->d_tw, &h->d_zc, zc);
    if (rc == OFDM_OK && c->rotators) rc = upload(&h->d_rot, reinterpret_cast<const cf*>(c->rotators), size_t(c->n_fo) * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_tsr, R * 4);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_H, R * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_htime, R * N);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_esf, R * MM);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_gain, R * Kd);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->t_edf, R * Kd);
    if (rc == OFDM_OK) rc = alloc_zeroed(&h->s_eqg, size_t(Ks));
    if (rc == OFDM_OK) rc = dev_alloc(&h->s_ysc, size_t(MM));
    if (rc == OFDM_OK && c->dsss > 0)
        rc = upload(&h->d_code, reinterpret_cast<const cf*>(c->spread_code), size_t(c->dsss), "spreading-code upload failed: %s");
    if (rc == OFDM_OK && c->dsss > 0) rc = alloc_zeroed(&h->t_edfd, R * size_t(h->n_spread), "spreading-code upload failed: %s");
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_trial_m, size_t(c->n_fo) * ofdm_fo::TRIAL_WIN);
    if (rc == OFDM_OK) rc = dev_alloc(&h->d_trial_d, size_t(c->n_fo) * ofdm_fo::TRIAL_WIN);
    if (rc != OFDM_OK) return create_failed(h, rc, ofdm_fo_destroy);
    *out = h;
    return OFDM_OK;
}

int64_t ofdm_fo_work(ofdm_fo* h, const float* h_in, int64_t n_in, float* h_out, int64_t n_out, ofdm_fo_report* rep) {
    if (!h || (!h_in && n_in > 0) || (!h_out && n_out > 0) || n_in < 0 || n_out < 0)
        return fail(OFDM_ERR_INVALID, "ofdm_fo_work: bad argument");
    const RxDev& d = h->dev;
    const int N = d.nfft, L = d.L, S = d.S, Kd = d.Kd, n_fo = h->cfg.n_fo;
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;

    const int rc = grow_input(&h->d_in, &h->in_cap, n_in, s);
    if (rc != OFDM_OK) return rc;
    if (n_in > 0) HIP_TRY(hipMemcpyAsync(h->d_in, h_in, size_t(n_in) * sizeof(cf), hipMemcpyHostToDevice, s));

    int trials_run = 0;
    auto fill_report = [&](int n_sync) {
        if (!rep) return;
        rep->n_sync = n_sync;
        rep->count = h->count;
        rep->dmax_tmp_ind = h->dmax_tmp_ind;
        rep->trials_run = trials_run;
        rep->n_data_items = int64_t(h->cfg.num_ofdm_symb / (d.S + d.D)) * (h->cfg.dsss > 0 ? h->n_spread : Kd);
    };

    // ---------------- Loop A: every valid trial, every candidate; NO break (FO:248-329)
    {
        const int64_t p_valid = valid_trials(d, n_in);                                       // :246,249
        std::vector<float> tm(size_t(n_fo) * ofdm_fo::TRIAL_WIN);
        std::vector<int> td(size_t(n_fo) * ofdm_fo::TRIAL_WIN);
        for (int64_t p0 = 0; p0 < p_valid; p0 += ofdm_fo::TRIAL_WIN) {
            const int cnt = int(std::min<int64_t>(ofdm_fo::TRIAL_WIN, p_valid - p0));
            SyncArgs sa = trial_window_args(h->d_in, n_in, p0, cnt, h->d_trial_m, h->d_trial_d);
            sa.rot = h->d_rot;
            sa.n_rot = n_fo;
            HIP_TRY(launch_rx_sync(d, sa, s));
            HIP_TRY(hipMemcpyAsync(tm.data(), h->d_trial_m, size_t(cnt) * n_fo * sizeof(float), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(td.data(), h->d_trial_d, size_t(cnt) * n_fo * sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (int w = 0; w < cnt; ++w) {
                const int64_t P = p0 + w;
                ++trials_run;
                int best = 0;                                                                // :282-285 first maximum wins
                for (int fo = 1; fo < n_fo; ++fo)
                    if (tm[size_t(fo) * cnt + w] > tm[size_t(best) * cnt + w]) best = fo;
                const float dmax_val = tm[size_t(best) * cnt + w];
                const int dmax_ind = td[size_t(best) * cnt + w];
                h->dmax_tmp_ind = best;                                                      // :283 (state: the LAST trial's)
                if (!(dmax_val > d.gate_mm)) continue;                                       // :288
                const double pos = double(P * d.stride + d.cp);
                const double ref = h->tsr[h->cor_obs > 0 ? h->cor_obs : 0][0];               // :289
                if (!(pos - ref > double(2 * d.cp + N) || h->cor_obs == -1)) continue;       // :291
                h->cor_obs += 1;                                                             // :294
                if (h->cor_obs >= OFDM_FO_MAX_SYNC) {
                    fill_report(h->cor_obs);
                    return fail(OFDM_ERR_INDEX, "time_synch_ref has %d rows, cor_obs=%d (the reference raises IndexError)",
                                OFDM_FO_MAX_SYNC, h->cor_obs);
                }
                const int row = h->cor_obs;
                h->tsr[row][0] = pos;                                                        // :296-298
                h->tsr[row][1] = double(dmax_ind);
                h->tsr[row][2] = double(int(dmax_val));
                // LS estimate of this sync on the device: sync vector of the LAST candidate, lag of the best one (:300-329)
                SyncArgs fa{};
                fa.iq = h->d_in;
                fa.frame_stride = n_in;
                fa.frame_len = n_in;
                fa.n_frames = 1;
                fa.mode = 0;
                fa.p_begin = int(P);
                fa.p_count = 1;
                fa.force_accept = 1;
                fa.rot = h->d_rot ? h->d_rot + size_t(n_fo - 1) * N : nullptr;
                fa.n_rot = 1;
                fa.force_dhat_p1 = dmax_ind + 1;
                fa.tsr = h->t_tsr + size_t(row) * 4;
                fa.H = h->t_H + size_t(row) * N;
                fa.H_for_gain = nullptr;                                                     // :352 own row
                fa.gain = h->t_gain + size_t(row) * Kd;
                fa.htime = h->t_htime + size_t(row) * N;
                fa.esf = h->t_esf + size_t(row) * d.MM;
                fa.eqg = h->s_eqg;
                fa.yscratch = h->s_ysc;
                HIP_TRY(launch_rx_sync(d, fa, s));
            }
        }
    }
    const int n_sync = h->cor_obs + 1;
    fill_report(n_sync);

    // ---------------- Loop B: one data symbol per sync (FO:332-358)
    if (n_sync > 0) {
        for (int r = 0; r < n_sync; ++r) {
            const int64_t ptr = int64_t(h->tsr[r][0]) + int64_t(S) * L;                      // :335
            if (h->d_rot && ptr + N - 1 <= n_in && ptr + N > n_in)                           // :334 passes, slice has N-1 items
                return fail(OFDM_ERR_SHAPE, "data window of sync %d is one sample short (the reference raises ValueError)", r);
        }
        if (h->cfg.dsss > 0 && !(int64_t(h->tsr[0][0]) + int64_t(S) * L + N - 1 <= n_in))   // DS:362 fails for row 0 ...
            return fail(OFDM_ERR_UNBOUND, "row 0 fails the data guard before any row passed (the reference raises UnboundLocalError, "
                                          "SynchEstFOAndDSSS.py:392)");                       // ... rows >= 1 of this call always pass
        if (h->d_rot && h->dmax_tmp_ind < 0)
            return fail(OFDM_ERR_INVALID, "no trial has ever been evaluated: dmax_tmp_ind is undefined (the reference raises NameError)");
        DemodArgs da{};
        da.iq = h->d_in;
        da.frame_stride = 0;                    // every "frame" is the same buffer seen from another sync
        da.frame_len = n_in;
        da.n_frames = n_sync;
        da.tsr = h->t_tsr;
        da.gain = h->t_gain;
        da.eq = h->t_edf;
        da.bits = nullptr;
        da.bits_mode = 0;
        da.mod = 2;
        da.n_dsym = 1;
        da.spc = 0;
        da.chunks_per_frame = 0;
        da.row_stride_pat = 1;
        da.rows_per_frame = 1;
        da.zero_skipped = 0;
        da.rot = h->d_rot ? h->d_rot + size_t(h->dmax_tmp_ind) * N : nullptr;              // :339 (table mode: none)
        HIP_TRY(launch_rx_demod(d, da, s));
        if (h->cfg.dsss > 0)                                                                 // DS:391-399
            HIP_TRY(launch_despread(h->t_edf, Kd, h->d_code, h->cfg.dsss, h->n_spread, n_sync, h->t_edfd, s));
    }

    // ---------------- output (:362-367)
    const int64_t corr_size = h->cfg.num_ofdm_symb / (d.S + d.D);
    if (corr_size > OFDM_FO_MAX_SYNC)
        return fail(OFDM_ERR_SHAPE, "corr_size=%lld exceeds the %d est_data_freq rows (the reference raises ValueError)",
                    (long long)corr_size, OFDM_FO_MAX_SYNC);
    if (h->cfg.dsss > 0) {                                                                   // DS:403-407: every call
        if (corr_size * h->n_spread > n_out)
            return fail(OFDM_ERR_SHAPE, "output buffer holds %lld items, need %lld (the reference raises ValueError)",
                        (long long)n_out, (long long)(corr_size * h->n_spread));
        if (corr_size * h->n_spread > 0)
            HIP_TRY(hipMemcpyAsync(h_out, h->t_edfd, size_t(corr_size) * h->n_spread * sizeof(cf), hipMemcpyDeviceToHost, s));
    } else if (h->count > 0) {
        if (corr_size * Kd > n_out)
            return fail(OFDM_ERR_SHAPE, "output buffer holds %lld items, need %lld (the reference raises ValueError)",
                        (long long)n_out, (long long)(corr_size * Kd));
        HIP_TRY(hipMemcpyAsync(h_out, h->t_edf, size_t(corr_size) * Kd * sizeof(cf), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->count += 1;                                                                           // :368
    h->cor_obs = 0;                                                                          // :369
    fill_report(n_sync);
    return n_out;
}

int ofdm_fo_get_state(ofdm_fo* h, double* h_tsr, float* h_chan_freq, float* h_chan_time, float* h_synch_freq,
                      float* h_data_freq, float* h_eq_gain) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_fo_get_state: null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const RxDev& d = h->dev;
    constexpr size_t R = OFDM_FO_MAX_SYNC;
    if (h_tsr) std::memcpy(h_tsr, h->tsr, sizeof(h->tsr));
    if (h_chan_freq) HIP_TRY(hipMemcpy(h_chan_freq, h->t_H, R * d.nfft * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_chan_time) HIP_TRY(hipMemcpy(h_chan_time, h->t_htime, R * d.nfft * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_synch_freq) HIP_TRY(hipMemcpy(h_synch_freq, h->t_esf, R * d.MM * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_data_freq) HIP_TRY(hipMemcpy(h_data_freq, h->t_edf, R * d.Kd * sizeof(cf), hipMemcpyDeviceToHost));
    if (h_eq_gain) HIP_TRY(hipMemcpy(h_eq_gain, h->s_eqg, size_t(d.Ks) * sizeof(cf), hipMemcpyDeviceToHost));
    return OFDM_OK;
}

int ofdm_fo_reserve(ofdm_fo* h, int64_t n_frames, int64_t frame_len) {
    if (!h || n_frames < 0 || frame_len < 0) return fail(OFDM_ERR_INVALID, "ofdm_fo_reserve: bad argument");
    const int64_t pv = valid_trials(h->dev, frame_len);
    if (n_frames > INT32_MAX / (8 * OFDM_FO_MAX_SYNC) || pv * h->cfg.n_fo > INT32_MAX / 2)
        return fail(OFDM_ERR_INVALID, "ofdm_fo_reserve: batch too large");
    const int64_t table = n_frames * h->cfg.n_fo * pv;
    if (n_frames <= h->cap_frames && table <= h->cap_table) return OFDM_OK;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    const int64_t frames = std::max(n_frames, h->cap_frames), tab = std::max(table, h->cap_table);
    free_dev(&h->b_tm, &h->b_td, &h->b_tsr, &h->b_fo, &h->b_gain, &h->b_edf);
    h->cap_frames = h->cap_table = 0;
    const size_t units = size_t(frames) * OFDM_FO_MAX_SYNC;
    int rc = dev_alloc(&h->b_tm, size_t(tab));
    if (rc == OFDM_OK) rc = dev_alloc(&h->b_td, size_t(tab));
    if (rc == OFDM_OK) rc = dev_alloc(&h->b_tsr, units * 4);
    if (rc == OFDM_OK) rc = dev_alloc(&h->b_fo, size_t(frames));
    if (rc == OFDM_OK) rc = dev_alloc(&h->b_gain, units * h->dev.Kd);
    if (rc == OFDM_OK && h->cfg.dsss > 0) rc = dev_alloc(&h->b_edf, units * h->dev.Kd);
    if (rc != OFDM_OK) return rc;
    h->cap_frames = frames;
    h->cap_table = tab;
    return OFDM_OK;
}

int64_t ofdm_fo_demod_frames(ofdm_fo* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             const ofdm_fo_batch_out* out, void* stream) {
    // checks that need neither the device nor the handle's contents come first
    if (!h || !out || !out->status) return fail(OFDM_ERR_INVALID, "ofdm_fo_demod_frames: null handle, output set or status");
    if (n_frames < 0 || frame_len < 0 || frame_stride < frame_len || (n_frames > 0 && !d_iq))
        return fail(OFDM_ERR_INVALID, "ofdm_fo_demod_frames: bad frame layout");
    if (out->data_freq_d && h->cfg.dsss <= 0) return fail(OFDM_ERR_INVALID, "data_freq_d needs a handle created with dsss >= 1");
    const RxDev& d = h->dev;
    const int N = d.nfft, Kd = d.Kd, n_fo = h->cfg.n_fo;
    constexpr int R = OFDM_FO_MAX_SYNC;
    if (out->bits) {
        if (out->bits_mode != OFDM_BITS_PACKED && out->bits_mode != OFDM_BITS_UNPACKED)
            return fail(OFDM_ERR_INVALID, "bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED");
        if (out->bits_mode == OFDM_BITS_PACKED && (Kd & 3)) return fail(OFDM_ERR_INVALID, "packed bits need num_data_bins %% 4 == 0");
    }
    const int64_t pv = valid_trials(d, frame_len);
    // index types of the kernels: units (frame, row) as int (x4 in the demod's tsr index), trials x candidates per frame as int
    if (n_frames > INT32_MAX / (8 * R) || pv * n_fo > INT32_MAX / 2)
        return fail(OFDM_ERR_INVALID, "ofdm_fo_demod_frames: batch too large (%lld frames, %lld trials x %d candidates)",
                    (long long)n_frames, (long long)pv, n_fo);
    if (n_frames == 0) return R;
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    if (n_frames > h->cap_frames || n_frames * n_fo * pv > h->cap_table) {
        int rc = refuse_growth_in_capture(s, "ofdm_fo_demod_frames", "ofdm_fo_reserve");
        if (rc == OFDM_OK) rc = ofdm_fo_reserve(h, n_frames, frame_len);
        if (rc != OFDM_OK) return rc;
    }
    const int64_t units = n_frames * R;
    const cf* iq = reinterpret_cast<const cf*>(d_iq);

    // 1. trial table of every frame, every candidate (FO:248-282), in parts of at most 65535 frames (one grid row per frame)
    for (int64_t f0 = 0; f0 < n_frames && pv > 0; f0 += 65535) {
        SyncArgs sa{};
        sa.iq = iq + f0 * frame_stride;
        sa.frame_stride = frame_stride;
        sa.frame_len = frame_len;
        sa.n_frames = int(std::min<int64_t>(65535, n_frames - f0));
        sa.mode = 1;
        sa.p_begin = 0;
        sa.p_count = int(pv);
        sa.trial_m = h->b_tm + f0 * n_fo * pv;
        sa.trial_d = h->b_td + f0 * n_fo * pv;
        sa.rot = h->d_rot;
        sa.n_rot = n_fo;
        HIP_TRY(launch_rx_sync(d, sa, s));
    }
    // 2. per-frame decision (FO:282-298): status, time_synch_ref, dmax_tmp_ind, the (frame, row) units
    int* fo_idx = out->fo_idx ? out->fo_idx : h->b_fo;
    FoDecideArgs da{};
    da.trial_m = h->b_tm;
    da.trial_d = h->b_td;
    da.n_frames = int(n_frames);
    da.n_rot = n_fo;
    da.p_count = int(pv);
    da.rows = R;
    da.err_index = OFDM_ERR_INDEX;
    da.status = out->status;
    da.tsr_out = out->tsr;
    da.fo_idx = fo_idx;
    da.u_tsr = h->b_tsr;
    HIP_TRY(launch_fo_decide(d, da, s));
    // 3. LS estimate per accepted sync: sync vector of the LAST candidate, lag of the best one (FO:268-274,300-329)
    SyncArgs fa{};
    fa.iq = iq;
    fa.frame_stride = frame_stride;
    fa.frame_len = frame_len;
    fa.n_frames = int(units);
    fa.tsr = h->b_tsr;
    fa.H = reinterpret_cast<cf*>(out->chan_freq);
    fa.gain = h->b_gain;
    fa.htime = reinterpret_cast<cf*>(out->chan_time);
    fa.esf = reinterpret_cast<cf*>(out->synch_freq);
    fa.rot = h->d_rot ? h->d_rot + size_t(n_fo - 1) * N : nullptr;
    fa.n_rot = 1;
    HIP_TRY(launch_fo_finalize(d, fa, R, s));
    // 4. one data symbol per sync at time_synch_ref[0] + S*L, rotated by the frame's LAST trial pick (FO:332-358)
    cf* edf = reinterpret_cast<cf*>(out->data_freq);
    if (!edf && out->data_freq_d) edf = h->b_edf;
    if (edf || out->bits) {
        DemodArgs ma{};
        ma.iq = iq;
        ma.frame_stride = frame_stride;
        ma.frame_len = frame_len;
        ma.n_frames = int(units);
        ma.tsr = h->b_tsr;
        ma.gain = h->b_gain;
        ma.eq = edf;
        ma.bits = out->bits;
        ma.bits_mode = out->bits ? out->bits_mode : 0;
        ma.mod = 2;
        ma.n_dsym = 1;
        ma.row_stride_pat = 1;
        ma.rows_per_frame = 1;
        ma.zero_skipped = 1;
        ma.rot = h->d_rot;                      // table mode: none
        ma.units_per_frame = R;
        ma.rot_idx = fo_idx;
        HIP_TRY(launch_rx_demod(d, ma, s));
    }
    if (out->data_freq_d) {                     // DS:391-399 over every row (zero rows despread to zero)
        for (int64_t r0 = 0; r0 < units; r0 += 65535) {
            const int rows = int(std::min<int64_t>(65535, units - r0));
            HIP_TRY(launch_despread(edf + r0 * Kd, Kd, h->d_code, h->cfg.dsss, h->n_spread, rows,
                                    reinterpret_cast<cf*>(out->data_freq_d) + r0 * h->n_spread, s));
        }
    }
    return R;
}

int ofdm_fo_get_despread(ofdm_fo* h, float* h_data_freq_d) {
    if (!h || !h_data_freq_d) return fail(OFDM_ERR_INVALID, "ofdm_fo_get_despread: null argument");
    if (h->cfg.dsss <= 0) return fail(OFDM_ERR_INVALID, "handle was not created with dsss >= 1");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h_data_freq_d, h->t_edfd, size_t(OFDM_FO_MAX_SYNC) * h->n_spread * sizeof(cf), hipMemcpyDeviceToHost));
    return OFDM_OK;
}

}  // extern "C"
