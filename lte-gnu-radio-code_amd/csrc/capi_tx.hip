// capi_tx.hip -- the transmitter handle: create / destroy, the decomposed stages, ofdm_tx_modulate_frames and
// ofdm_channel_apply.  Its codec calls live with their codecs (capi_tbcc.hip, capi_bitproc.hip, capi_turbo.hip, capi_tb.hip).
#include "capi_internal.hpp"

extern "C" {

int ofdm_tx_destroy(ofdm_tx* h) {
    if (!h) return OFDM_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_dev(&h->d_tw, &h->d_zc, &h->d_sync_time, &h->d_pilots, &h->tb_ws, &h->sp_sym, &h->sp_grid, &h->sp_time);
    dft_plans_free(h->dft);
    dft_alloc_free(h->alloc);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return OFDM_OK;
}

int ofdm_tx_create(const ofdm_tx_cfg* c, ofdm_tx** out) {
    if (!c || !out) return fail(OFDM_ERR_INVALID, "ofdm_tx_create: null argument");
    *out = nullptr;
    if (int bad = check_nfft(c->nfft)) return bad;
    if (c->cp_len < 0 || c->cp_len >= c->nfft) return fail(OFDM_ERR_INVALID, "cp_len=%d out of range", c->cp_len);
    if (c->num_synch_bins < 2 || c->num_synch_bins > c->nfft || (c->num_synch_bins & 1) || c->num_data_bins < 2 ||
        c->num_data_bins > c->nfft || (c->num_data_bins & 1))
        return fail(OFDM_ERR_INVALID, "bin counts must be even and in [2, nfft]");
    if (c->synch_S < 1 || c->synch_D < 1) return fail(OFDM_ERR_INVALID, "synch_dat must be [>=1, >=1]");
    if (c->modulation != 1 && c->modulation != 2 && c->modulation != 4 && c->modulation != 6)
        return fail(OFDM_ERR_INVALID, "modulation must be 1, 2, 4 or 6 bits per symbol");
    HIP_TRY(hipSetDevice(c->device));
    ofdm_tx* h = new (std::nothrow) ofdm_tx();
    if (!h) return fail(OFDM_ERR_NOMEM, "out of host memory");
    h->cfg = *c;
    const int N = c->nfft, MM = c->synch_S * c->num_synch_bins;
    int rc = OFDM_OK;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(OFDM_ERR_HIP, "hipStreamCreate failed");
    if (rc == OFDM_OK) rc = upload(&h->d_tw, make_twiddles(N), "device table initialisation failed");
    if (rc == OFDM_OK) rc = upload(&h->d_zc, make_zc(MM, c->zc_root ? c->zc_root : 23, MM), "device table initialisation failed");
    if (rc != OFDM_OK) return create_failed(h, rc, ofdm_tx_destroy);
    TxDev& d = h->dev;
    d.nfft = N;
    d.cp = c->cp_len;
    d.L = N + c->cp_len;
    d.Ks = c->num_synch_bins;
    d.Kd = c->num_data_bins;
    d.S = c->synch_S;
    d.D = c->synch_D;
    d.bps = c->modulation;
    d.tw = h->d_tw;
    d.zc = h->d_zc;
    // the sync symbol(s) of SynchDataMux: ZC grid rows -> IFFT + CP + normalise, once (same kernels as the data symbols)
    {
        cf* d_grid = nullptr;
        rc = dev_alloc(&d_grid, size_t(d.S) * N);
        if (rc == OFDM_OK) rc = dev_alloc(&h->d_sync_time, size_t(d.S) * d.L);
        if (rc == OFDM_OK) {
            TimeArgs ta{};
            ta.in = d_grid;
            ta.n_rows = d.S;
            ta.do_ifft = 1;
            ta.do_cp = 1;
            ta.out = h->d_sync_time;
            if (launch_tx_sync_grid(d, d_grid, h->stream) != hipSuccess || launch_tx_time(d, ta, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess)
                rc = fail(OFDM_ERR_HIP, "sync-symbol synthesis failed: %s", hipGetErrorString(hipGetLastError()));
        }
        free_dev(&d_grid);
        if (rc != OFDM_OK) return create_failed(h, rc, ofdm_tx_destroy);
    }
    *out = h;
    return OFDM_OK;
}

// ---- decomposed stages
int ofdm_tx_random_bits(ofdm_tx* h, uint64_t seed, uint64_t offset, uint8_t* d_bits, int64_t n_bits, void* stream) {
    if (!h || (!d_bits && n_bits > 0) || n_bits < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_random_bits: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tx_random_bits(seed, offset, d_bits, n_bits, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tx_map(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_symbols, float* d_sym, void* stream) {
    if (!h || n_symbols < 0 || (n_symbols > 0 && (!d_bits || !d_sym))) return fail(OFDM_ERR_INVALID, "ofdm_tx_map: bad argument");
    if (bits_mode != OFDM_BITS_PACKED && bits_mode != OFDM_BITS_UNPACKED)
        return fail(OFDM_ERR_INVALID, "bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tx_map(d_bits, bits_mode, h->dev.bps, n_symbols, reinterpret_cast<cf*>(d_sym),
                          pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tx_set_pilots(ofdm_tx* h, const int32_t* h_locations, int32_t n_pilots, float pilot_re, float pilot_im) {
    if (!h || n_pilots < 0 || (n_pilots > 0 && !h_locations)) return fail(OFDM_ERR_INVALID, "ofdm_tx_set_pilots: bad argument");
    const int K = h->dev.Kd + n_pilots;
    if ((K & 1) || K > h->dev.nfft)
        return fail(OFDM_ERR_INVALID, "num_data_bins + pilots = %d must be even and <= nfft", K);
    std::vector<int> idx(size_t(n_pilots), 0);
    for (int p = 0; p < n_pilots; ++p) {
        const int loc = h_locations[p];
        if (loc == 0 || loc < -(K / 2) || loc > K / 2)
            return fail(OFDM_ERR_INVALID, "pilot location %d outside the occupied bins [-%d..-1, 1..%d]", loc, K / 2, K / 2);
        idx[size_t(p)] = loc < 0 ? loc + K / 2 : K / 2 + loc - 1;
    }
    std::sort(idx.begin(), idx.end());
    for (int p = 1; p < n_pilots; ++p)
        if (idx[size_t(p)] == idx[size_t(p - 1)]) return fail(OFDM_ERR_INVALID, "pilot locations must be distinct");
    const int drained = drain(h);
    if (drained != OFDM_OK) return drained;
    free_dev(&h->d_pilots);
    h->n_pilots = 0;
    const int rc = upload(&h->d_pilots, idx);
    if (rc != OFDM_OK) return rc;
    h->n_pilots = n_pilots;
    h->pilot_value = cf{pilot_re, pilot_im};
    return OFDM_OK;
}

int ofdm_tx_grid(ofdm_tx* h, const float* d_sym, int64_t n_rows, float* d_grid, void* stream) {
    if (!h || n_rows < 0 || (n_rows > 0 && (!d_sym || !d_grid))) return fail(OFDM_ERR_INVALID, "ofdm_tx_grid: bad argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    GridArgs a{};
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_rows = n_rows;
    a.pilots = h->d_pilots;
    a.n_pilots = h->n_pilots;
    a.pilot_value = h->pilot_value;
    a.grid = reinterpret_cast<cf*>(d_grid);
    HIP_TRY(launch_tx_grid(h->dev, a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tx_ifft_cp(ofdm_tx* h, const float* d_in, int64_t n_rows, int32_t do_ifft, int32_t add_cp, float* d_out, void* stream) {
    if (!h || n_rows < 0 || (n_rows > 0 && (!d_in || !d_out))) return fail(OFDM_ERR_INVALID, "ofdm_tx_ifft_cp: bad argument");
    if (!do_ifft && !add_cp) return fail(OFDM_ERR_INVALID, "ofdm_tx_ifft_cp: nothing to do (do_ifft = add_cp = 0)");
    if (n_rows > INT32_MAX) return fail(OFDM_ERR_INVALID, "batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    TimeArgs a{};
    a.in = reinterpret_cast<const cf*>(d_in);
    a.n_rows = n_rows;
    a.do_ifft = do_ifft != 0;
    a.do_cp = add_cp != 0;
    a.out = reinterpret_cast<cf*>(d_out);
    HIP_TRY(launch_tx_time(h->dev, a, pick_stream(h, stream)));
    return OFDM_OK;
}

int64_t ofdm_tx_mux(ofdm_tx* h, const float* d_data, int64_t n_data_sym, float* d_out, void* stream) {
    if (!h || n_data_sym < 0 || (n_data_sym > 0 && (!d_data || !d_out))) return fail(OFDM_ERR_INVALID, "ofdm_tx_mux: bad argument");
    const TxDev& d = h->dev;
    const int64_t full = n_data_sym / d.D, rem = n_data_sym % d.D;
    const int64_t n_out = full * (d.S + d.D) + (rem ? d.S + rem : 0);
    if (n_out == 0) return 0;
    HIP_TRY(hipSetDevice(h->cfg.device));
    MuxArgs a{};
    a.sync_time = h->d_sync_time;
    a.data = reinterpret_cast<const cf*>(d_data);
    a.n_out_sym = n_out;
    a.out = reinterpret_cast<cf*>(d_out);
    HIP_TRY(launch_tx_mux(d, a, pick_stream(h, stream)));
    return n_out;
}

int ofdm_tx_get_sync_symbol(ofdm_tx* h, float* h_sync_time) {
    if (!h || !h_sync_time) return fail(OFDM_ERR_INVALID, "ofdm_tx_get_sync_symbol: null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipMemcpy(h_sync_time, h->d_sync_time, size_t(h->dev.S) * h->dev.L * sizeof(cf), hipMemcpyDeviceToHost));
    return OFDM_OK;
}

int ofdm_tx_modulate_frames(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                            float* d_iq, int64_t frame_stride, void* stream) {
    if (!h || !d_iq || n_frames < 0 || n_sym < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_modulate_frames: bad argument");
    if (bits_mode != OFDM_BITS_PACKED && bits_mode != OFDM_BITS_UNPACKED)
        return fail(OFDM_ERR_INVALID, "bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED");
    const TxDev& d = h->dev;
    if (frame_stride < int64_t(n_sym) * d.L) return fail(OFDM_ERR_INVALID, "frame_stride shorter than n_sym*(nfft+cp)");
    if (n_frames * int64_t(n_sym) > INT32_MAX) return fail(OFDM_ERR_INVALID, "batch too large");
    const int SD = d.S + d.D;
    int64_t n_data = int64_t(n_sym / SD) * d.D;
    const int rem = n_sym % SD;
    if (rem > d.S) n_data += rem - d.S;
    const int64_t bits_per_frame = n_data * d.Kd * d.bps;
    if (bits_mode == OFDM_BITS_PACKED && (bits_per_frame & 7))
        return fail(OFDM_ERR_INVALID, "packed bits need a whole number of bytes per frame");
    if (bits_per_frame > INT32_MAX) return fail(OFDM_ERR_INVALID, "more than 2^31 bits per frame");
    HIP_TRY(hipSetDevice(h->cfg.device));
    ModArgs a{};
    a.bits = d_bits;
    a.bits_mode = bits_mode;
    a.bits_stride = bits_mode == OFDM_BITS_PACKED ? bits_per_frame / 8 : bits_per_frame;
    a.n_frames = int(n_frames);
    a.n_sym = n_sym;
    a.iq = reinterpret_cast<cf*>(d_iq);
    a.frame_stride = frame_stride;
    a.sync_time = h->d_sync_time;
    HIP_TRY(launch_tx_modulate(d, a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_channel_apply(ofdm_tx* h, const float* d_in, int64_t n_frames, int64_t in_stride, int64_t in_len,
                       const float* d_taps, int32_t n_taps, int32_t per_frame_taps, float noise_var, uint64_t seed,
                       float* d_out, int64_t out_stride, int64_t out_len, void* stream) {
    if (!h || !d_in || !d_out || !d_taps || n_taps < 1 || n_frames < 0 || in_len < 0 || out_len < 0 || noise_var < 0.f)
        return fail(OFDM_ERR_INVALID, "ofdm_channel_apply: bad argument");
    if (out_len > in_len + n_taps - 1) return fail(OFDM_ERR_INVALID, "out_len exceeds the convolution length");
    if (in_stride < in_len || out_stride < out_len) return fail(OFDM_ERR_INVALID, "stride shorter than length");
    if (n_frames > 65535) return fail(OFDM_ERR_INVALID, "at most 65535 frames per call");
    HIP_TRY(hipSetDevice(h->cfg.device));
    ChanArgs a{};
    a.in = reinterpret_cast<const cf*>(d_in);
    a.in_stride = in_stride;
    a.in_len = in_len;
    a.n_frames = int(n_frames);
    a.taps = reinterpret_cast<const cf*>(d_taps);
    a.n_taps = n_taps;
    a.per_frame_taps = per_frame_taps;
    a.noise_std = std::sqrt(noise_var / 2.f);
    a.seed = seed;
    a.out = reinterpret_cast<cf*>(d_out);
    a.out_stride = out_stride;
    a.out_len = out_len;
    HIP_TRY(launch_channel(a, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
