// capi_chantrack.hip -- the channel tracked across the sync symbols of a frame on the receiver handle: the stage on any device IQ
// buffer, the call that runs the handle's sync search in front of it, and the workspace (definition: include/ofdm_mi355x.h,
// "channel tracked across the sync symbols of a frame").
#include "capi_internal.hpp"

namespace {
int64_t frame_patterns(const RxDev& d, int64_t frame_len) { return frame_len / d.L / (d.S + d.D); }
// what the arguments alone decide; "" = fine.  (pre, post) == (0, 0) is the window switched off.
const char* track_bad(const RxDev& d, int64_t n_frames, int64_t frame_stride, int64_t frame_len, int32_t mode, int32_t pre,
                      int32_t post, int32_t bits_mode, const ofdm_track_out* out) {
    if (d.S != 1) return "the stage needs synch_S == 1";
    if (mode != OFDM_TRACK_HOLD && mode != OFDM_TRACK_LINEAR) return "mode must be OFDM_TRACK_HOLD or OFDM_TRACK_LINEAR";
    if (pre != 0 || post != 0) {
        if (pre < 0) return "window: pre must be >= 0";
        if (post < 1) return "window: post must be >= 1";
        if (int64_t(pre) + int64_t(post) > d.nfft) return "window: pre + post must not exceed nfft";
    }
    if (bits_mode != OFDM_BITS_NONE && !bits_mode_ok(bits_mode))
        return "bits_mode must be OFDM_BITS_NONE, OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    if (out && out->bits) {
        if (bits_mode == OFDM_BITS_NONE) return "bits wanted with OFDM_BITS_NONE";
        if (bits_mode == OFDM_BITS_PACKED && ((d.Kd & 3) || (d.bps & 1)))
            return "packed bits need num_data_bins % 4 == 0 and an even number of bits per symbol";
    }
    if (n_frames < 0 || frame_len < 0) return "negative count";
    if (frame_stride < frame_len) return "frame_stride < frame_len";
    const int64_t n_pat = frame_patterns(d, frame_len);
    // one workgroup slot per (frame, pattern) and per (frame, run); rows and symbols are 64-bit in the kernels
    if (n_frames > MAX_BLOCKS || n_pat * d.D > INT32_MAX / 8 || (n_frames > 0 && n_pat * d.D > MAX_BLOCKS / n_frames))
        return "batch beyond the kernels' index range";
    if (n_frames > 0 && frame_stride > MAX_ITEMS / n_frames) return "batch beyond the kernels' index range";
    // the hard-decision pass: one lane per four symbols, 256 lanes per workgroup
    if (n_frames > 0 && n_pat * d.D * d.Kd / 1024 + 1 > MAX_BLOCKS / n_frames) return "batch beyond the kernels' index range";
    return "";
}
// the workspace holds n_frames * n_pat flags, neighbours and row tsr, and (need_H: the caller does not take H_pat) as many rows
// a_p, or grows -- outside a capture
int track_ensure(ofdm_rx* h, int64_t rows, bool need_H, hipStream_t s, const char* who) {
    const bool grow_rows = rows > h->cap_trk_rows, grow_H = need_H && rows > h->cap_trk_H;
    if (!grow_rows && !grow_H) return OFDM_OK;
    if (s) {
        const int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve_chan_track");
        if (rc != OFDM_OK) return rc;
    }
    int rc = OFDM_OK;
    if (grow_rows)
        rc = regrow(h, {{&h->cap_trk_rows, rows}}, ws_buf(&h->k_flag, size_t(rows)), ws_buf(&h->k_nb, size_t(rows)),
                    ws_buf(&h->k_rtsr, size_t(rows) * 4));
    if (rc == OFDM_OK && grow_H) rc = regrow(h, {{&h->cap_trk_H, rows}}, ws_buf(&h->k_H, size_t(rows) * h->dev.nfft));
    return rc;
}
// the rows of a call that wants bits without eq
int track_ensure_eq(ofdm_rx* h, int64_t n_sym, hipStream_t s, const char* who) {
    if (n_sym <= h->cap_trk_eq) return OFDM_OK;
    if (stream_is_capturing(s))
        return fail(OFDM_ERR_INVALID, "%s: bits without eq need a workspace for the equalised rows, which cannot grow inside a capture "
                                      "(pass eq, or make the call once outside the capture)", who);
    return regrow(h, {{&h->cap_trk_eq, n_sym}}, ws_buf(&h->k_eq, size_t(n_sym)));
}
// every workspace the call needs, before anything is enqueued
int track_prepare(ofdm_rx* h, int64_t n_frames, int64_t frame_len, const ofdm_track_out* out, hipStream_t s, const char* who) {
    const RxDev& d = h->dev;
    const int64_t n_pat = frame_patterns(d, frame_len);
    if (n_pat == 0) return OFDM_OK;
    const int rc = track_ensure(h, n_frames * n_pat, !out->H_pat, s, who);
    if (rc != OFDM_OK || !out->bits || out->eq) return rc;
    return track_ensure_eq(h, n_frames * n_pat * d.D * d.Kd, s, who);
}
// the stage; the arguments have been checked, n_frames > 0 and track_prepare has run
int64_t track_run(ofdm_rx* h, const cf* iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t* d_tsr,
                  int32_t mode, int32_t pre, int32_t post, int32_t bits_mode, const ofdm_track_out* out, hipStream_t s) {
    const RxDev& d = h->dev;
    const int64_t n_pat = frame_patterns(d, frame_len), n_dsym = n_pat * d.D;
    if (n_pat == 0) return 0;
    const bool ws_eq = out->bits && !out->eq;
    ChanTrackArgs a{};
    a.iq = iq;
    a.frame_stride = frame_stride;
    a.frame_len = frame_len;
    a.n_frames = n_frames;
    a.tsr = d_tsr;
    a.n_pat = int(n_pat);
    a.n_dsym = int(n_dsym);
    a.n_runs = int(chantrack_runs(n_dsym));
    a.linear = mode == OFDM_TRACK_LINEAR;
    a.H_pat = out->H_pat ? reinterpret_cast<cf*>(out->H_pat) : h->k_H;
    a.flag = h->k_flag;
    a.nb = h->k_nb;
    a.row_tsr = post > 0 ? h->k_rtsr : nullptr;
    a.takes = out->takes;
    a.eq = ws_eq ? h->k_eq : reinterpret_cast<cf*>(out->eq);
    a.csi = out->csi;
    a.bits = out->bits;
    a.bits_mode = bits_mode;
    a.mod = d.bps;
    HIP_TRY(launch_chan_track_est(d, a, s));
    if (post > 0) {                      // the delay window over the frames * n_pat rows, in place: a row that does not take part stays +0
        ChanWinArgs wa{};
        wa.H_in = a.H_pat;
        wa.tsr = a.row_tsr;
        wa.n_rows = n_frames * n_pat;
        wa.pre = pre;
        wa.post = post;
        wa.H_out = a.H_pat;
        HIP_TRY(launch_chan_window(d, wa, s));
    }
    HIP_TRY(launch_chan_track_demod(d, a, s));
    return n_dsym;
}
bool no_output(const ofdm_track_out* out) { return !out || !(out->eq || out->bits || out->csi || out->H_pat || out->takes); }
}  // namespace

extern "C" {

int64_t ofdm_chan_track_frames(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                               const int32_t* d_tsr, int32_t mode, int32_t pre, int32_t post, int32_t bits_mode,
                               const ofdm_track_out* out, void* stream) {
    constexpr const char* who = "ofdm_chan_track_frames";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const char* bad = track_bad(h->dev, n_frames, frame_stride, frame_len, mode, pre, post, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    const int64_t n_dsym = frame_patterns(h->dev, frame_len) * h->dev.D;
    if (n_frames == 0) return n_dsym;
    if (!d_iq || !d_tsr) return fail(OFDM_ERR_INVALID, "%s: null d_iq or d_tsr", who);
    if (no_output(out)) return fail(OFDM_ERR_INVALID, "%s: no output wanted", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    if (const int rc = track_prepare(h, n_frames, frame_len, out, s, who)) return rc;
    return track_run(h, reinterpret_cast<const cf*>(d_iq), n_frames, frame_stride, frame_len, d_tsr, mode, pre, post, bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_track(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                   int32_t mode, int32_t bits_mode, int32_t* d_tsr, const ofdm_track_out* out, void* stream) {
    constexpr const char* who = "ofdm_rx_demod_frames_track";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const char* bad = track_bad(h->dev, n_frames, frame_stride, frame_len, mode, h->win_pre, h->win_post, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_frames > INT32_MAX / 8) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    const int64_t n_dsym = frame_patterns(h->dev, frame_len) * h->dev.D;
    if (n_frames == 0) return n_dsym;
    if (!d_iq) return fail(OFDM_ERR_INVALID, "%s: null d_iq", who);
    if (no_output(out)) return fail(OFDM_ERR_INVALID, "%s: no output wanted", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    if (n_frames > h->cap_frames) {
        const int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve");
        if (rc != OFDM_OK) return rc;
        const int rr = ofdm_rx_reserve(h, n_frames);
        if (rr != OFDM_OK) return rr;
    }
    if (const int rc = track_prepare(h, n_frames, frame_len, out, s, who)) return rc;
    const cf* iq = reinterpret_cast<const cf*>(d_iq);
    if (const int rc = rx_sync_leg(h, iq, n_frames, frame_stride, frame_len, s)) return rc;
    if (d_tsr) HIP_TRY(hipMemcpyAsync(d_tsr, h->f_tsr, size_t(n_frames) * 4 * sizeof(int), hipMemcpyDeviceToDevice, s));
    return track_run(h, iq, n_frames, frame_stride, frame_len, h->f_tsr, mode, h->win_pre, h->win_post, bits_mode, out, s);
}

int ofdm_rx_reserve_chan_track(ofdm_rx* h, int64_t n_frames, int64_t frame_len) {
    constexpr const char* who = "ofdm_rx_reserve_chan_track";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const char* bad = track_bad(h->dev, n_frames, frame_len, frame_len, OFDM_TRACK_LINEAR, 0, 0, OFDM_BITS_NONE, nullptr);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(chan_track_prepare());
    HIP_TRY(chan_window_prepare());
    return track_ensure(h, n_frames * frame_patterns(h->dev, frame_len), true, nullptr, who);
}

}  // extern "C"
