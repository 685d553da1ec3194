// capi_chanavg.hip -- the channel estimate averaged over every sync symbol of a frame on the receiver handle: the stage on any
// device IQ buffer, the handle's setting (ofdm_rx_demod_frames runs the stage in place between its sync launch and the delay
// window, capi_rx.hip), its workspace and the spreads of that call as noise variances (definition: include/ofdm_mi355x.h,
// "channel estimate averaged over every sync symbol of a frame").
#include "capi_internal.hpp"

static_assert(CHANAVG_CHUNK == OFDM_CHANAVG_CHUNK, "the header's chunk length is the kernel's");

namespace {
// patterns of a frame of frame_len samples
int64_t frame_patterns(const RxDev& d, int64_t frame_len) { return frame_len / d.L / (d.S + d.D); }
// what the batch arguments alone decide; "" = fine
const char* average_bad(const RxDev& d, int64_t n_frames, int64_t frame_stride, int64_t frame_len) {
    if (d.S != 1) return "the stage needs synch_S == 1";
    if (n_frames < 0 || frame_len < 0) return "negative count";
    if (n_frames > MAX_BLOCKS) return "n_frames beyond the kernel's index range";
    if (frame_stride < frame_len) return "frame_stride < frame_len";
    const int64_t chunks = chanavg_chunks(frame_patterns(d, frame_len));
    if (frame_patterns(d, frame_len) > INT32_MAX / 8 || (n_frames > 0 && chunks > MAX_BLOCKS / n_frames))
        return "batch beyond the kernel's index range";
    if (n_frames > 0 && frame_stride > MAX_ITEMS / n_frames) return "batch beyond the kernel's index range";
    return "";
}
// the workspace holds the partials of n_frames frames of `chunks` chunks, or grows -- outside a capture
int average_ensure(ofdm_rx* h, int64_t n_frames, int64_t chunks, hipStream_t s, const char* who) {
    const int64_t frames = std::max(n_frames, h->cap_avg_frames), items = std::max(n_frames * chunks, h->cap_avg_items);
    if (frames <= h->cap_avg_frames && items <= h->cap_avg_items) return OFDM_OK;
    if (s) {
        const int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve_chan_average");
        if (rc != OFDM_OK) return rc;
    }
    const size_t N = size_t(h->dev.nfft);
    return regrow(h, {{&h->cap_avg_frames, frames}, {&h->cap_avg_items, items}}, ws_buf(&h->a_part_d, size_t(items) * N),
                  ws_buf(&h->a_part_a0, size_t(frames) * N), ws_buf(&h->a_part_q, size_t(items)), ws_buf(&h->a_part_n, size_t(items)));
}
// the stage; the batch arguments have been checked
int average_run(ofdm_rx* h, const cf* iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const int32_t* d_tsr,
                int32_t n_avg, cf* H, cf* gain, float* spread, int32_t* n_used, cf* rot, hipStream_t s, const char* who) {
    const int64_t n_pat = frame_patterns(h->dev, frame_len);
    ChanAvgArgs a{};
    a.iq = iq;
    a.frame_stride = frame_stride;
    a.frame_len = frame_len;
    a.n_frames = n_frames;
    a.tsr = d_tsr;
    a.n_pat = int(n_avg < 0 ? n_pat : std::min<int64_t>(n_avg, n_pat));
    a.n_chunks = int(chanavg_chunks(a.n_pat));
    const int rc = average_ensure(h, n_frames, a.n_chunks, s, who);
    if (rc != OFDM_OK) return rc;
    a.part_d = h->a_part_d;
    a.part_a0 = h->a_part_a0;
    a.part_q = h->a_part_q;
    a.part_n = h->a_part_n;
    a.H_out = H;
    a.gain = gain;
    a.spread = spread;
    a.n_used = n_used;
    a.rot = rot;
    HIP_TRY(launch_chan_average(h->dev, a, s));
    return OFDM_OK;
}
}  // namespace

int chan_average_in_place(ofdm_rx* h, const cf* iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len, hipStream_t s) {
    const char* bad = average_bad(h->dev, n_frames, frame_stride, frame_len);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames: channel-estimate averaging: %s", bad);
    const int rc = average_run(h, iq, n_frames, frame_stride, frame_len, h->f_tsr, h->avg_n, h->f_H, h->f_gain, h->f_spread, nullptr,
                               nullptr, s, "ofdm_rx_demod_frames");
    if (rc == OFDM_OK) h->spread_frames = n_frames;
    return rc;
}

extern "C" {

int ofdm_chan_average_frames(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                             const int32_t* d_tsr, int32_t n_avg, float* d_H_out, float* d_gain_out, float* d_spread,
                             int32_t* d_n_used, float* d_rot, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_chan_average_frames: null handle");
    if (n_avg == 0 || n_avg < -1) return fail(OFDM_ERR_INVALID, "ofdm_chan_average_frames: n_avg must be >= 1, or -1 for all patterns");
    const char* bad = average_bad(h->dev, n_frames, frame_stride, frame_len);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_chan_average_frames: %s", bad);
    if (n_frames == 0) return OFDM_OK;
    if (!d_iq || !d_tsr) return fail(OFDM_ERR_INVALID, "ofdm_chan_average_frames: null d_iq or d_tsr");
    if (!d_H_out && !d_gain_out && !d_spread && !d_n_used && !d_rot)
        return fail(OFDM_ERR_INVALID, "ofdm_chan_average_frames: no output wanted");
    HIP_TRY(hipSetDevice(h->cfg.device));
    return average_run(h, reinterpret_cast<const cf*>(d_iq), n_frames, frame_stride, frame_len, d_tsr, n_avg,
                       reinterpret_cast<cf*>(d_H_out), reinterpret_cast<cf*>(d_gain_out), d_spread, d_n_used,
                       reinterpret_cast<cf*>(d_rot), pick_stream(h, stream), "ofdm_chan_average_frames");
}

int ofdm_rx_set_chan_average(ofdm_rx* h, int32_t n_avg) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_chan_average: null handle");
    if (n_avg < -1) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_chan_average: n_avg must be 0 (off), >= 1, or -1 for all patterns");
    if (n_avg == 0) {
        h->avg_n = 0;
        return OFDM_OK;
    }
    if (h->dev.S != 1) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_chan_average: the stage needs synch_S == 1");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(chan_average_prepare());     // a first ofdm_rx_demod_frames inside a capture has nothing left to load
    h->avg_n = n_avg;
    return OFDM_OK;
}

int ofdm_rx_reserve_chan_average(ofdm_rx* h, int64_t n_frames, int64_t frame_len) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_chan_average: null handle");
    const char* bad = average_bad(h->dev, n_frames, frame_len, frame_len);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_chan_average: %s", bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(chan_average_prepare());
    return average_ensure(h, n_frames, chanavg_chunks(frame_patterns(h->dev, frame_len)), nullptr, "ofdm_rx_reserve_chan_average");
}

int ofdm_rx_chan_spread_frames(ofdm_rx* h, int64_t n_frames, double* d_sigma2, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_spread_frames: null handle");
    if (n_frames < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_spread_frames: negative count");
    if (h->spread_frames < 0)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_spread_frames: the last ofdm_rx_demod_frames call ran without averaging "
                                      "(ofdm_rx_set_chan_average)");
    if (n_frames > h->spread_frames)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_spread_frames: %lld frames asked, the last ofdm_rx_demod_frames call had %lld",
                    static_cast<long long>(n_frames), static_cast<long long>(h->spread_frames));
    if (n_frames == 0) return OFDM_OK;
    if (!d_sigma2) return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_spread_frames: null d_sigma2");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_chan_spread(h->f_spread, n_frames, d_sigma2, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
