// capi_chanwin.hip -- delay-window denoising of the LS channel estimate on the receiver handle: the stage on any device buffer,
// the handle's window setting (ofdm_rx_demod_frames runs the stage in place between its sync and demod launches, capi_rx.hip)
// and the tail powers of that call as noise variances (definition: include/ofdm_mi355x.h, "delay-window channel-estimate
// denoising").
#include "capi_internal.hpp"

namespace {
// what the arguments alone decide; "" = fine
const char* window_bad(int nfft, int32_t pre, int32_t post) {
    if (pre < 0) return "pre must be >= 0";
    if (post < 1) return "post must be >= 1";
    if (int64_t(pre) + int64_t(post) > nfft) return "pre + post must not exceed nfft";
    return "";
}
}  // namespace

extern "C" {

int ofdm_chan_window_frames(ofdm_rx* h, const float* d_H_in, const int32_t* d_tsr, int64_t n_rows, int32_t pre, int32_t post,
                            float* d_H_out, float* d_gain_out, float* d_tail, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_chan_window_frames: null handle");
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_chan_window_frames: negative count");
    if (n_rows > MAX_BLOCKS) return fail(OFDM_ERR_INVALID, "ofdm_chan_window_frames: n_rows beyond the kernel's index range");
    const char* bad = window_bad(h->dev.nfft, pre, post);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_chan_window_frames: %s", bad);
    if (n_rows == 0) return OFDM_OK;
    if (!d_H_in || !d_tsr || !d_H_out) return fail(OFDM_ERR_INVALID, "ofdm_chan_window_frames: null d_H_in, d_tsr or d_H_out");
    HIP_TRY(hipSetDevice(h->cfg.device));
    ChanWinArgs a{};
    a.H_in = reinterpret_cast<const cf*>(d_H_in);
    a.tsr = d_tsr;
    a.n_rows = n_rows;
    a.pre = pre;
    a.post = post;
    a.H_out = reinterpret_cast<cf*>(d_H_out);
    a.gain = reinterpret_cast<cf*>(d_gain_out);
    a.tail = d_tail;
    HIP_TRY(launch_chan_window(h->dev, a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_rx_set_chan_window(ofdm_rx* h, int32_t pre, int32_t post) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_chan_window: null handle");
    if (pre == 0 && post == 0) {
        h->win_pre = h->win_post = 0;
        return OFDM_OK;
    }
    const char* bad = window_bad(h->dev.nfft, pre, post);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_chan_window: %s", bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(chan_window_prepare());      // a first ofdm_rx_demod_frames inside a capture has nothing left to load
    h->win_pre = pre;
    h->win_post = post;
    return OFDM_OK;
}

int ofdm_rx_chan_noise_frames(ofdm_rx* h, int64_t n_frames, double* d_sigma2, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_noise_frames: null handle");
    if (n_frames < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_noise_frames: negative count");
    if (h->tail_frames < 0)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_noise_frames: the last ofdm_rx_demod_frames call ran without a window "
                                      "(ofdm_rx_set_chan_window)");
    if (n_frames > h->tail_frames)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_noise_frames: %lld frames asked, the last ofdm_rx_demod_frames call had %lld",
                    static_cast<long long>(n_frames), static_cast<long long>(h->tail_frames));
    if (n_frames == 0) return OFDM_OK;
    if (!d_sigma2) return fail(OFDM_ERR_INVALID, "ofdm_rx_chan_noise_frames: null d_sigma2");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_chan_noise(h->f_tail, n_frames, d_sigma2, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
