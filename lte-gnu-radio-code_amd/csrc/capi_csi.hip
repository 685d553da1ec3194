// capi_csi.hip -- channel-state-weighted LLRs behind the batch receiver on its handle: the workspace, the |H|^2 rows of the last
// ofdm_rx_demod_frames call, the stage on any device buffer, and the call that chains the three (definition:
// include/ofdm_mi355x.h, "channel-state-weighted LLRs").
#include "capi_internal.hpp"

namespace {
bool csi_wanted(const ofdm_csi_out* o) { return o && (o->llr || o->sigma2 || o->n_used); }
// what the arguments alone decide (no read of the handle, no device access); "" = fine
const char* csi_bad_args(int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride, int64_t csi_stride, float rho,
                         int32_t modulation, int32_t noise_mode, double noise_var) {
    if (n_seg < 0 || rows < 0 || row_len < 0) return "negative count";
    if (row_len > SOFT_MAX_ROW || (row_len > 0 && rows > SOFT_MAX_LEN / row_len)) return "index range exceeded (rows * row_len)";
    if (seg_stride < rows * row_len) return "seg_stride < rows * row_len";
    if (csi_stride < row_len) return "csi_stride < row_len";
    if (!soft_mod_ok(modulation)) return "modulation must be 2, 4 or 6 bits per symbol (no BPSK soft metrics)";
    if (noise_mode != OFDM_CSI_NOISE_EST && noise_mode != OFDM_CSI_NOISE_GIVEN)
        return "noise_mode must be OFDM_CSI_NOISE_EST or OFDM_CSI_NOISE_GIVEN";
    if (noise_mode == OFDM_CSI_NOISE_GIVEN && !(std::isfinite(noise_var) && noise_var > 0.0))
        return "OFDM_CSI_NOISE_GIVEN needs a finite noise_var > 0";
    if (!(std::isfinite(rho) && rho >= 0.f)) return "rho must be finite and >= 0";
    if (n_seg > SOFT_MAX_N || (n_seg > 0 && (seg_stride > SOFT_MAX_LEN / n_seg || csi_stride > SOFT_MAX_LEN / n_seg)))
        return "index range exceeded (batch beyond the kernels' index range)";
    return "";
}
const char* csi_bad_reserve(int64_t n_seg, int64_t rows, int64_t row_len) {
    if (n_seg < 0 || rows < 0 || row_len < 0) return "negative count";
    if (n_seg > SOFT_MAX_N || row_len > SOFT_MAX_ROW || (row_len > 0 && rows > SOFT_MAX_LEN / row_len) ||
        (n_seg > 0 && row_len > SOFT_MAX_LEN / n_seg))
        return "batch too large";
    return "";
}
// grows the workspace; refuses inside a stream capture (growing synchronises and allocates)
int csi_ensure(ofdm_rx* h, int64_t n_seg, int64_t rows, int64_t row_len, hipStream_t s, const char* who) {
    return grow_outside_capture(n_seg * seg_slices(rows * row_len) <= h->cap_csi_items && n_seg * row_len <= h->cap_csi_tab, s, who,
                                "ofdm_rx_reserve_csi", [&] { return ofdm_rx_reserve_csi(h, n_seg, rows, row_len); });
}
int csi_launch(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride, const float* d_csi,
               int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode, double noise_var, const ofdm_csi_out* out,
               hipStream_t s) {
    CsiArgs a{};
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_seg = n_seg;
    a.rows = rows;
    a.seg_stride = seg_stride;
    a.row_len = int(row_len);
    a.seg_len = rows * row_len;
    a.n_slices = seg_slices(a.seg_len);
    a.csi = d_csi;
    a.csi_stride = csi_stride;
    a.rho = rho;
    a.mod = modulation;
    a.est = noise_mode == OFDM_CSI_NOISE_EST;
    a.noise_var = a.est ? 0.0 : noise_var;
    a.llr = out->llr;
    a.sigma2 = out->sigma2;
    a.n_used = reinterpret_cast<long long*>(out->n_used);
    a.tab = h->c_tab;
    a.part_e = h->c_part_e;
    a.part_n = h->c_part_n;
    HIP_TRY(launch_demap_csi(a, s));
    return OFDM_OK;
}
int csi_frames_launch(ofdm_rx* h, int64_t n_frames, int32_t layout, float* d_csi, int64_t csi_stride, hipStream_t s) {
    const RxDev& d = h->dev;
    const bool data = layout == OFDM_CSI_ROWS_DATA;
    HIP_TRY(launch_csi_frames(h->f_H, d.nfft, d.Kd, data ? h->p_src : nullptr, data ? d.Kd - h->n_pilots : d.Kd, n_frames, d_csi,
                              csi_stride, s));
    return OFDM_OK;
}
}  // namespace

extern "C" {

int ofdm_rx_reserve_csi(ofdm_rx* h, int64_t n_seg, int64_t rows, int64_t row_len) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_csi: null handle");
    const char* bad = csi_bad_reserve(n_seg, rows, row_len);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_csi: %s", bad);
    const int64_t items = std::max(n_seg * seg_slices(rows * row_len), h->cap_csi_items);
    const int64_t tab = std::max(n_seg * row_len, h->cap_csi_tab);
    if (items <= h->cap_csi_items && tab <= h->cap_csi_tab) return OFDM_OK;
    return regrow(h, {{&h->cap_csi_items, items}, {&h->cap_csi_tab, tab}}, ws_buf(&h->c_part_e, size_t(items)),
                  ws_buf(&h->c_part_n, size_t(items)), ws_buf(&h->c_tab, size_t(tab)), ws_buf(&h->c_a, size_t(tab)));
}

int ofdm_rx_csi_frames(ofdm_rx* h, int64_t n_frames, int32_t layout, float* d_csi, int64_t csi_stride, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: null handle");
    if (n_frames < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: negative count");
    if (layout != OFDM_CSI_ROWS_ALL && layout != OFDM_CSI_ROWS_DATA)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: layout must be OFDM_CSI_ROWS_ALL or OFDM_CSI_ROWS_DATA");
    if (layout == OFDM_CSI_ROWS_DATA && h->n_pilots == 0)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: OFDM_CSI_ROWS_DATA without pilots set (ofdm_rx_set_pilots)");
    const int64_t n_out = layout == OFDM_CSI_ROWS_DATA ? h->dev.Kd - h->n_pilots : h->dev.Kd;
    if (csi_stride < n_out) return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: csi_stride < entries per row");
    if (n_frames > h->last_frames)
        return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: %lld frames asked, the last ofdm_rx_demod_frames call had %lld",
                    static_cast<long long>(n_frames), static_cast<long long>(h->last_frames));
    if (n_frames > SOFT_MAX_N || (n_frames > 0 && csi_stride > SOFT_MAX_LEN / n_frames))
        return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: index range exceeded");
    if (n_frames == 0 || n_out == 0) return OFDM_OK;
    if (!d_csi) return fail(OFDM_ERR_INVALID, "ofdm_rx_csi_frames: null d_csi");
    HIP_TRY(hipSetDevice(h->cfg.device));
    return csi_frames_launch(h, n_frames, layout, d_csi, csi_stride, pick_stream(h, stream));
}

int ofdm_demap_csi_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride,
                          const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode, double noise_var,
                          const ofdm_csi_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_demap_csi_frames: null handle");
    const char* bad = csi_bad_args(n_seg, rows, row_len, seg_stride, csi_stride, rho, modulation, noise_mode, noise_var);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_demap_csi_frames: %s", bad);
    if (n_seg == 0 || rows == 0 || row_len == 0 || !csi_wanted(out)) return OFDM_OK;
    if (!d_sym || !d_csi) return fail(OFDM_ERR_INVALID, "ofdm_demap_csi_frames: null d_sym or d_csi");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = csi_ensure(h, n_seg, rows, row_len, s, "ofdm_demap_csi_frames");
    if (rc != OFDM_OK) return rc;
    return csi_launch(h, d_sym, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, modulation, noise_mode, noise_var, out, s);
}

int64_t ofdm_rx_demod_frames_csi(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                 float* d_eq, uint8_t* d_bits, int32_t bits_mode, int32_t* d_tsr, int32_t noise_mode,
                                 double noise_var, const ofdm_csi_out* out, void* stream) {
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, "ofdm_rx_demod_frames_csi");
    if (open != OFDM_OK) return open;
    const bool want = csi_wanted(out);
    if (want && !d_eq) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_csi: the LLR stage needs d_eq (it reads it)");
    const RxDev& d = h->dev;
    const int mod = h->cfg.modulation;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, n_frames, n_dsym, d_bits, bits_mode);
    if (!*bad && want) bad = csi_bad_args(n_frames, n_dsym, d.Kd, n_dsym * d.Kd, d.Kd, d.inv_snr_data, mod, noise_mode, noise_var);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_csi: %s", bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = want && n_frames > 0 && n_dsym > 0;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = csi_ensure(h, n_frames, n_dsym, d.Kd, s, "ofdm_rx_demod_frames_csi");
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, n_frames, frame_stride, frame_len, d_eq, d_bits, bits_mode, d_tsr, stream);
    if (r < 0 || !run) return r;
    int rc = csi_frames_launch(h, n_frames, OFDM_CSI_ROWS_ALL, h->c_a, d.Kd, s);
    if (rc == OFDM_OK)
        rc = csi_launch(h, d_eq, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, h->c_a, d.Kd, d.inv_snr_data, mod, noise_mode, noise_var, out, s);
    return rc != OFDM_OK ? rc : r;
}

}  // extern "C"
