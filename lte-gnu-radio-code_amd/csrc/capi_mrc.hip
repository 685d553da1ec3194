// capi_mrc.hip -- receive-diversity combining behind the batch receiver on its handle: the workspace, the stage on any device
// buffer, and the call that chains ofdm_rx_demod_frames, the |H|^2 rows, the noise estimate of the channel-state-weighted LLR
// stage and the combiner (definition: include/ofdm_mi355x.h, "receive-diversity combining").
#include "capi_internal.hpp"

namespace {
// Index range of the kernels: SOFT_MAX_* with the units n_branch*n_seg in place of the segments.
static_assert(OFDM_MRC_MAX_BRANCHES == MRC_MAX_BRANCHES, "the header's branch limit is the kernels'");
bool mrc_wanted(const ofdm_mrc_out* o) { return o && (o->llr || o->sym || o->weight); }
bool mrc_units_ok(int32_t n_branch, int64_t n_seg) { return n_seg <= SOFT_MAX_N / n_branch; }
constexpr const char* BAD_BRANCHES = "n_branch must lie in 1 .. OFDM_MRC_MAX_BRANCHES";
}  // namespace

// Declared in capi_internal.hpp: the stages of capi_despread.hip that combine branches make the same checks and fill the same table.
const char* mrc_bad_branches(int32_t n_branch) { return n_branch < 1 || n_branch > OFDM_MRC_MAX_BRANCHES ? BAD_BRANCHES : ""; }
// what the arguments alone decide (no read of the handle, no device access); "" = fine.  composite: the call that takes
// the variances from the host or estimates them.
const char* mrc_bad_args(int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride, int64_t csi_stride,
                         float rho, int32_t modulation, int32_t noise_mode, const double* h_noise_var, const double* d_sigma2,
                         bool composite) {
    if (n_seg < 0 || rows < 0 || row_len < 0) return "negative count";
    if (*mrc_bad_branches(n_branch)) return mrc_bad_branches(n_branch);
    if (row_len > SOFT_MAX_ROW || (row_len > 0 && rows > SOFT_MAX_LEN / row_len)) return "index range exceeded (rows * row_len)";
    if (seg_stride < rows * row_len) return "seg_stride < rows * row_len";
    if (csi_stride < row_len) return "csi_stride < row_len";
    if (!soft_mod_ok(modulation)) return "modulation must be 2, 4 or 6 bits per symbol (no BPSK soft metrics)";
    if (composite) {
        if (noise_mode != OFDM_MRC_NOISE_GIVEN && noise_mode != OFDM_MRC_NOISE_EST)
            return "noise_mode must be OFDM_MRC_NOISE_GIVEN or OFDM_MRC_NOISE_EST";
    } else if (noise_mode != OFDM_MRC_NOISE_GIVEN && noise_mode != OFDM_MRC_NOISE_SEG) {
        return "noise_mode must be OFDM_MRC_NOISE_GIVEN or OFDM_MRC_NOISE_SEG";
    }
    if (noise_mode == OFDM_MRC_NOISE_GIVEN) {
        if (!h_noise_var) return "OFDM_MRC_NOISE_GIVEN needs h_noise_var";
        for (int b = 0; b < n_branch; ++b)
            if (!(std::isfinite(h_noise_var[b]) && h_noise_var[b] > 0.0)) return "OFDM_MRC_NOISE_GIVEN needs every noise_var finite and > 0";
    }
    if (noise_mode == OFDM_MRC_NOISE_SEG && !d_sigma2) return "OFDM_MRC_NOISE_SEG needs d_sigma2";
    if (!(std::isfinite(rho) && rho >= 0.f)) return "rho must be finite and >= 0";
    if (!mrc_units_ok(n_branch, n_seg)) return "index range exceeded (batch beyond the kernels' index range)";
    const int64_t units = n_branch * n_seg;
    if (units > 0 && (seg_stride > SOFT_MAX_LEN / units || csi_stride > SOFT_MAX_LEN / units))
        return "index range exceeded (batch beyond the kernels' index range)";
    return "";
}
// the arguments of the combiner's {c, t} table; d_sigma2 == null: the host array (OFDM_MRC_NOISE_GIVEN)
MrcArgs mrc_table_args(int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride, const float* d_csi,
                       int64_t csi_stride, float rho, int32_t modulation, const double* h_noise_var, const double* d_sigma2, float2* tab) {
    MrcArgs a{};
    a.n_branch = n_branch;
    a.n_seg = n_seg;
    a.rows = rows;
    a.seg_stride = seg_stride;
    a.row_len = int(row_len);
    a.seg_len = rows * row_len;
    a.csi = d_csi;
    a.csi_stride = csi_stride;
    a.rho = rho;
    a.mod = modulation;
    a.sigma2 = d_sigma2;
    for (int b = 0; b < MRC_MAX_BRANCHES; ++b) a.noise_var[b] = (!d_sigma2 && b < n_branch) ? h_noise_var[b] : 0.0;
    a.tab = tab;
    return a;
}

namespace {
// grows the workspace; refuses inside a stream capture (growing synchronises and allocates)
int mrc_ensure(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len, bool composite, hipStream_t s,
               const char* who) {
    const int64_t units = n_branch * n_seg;
    bool fits = units * row_len <= h->cap_mrc_tab;
    if (composite)
        fits = fits && units <= h->cap_mrc_units && units * seg_slices(rows * row_len) <= h->cap_csi_items &&
               units * row_len <= h->cap_csi_tab;
    return grow_outside_capture(fits, s, who, "ofdm_rx_reserve_mrc", [&] { return ofdm_rx_reserve_mrc(h, n_branch, n_seg, rows, row_len); });
}
int mrc_launch(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride,
               const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, const double* h_noise_var,
               const double* d_sigma2, const ofdm_mrc_out* out, double* d_sigma2_out, hipStream_t s) {
    MrcArgs a = mrc_table_args(n_branch, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, modulation, h_noise_var, d_sigma2, h->m_tab);
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_slices = seg_slices(a.seg_len);
    a.llr = out ? out->llr : nullptr;
    a.osym = out ? reinterpret_cast<cf*>(out->sym) : nullptr;
    a.weight = out ? out->weight : nullptr;
    a.sigma2_out = d_sigma2_out;
    HIP_TRY(launch_combine_mrc(a, s));
    return OFDM_OK;
}
}  // namespace

extern "C" {

int ofdm_rx_reserve_mrc(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_mrc: null handle");
    if (n_seg < 0 || rows < 0 || row_len < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_mrc: negative count");
    if (*mrc_bad_branches(n_branch)) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_mrc: %s", mrc_bad_branches(n_branch));
    if (!mrc_units_ok(n_branch, n_seg) || row_len > SOFT_MAX_ROW || (row_len > 0 && rows > SOFT_MAX_LEN / row_len) ||
        (n_seg > 0 && row_len > SOFT_MAX_LEN / (n_branch * n_seg)))
        return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_mrc: batch too large");
    const int64_t units = n_branch * n_seg;
    // the composite call runs the |H|^2 rows and the noise estimate of the channel-state-weighted LLR stage over the units
    const int rc_csi = ofdm_rx_reserve_csi(h, units, rows, row_len);
    if (rc_csi != OFDM_OK) return rc_csi;
    const int64_t tab = std::max(units * row_len, h->cap_mrc_tab);
    const int64_t n_units = std::max(units, h->cap_mrc_units);
    if (tab <= h->cap_mrc_tab && n_units <= h->cap_mrc_units) return OFDM_OK;
    return regrow(h, {{&h->cap_mrc_tab, tab}, {&h->cap_mrc_units, n_units}}, ws_buf(&h->m_tab, size_t(tab)),
                  ws_buf(&h->m_sigma2, size_t(n_units)));
}

int ofdm_combine_csi_frames(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len,
                            int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, int32_t modulation,
                            int32_t noise_mode, const double* h_noise_var, const double* d_sigma2, const ofdm_mrc_out* out,
                            void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_combine_csi_frames: null handle");
    const char* bad = mrc_bad_args(n_branch, n_seg, rows, row_len, seg_stride, csi_stride, rho, modulation, noise_mode, h_noise_var,
                                   d_sigma2, false);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_combine_csi_frames: %s", bad);
    if (n_seg == 0 || rows == 0 || row_len == 0 || !mrc_wanted(out)) return OFDM_OK;
    if (!d_sym || !d_csi) return fail(OFDM_ERR_INVALID, "ofdm_combine_csi_frames: null d_sym or d_csi");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = mrc_ensure(h, n_branch, n_seg, rows, row_len, false, s, "ofdm_combine_csi_frames");
    if (rc != OFDM_OK) return rc;
    return mrc_launch(h, d_sym, n_branch, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, modulation, h_noise_var,
                      noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, out, nullptr, s);
}

int64_t ofdm_rx_demod_frames_mrc(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                 int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode, const double* h_noise_var,
                                 const ofdm_mrc_out* out, double* d_sigma2_out, void* stream) {
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, "ofdm_rx_demod_frames_mrc");
    if (open != OFDM_OK) return open;
    if (*mrc_bad_branches(n_branch) || !mrc_units_ok(n_branch, n_frames))
        return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_mrc: %s", BAD_BRANCHES);
    if (!d_eq) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_mrc: the combiner needs d_eq (it reads it)");
    const RxDev& d = h->dev;
    const int mod = h->cfg.modulation;
    const int64_t units = n_branch * n_frames;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, units, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad)
        bad = mrc_bad_args(n_branch, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, d.Kd, d.inv_snr_data, mod, noise_mode, h_noise_var, nullptr,
                           true);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_mrc: %s", bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = (mrc_wanted(out) || d_sigma2_out) && units > 0 && n_dsym > 0;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = mrc_ensure(h, n_branch, n_frames, n_dsym, d.Kd, true, s, "ofdm_rx_demod_frames_mrc");
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, units, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !run) return r;
    int rc = ofdm_rx_csi_frames(h, units, OFDM_CSI_ROWS_ALL, h->c_a, d.Kd, stream);
    const bool est = noise_mode == OFDM_MRC_NOISE_EST;
    if (rc == OFDM_OK && est) {                             // the estimation pass of the channel-state-weighted LLR stage, per unit
        ofdm_csi_out o{nullptr, h->m_sigma2, nullptr};
        rc = ofdm_demap_csi_frames(h, d_eq, units, n_dsym, d.Kd, n_dsym * d.Kd, h->c_a, d.Kd, d.inv_snr_data, mod, OFDM_CSI_NOISE_EST,
                                   0.0, &o, stream);
    }
    if (rc == OFDM_OK)
        rc = mrc_launch(h, d_eq, n_branch, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, h->c_a, d.Kd, d.inv_snr_data, mod, h_noise_var,
                        est ? h->m_sigma2 : nullptr, out, d_sigma2_out, s);
    return rc != OFDM_OK ? rc : r;
}

}  // extern "C"
