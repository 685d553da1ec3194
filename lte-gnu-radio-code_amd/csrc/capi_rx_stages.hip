// capi_rx_stages.hip -- the stages that run behind the batch receiver on its handle: segmented soft de-mapper and pilot-aided
// phase tracking (with ofdm_rx_set_pilots), and the calls that chain them to ofdm_rx_demod_frames.
#include "capi_internal.hpp"

// ---- segmented soft de-mapper (one sigma per segment = per frame of the batch path)
namespace {
bool soft_wanted(const ofdm_soft_out* o) { return o && (o->soft0 || o->soft1 || o->llr || o->sigma); }
// argument check shared by both entry points (no device access); "" = fine
const char* soft_bad_args(int64_t n_seg, int64_t seg_len, int64_t seg_stride) {
    if (n_seg < 0 || seg_len < 0) return "negative count";
    if (seg_stride < seg_len) return "seg_stride < seg_len";
    if (n_seg > SOFT_MAX_N || seg_len > SOFT_MAX_LEN || (n_seg > 0 && seg_stride > SOFT_MAX_LEN / n_seg))
        return "batch beyond the kernels' index range";
    return "";
}
// grows the partial-sum workspace; refuses inside a stream capture (growing synchronises and allocates)
int soft_ensure(ofdm_rx* h, int64_t n_seg, int64_t seg_len, hipStream_t s, const char* who) {
    return grow_outside_capture(n_seg * seg_slices(seg_len) <= h->cap_seg_partial, s, who, "ofdm_rx_reserve_soft",
                                [&] { return ofdm_rx_reserve_soft(h, n_seg, seg_len); });
}
int soft_launch(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t seg_len, int64_t seg_stride, int32_t modulation,
                const ofdm_soft_out* out, hipStream_t s) {
    SegDemapArgs a{};
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_seg = n_seg;
    a.seg_len = seg_len;
    a.seg_stride = seg_stride;
    a.n_slices = seg_slices(seg_len);
    a.mod = modulation;
    a.soft0 = out->soft0;
    a.soft1 = out->soft1;
    a.llr = out->llr;
    a.sigma = out->sigma;
    a.partial = h->f_seg_partial;
    HIP_TRY(launch_demap_frames(a, s));
    return OFDM_OK;
}
}  // namespace
extern "C" {

int ofdm_rx_reserve_soft(ofdm_rx* h, int64_t n_seg, int64_t seg_len) {
    if (!h || n_seg < 0 || seg_len < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_soft: bad argument");
    if (n_seg > SOFT_MAX_N || seg_len > SOFT_MAX_LEN) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_soft: batch too large");
    const int64_t need = n_seg * seg_slices(seg_len);
    if (need <= h->cap_seg_partial) return OFDM_OK;
    return regrow(h, {{&h->cap_seg_partial, need}}, ws_buf(&h->f_seg_partial, size_t(need)));
}

int ofdm_demap_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t seg_len, int64_t seg_stride, int32_t modulation,
                      const ofdm_soft_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_demap_frames: null handle");
    const char* bad = soft_bad_args(n_seg, seg_len, seg_stride);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_demap_frames: %s", bad);
    if (!soft_mod_ok(modulation))
        return fail(OFDM_ERR_INVALID, "ofdm_demap_frames: modulation must be 2, 4 or 6 bits per symbol (no BPSK soft metrics)");
    if (n_seg == 0 || seg_len == 0 || !soft_wanted(out)) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "ofdm_demap_frames: null d_sym");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = soft_ensure(h, n_seg, seg_len, s, "ofdm_demap_frames");
    if (rc != OFDM_OK) return rc;
    return soft_launch(h, d_sym, n_seg, seg_len, seg_stride, modulation, out, s);
}

int64_t ofdm_rx_demod_frames_soft(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                  float* d_eq, uint8_t* d_bits, int32_t bits_mode, int32_t* d_tsr, const ofdm_soft_out* soft,
                                  void* stream) {
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, "ofdm_rx_demod_frames_soft");
    if (open != OFDM_OK) return open;
    const bool want = soft_wanted(soft);
    if (want && !d_eq) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_soft: soft outputs need d_eq (the soft pass reads it)");
    const int mod = h->cfg.modulation;
    if (want && !soft_mod_ok(mod))
        return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_soft: soft metrics need QPSK, 16-QAM or 64-QAM");
    const RxDev& d = h->dev;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    const int64_t seg_len = n_dsym * d.Kd;
    // the checks ofdm_rx_demod_frames makes, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, n_frames, n_dsym, d_bits, bits_mode);
    if (!*bad && want) bad = soft_bad_args(n_frames, seg_len, seg_len);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_soft: %s", bad);
    hipStream_t s = pick_stream(h, stream);
    if (want && n_frames > 0 && seg_len > 0) {              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        int rc = soft_ensure(h, n_frames, seg_len, s, "ofdm_rx_demod_frames_soft");
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, n_frames, frame_stride, frame_len, d_eq, d_bits, bits_mode, d_tsr, stream);
    if (r < 0 || !want || n_frames == 0 || seg_len == 0) return r;
    const int rc = soft_launch(h, d_eq, n_frames, seg_len, seg_len, mod, soft, s);
    return rc != OFDM_OK ? rc : r;
}

// ---- pilot-aided phase tracking behind the batch receiver (definition: include/ofdm_mi355x.h)
}  // extern "C"
namespace {
constexpr int64_t PILOT_MAX_ROWS = int64_t(1) << 31;      // rows of one call: the row kernel's grid stays below 2^31 workgroups
bool pilot_wanted(const ofdm_pilot_out* o) { return o && (o->data || o->bits || o->cpe || o->slope || o->cfo); }
// argument check shared by both entry points (no device access); "" = fine
const char* pilot_bad_args(const ofdm_rx* h, int64_t n_seg, int64_t rows, int64_t seg_stride, int32_t rows_per_pattern, int32_t mode,
                           const ofdm_pilot_out* out) {
    // what the arguments alone decide comes first: these checks do not read the handle
    if (mode != OFDM_PILOT_CPE && mode != OFDM_PILOT_CPE_SLOPE) return "mode must be OFDM_PILOT_CPE or OFDM_PILOT_CPE_SLOPE";
    if (n_seg < 0 || rows < 0) return "negative count";
    if (rows_per_pattern < 1) return "rows_per_pattern < 1";
    if (out && out->slope && mode != OFDM_PILOT_CPE_SLOPE) return "slope output needs OFDM_PILOT_CPE_SLOPE";
    if (out && out->bits) {
        if (!out->data) return "bits are the hard decisions of data: data is required with bits";
        if (out->bits_mode != OFDM_BITS_PACKED && out->bits_mode != OFDM_BITS_UNPACKED)
            return "bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    }
    if (h->n_pilots == 0) return "no pilots set (ofdm_rx_set_pilots)";
    if (mode == OFDM_PILOT_CPE_SLOPE && h->n_pilots < 2) return "OFDM_PILOT_CPE_SLOPE needs at least two pilots";
    const int64_t K = h->dev.Kd;
    if (rows > SOFT_MAX_LEN / K || seg_stride < rows * K) return "seg_stride < rows * num_data_bins";
    if (n_seg >= SOFT_MAX_N || (n_seg > 0 && (seg_stride > SOFT_MAX_LEN / n_seg || rows > PILOT_MAX_ROWS / n_seg)))
        return "batch beyond the kernels' index range";
    if (out && out->bits) {
        const int mod = h->cfg.modulation;
        if (!soft_mod_ok(mod)) return "hard bits need QPSK, 16-QAM or 64-QAM";
        if (out->bits_mode == OFDM_BITS_PACKED && ((K - h->n_pilots) * mod) % 8 != 0)
            return "packed bits need (num_data_bins - n_pilots) * bits per symbol % 8 == 0";
    }
    return "";
}
// grows the pilot-sum workspace; refuses inside a stream capture (growing synchronises and allocates)
int pilot_ensure(ofdm_rx* h, int64_t n_seg, int64_t rows, hipStream_t s, const char* who) {
    return grow_outside_capture(n_seg * rows <= h->cap_usum, s, who, "ofdm_rx_reserve_pilots", [&] { return ofdm_rx_reserve_pilots(h, n_seg, rows); });
}
int pilot_launch(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t seg_stride, int32_t rows_per_pattern,
                 int32_t mode, const ofdm_pilot_out* out, hipStream_t s) {
    const RxDev& d = h->dev;
    PilotArgs a{};
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_seg = n_seg;
    a.rows = rows;
    a.seg_stride = seg_stride;
    a.K = d.Kd;
    a.Kd = d.Kd - h->n_pilots;
    a.n_pilots = h->n_pilots;
    a.g_log2 = pilot_group_log2(a.Kd);
    a.rows_per_group = pilot_rows_per_group(a.K, a.g_log2);
    a.slope = mode == OFDM_PILOT_CPE_SLOPE;
    a.mod = h->cfg.modulation;
    a.pilot_conj = h->pilot_conj;
    a.pidx = h->p_idx;
    a.pk = h->p_k;
    a.src = h->p_src;
    a.kbar = h->p_kbar;
    a.inv_skk = h->p_inv_skk;
    a.data = reinterpret_cast<cf*>(out->data);
    a.bits = out->bits;
    a.bits_mode = out->bits_mode;
    a.cpe = reinterpret_cast<cf*>(out->cpe);
    a.slope_out = out->slope;
    a.usum = out->cfo ? h->f_usum : nullptr;
    a.cfo = out->cfo;
    a.rows_per_pattern = rows_per_pattern;
    a.cfo_scale = double(d.nfft) / (2.0 * M_PI * double(d.L));
    HIP_TRY(launch_pilot_track(a, s));
    return OFDM_OK;
}
}  // namespace
extern "C" {

int ofdm_rx_set_pilots(ofdm_rx* h, const int32_t* h_locations, int32_t n_pilots, float pilot_re, float pilot_im) {
    if (!h || n_pilots < 0 || (n_pilots > 0 && !h_locations)) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_pilots: bad argument");
    const int K = h->dev.Kd;
    if (n_pilots > K) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_pilots: %d pilots in %d occupied bins", n_pilots, K);
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
    if (n_pilots > 0 && !(std::isfinite(pilot_re) && std::isfinite(pilot_im) && (pilot_re != 0.f || pilot_im != 0.f)))
        return fail(OFDM_ERR_INVALID, "ofdm_rx_set_pilots: pilot value must be finite and non-zero");
    const int drained = drain(h);
    if (drained != OFDM_OK) return drained;
    free_dev(&h->p_idx, &h->p_k, &h->p_src);
    h->n_pilots = 0;
    if (n_pilots == 0) return OFDM_OK;
    // signed offsets of the pilots (ascending list index), their mean and spread; the source index of every data entry
    std::vector<float> pk(size_t(n_pilots), 0.f);
    double kbar = 0.0, skk = 0.0;
    for (int p = 0; p < n_pilots; ++p) {
        const int i = idx[size_t(p)], k = i < K / 2 ? i - K / 2 : i - K / 2 + 1;
        pk[size_t(p)] = float(k);
        kbar += double(k) / n_pilots;
    }
    for (int p = 0; p < n_pilots; ++p) skk += (double(pk[size_t(p)]) - kbar) * (double(pk[size_t(p)]) - kbar);
    std::vector<uint16_t> src;
    for (int i = 0, p = 0; i < K; ++i) {
        if (p < n_pilots && idx[size_t(p)] == i)
            ++p;
        else
            src.push_back(uint16_t(i));
    }
    if (src.size() & 1) src.push_back(src.back());                    // the kernel reads the table in pairs
    if (src.empty()) src.assign(2, 0);
    int rc = upload(&h->p_idx, idx);
    if (rc == OFDM_OK) rc = upload(&h->p_k, pk);
    if (rc == OFDM_OK) rc = upload(&h->p_src, src);
    if (rc != OFDM_OK) return rc;
    h->pilot_conj = cf{pilot_re, -pilot_im};
    h->p_kbar = float(kbar);
    h->p_inv_skk = skk > 0.0 ? float(1.0 / skk) : 0.f;
    h->n_pilots = n_pilots;
    return OFDM_OK;
}

int ofdm_rx_reserve_pilots(ofdm_rx* h, int64_t n_seg, int64_t rows) {
    if (!h || n_seg < 0 || rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_pilots: bad argument");
    if (n_seg >= SOFT_MAX_N || (n_seg > 0 && rows > PILOT_MAX_ROWS / n_seg))
        return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_pilots: batch too large");
    const int64_t need = n_seg * rows;
    if (need <= h->cap_usum) return OFDM_OK;
    return regrow(h, {{&h->cap_usum, need}}, ws_buf(&h->f_usum, size_t(need)));
}

int ofdm_pilot_track_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t seg_stride,
                            int32_t rows_per_pattern, int32_t mode, const ofdm_pilot_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_pilot_track_frames: null handle");
    const char* bad = pilot_bad_args(h, n_seg, rows, seg_stride, rows_per_pattern, mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_pilot_track_frames: %s", bad);
    if (n_seg == 0 || !pilot_wanted(out)) return OFDM_OK;
    if (!d_sym && rows > 0) return fail(OFDM_ERR_INVALID, "ofdm_pilot_track_frames: null d_sym");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    if (out->cfo) {
        const int rc = pilot_ensure(h, n_seg, rows, s, "ofdm_pilot_track_frames");
        if (rc != OFDM_OK) return rc;
    }
    return pilot_launch(h, d_sym, n_seg, rows, seg_stride, rows_per_pattern, mode, out, s);
}

int64_t ofdm_rx_demod_frames_pilots(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                    float* d_eq, int32_t* d_tsr, int32_t mode, const ofdm_pilot_out* out, const ofdm_soft_out* soft,
                                    void* stream) {
    const int open = demod_stage_open(h, d_iq && d_eq, n_frames, frame_stride, frame_len, "ofdm_rx_demod_frames_pilots",
                                      "bad argument (d_eq is required: the pilot stage reads it)");
    if (open != OFDM_OK) return open;
    const RxDev& d = h->dev;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the three stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, n_frames, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad) bad = pilot_bad_args(h, n_frames, n_dsym, n_dsym * d.Kd, d.D, mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_pilots: %s", bad);
    const bool want = pilot_wanted(out), want_soft = soft_wanted(soft);
    const int64_t seg_len = n_dsym * (d.Kd - h->n_pilots);
    if (want_soft) {
        if (!want || !out->data)
            return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_pilots: soft outputs need out->data (the soft pass reads it)");
        if (!soft_mod_ok(h->cfg.modulation))
            return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_pilots: soft metrics need QPSK, 16-QAM or 64-QAM");
        bad = soft_bad_args(n_frames, seg_len, seg_len);
        if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_demod_frames_pilots: %s", bad);
    }
    hipStream_t s = pick_stream(h, stream);
    if (n_frames > 0) {                                               // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        int rc = OFDM_OK;
        if (want && out->cfo) rc = pilot_ensure(h, n_frames, n_dsym, s, "ofdm_rx_demod_frames_pilots");
        if (rc == OFDM_OK && want_soft && seg_len > 0) rc = soft_ensure(h, n_frames, seg_len, s, "ofdm_rx_demod_frames_pilots");
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, n_frames, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !want || n_frames == 0) return r;
    int rc = pilot_launch(h, d_eq, n_frames, n_dsym, n_dsym * d.Kd, d.D, mode, out, s);
    if (rc == OFDM_OK && want_soft && seg_len > 0) rc = soft_launch(h, out->data, n_frames, seg_len, seg_len, h->cfg.modulation, soft, s);
    return rc != OFDM_OK ? rc : r;
}

}  // extern "C"
