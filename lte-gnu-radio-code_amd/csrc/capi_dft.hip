// capi_dft.hip -- DFT-spread OFDM on both handles: the plan cache, the transform precoder and the composite transmitter, the
// despreading stage and the call that chains it behind ofdm_rx_demod_frames (definition: include/ofdm_mi355x.h, "DFT-spread
// OFDM"), and the stage that combines B receive branches before it despreads, with its composite call
// ("receive diversity for DFT-spread OFDM"): it lives here for the plan cache.  Last, the allocation sets of
// both handles and the calls that walk them ("multi-user allocations of DFT-spread OFDM"): they share the
// argument checks of the despreading stage; and the stage that combines B branches per allocation of that set ("receive diversity
// for multi-user allocations of DFT-spread OFDM").
#include "capi_internal.hpp"

void dft_plans_free(DftPlanCache& c) {
    for (int i = 0; i < c.n; ++i) free_dev(&c.d_tw[i]);
    c.n = 0;
}

namespace {

int dft_plan_find(DftPlanCache& c, int M) {
    for (int i = 0; i < c.n; ++i)
        if (c.pl[i].M == M) {
            c.used[i] = ++c.tick;
            return i;
        }
    return -1;
}
// builds the plan for M (a size that is ok) into the cache; the least recently used one makes room
template <class H>
int dft_plan_build(H* h, int M, int* slot) {
    DftPlanCache& c = h->dft;
    DftPlan pl;
    dft_make_plan(M, pl);
    std::vector<cf> tw(size_t(M), cf{1.f, 0.f});
    for (int j = 0; j < M; ++j) {
        const double ang = -2.0 * M_PI * double(j) / double(M);
        tw[size_t(j)] = cf{float(std::cos(ang)), float(std::sin(ang))};
    }
    HIP_TRY(dft_spread_prepare());
    if (c.n == DftPlanCache::SLOTS) {
        int v = 0;
        for (int i = 1; i < c.n; ++i)
            if (c.used[i] < c.used[v]) v = i;
        const int drained = drain(h);                       // work queued on a caller's stream may still read the table
        if (drained != OFDM_OK) return drained;
        free_dev(&c.d_tw[v]);
        const int last = c.n - 1;
        c.pl[v] = c.pl[last];
        c.d_tw[v] = c.d_tw[last];
        c.used[v] = c.used[last];
        c.d_tw[last] = nullptr;
        c.n = last;
    }
    const int rc = upload(&c.d_tw[c.n], tw);
    if (rc != OFDM_OK) {
        free_dev(&c.d_tw[c.n]);
        return rc;
    }
    c.pl[c.n] = pl;
    c.used[c.n] = ++c.tick;
    *slot = c.n++;
    return OFDM_OK;
}
const char* dft_bad_size(int32_t M) { return dft_size_ok(M) ? "" : "M must be 2^a 3^b 5^c in 1 .. 4096"; }
bool dft_rows_in_range(const DftPlan& pl, int64_t rows, int64_t n_seg) {
    const int64_t groups = (rows + pl.rows_per_group - 1) / pl.rows_per_group;
    return n_seg <= 0 || groups <= DFT_MAX_GROUPS / n_seg;
}

// ---- transmitter
int tx_spread_ensure(ofdm_tx* h, int32_t M, int64_t ws_rows, hipStream_t s, const char* who, int* slot) {
    *slot = dft_plan_find(h->dft, M);
    if (*slot >= 0 && ws_rows <= h->cap_sp_rows) return OFDM_OK;
    int rc = refuse_growth_in_capture(s, who, "ofdm_tx_reserve_spread");
    if (rc == OFDM_OK) rc = ofdm_tx_reserve_spread(h, M, ws_rows);
    if (rc == OFDM_OK) *slot = dft_plan_find(h->dft, M);
    return rc;
}

// ---- receiver
bool despread_wanted(const ofdm_despread_out* o) { return o && (o->sym || o->llr || o->bits || o->beta || o->weight); }
// what the arguments alone decide (no read of the handle, no device access); "" = fine
const char* despread_bad_args(const float* d_sym, int64_t n_seg, int64_t rows, int32_t M, int64_t seg_stride, bool has_csi,
                              int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode, double noise_var,
                              const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out) {
    if (*dft_bad_size(M)) return dft_bad_size(M);
    if (n_seg < 0 || rows < 0) return "negative count";
    if (rows > SOFT_MAX_LEN / M) return "index range exceeded (rows * M)";
    if (seg_stride < rows * M) return "seg_stride < rows * M";
    if (!soft_mod_ok(modulation)) return "modulation must be 2, 4 or 6 bits per symbol (no BPSK soft metrics)";
    if (has_csi) {
        if (csi_stride < M) return "csi_stride < M";
        if (noise_mode != OFDM_DESPREAD_NOISE_RHO && noise_mode != OFDM_DESPREAD_NOISE_GIVEN && noise_mode != OFDM_DESPREAD_NOISE_SEG)
            return "noise_mode must be OFDM_DESPREAD_NOISE_RHO, OFDM_DESPREAD_NOISE_GIVEN or OFDM_DESPREAD_NOISE_SEG";
        if (noise_mode == OFDM_DESPREAD_NOISE_GIVEN && !(std::isfinite(noise_var) && noise_var > 0.0))
            return "OFDM_DESPREAD_NOISE_GIVEN needs a finite noise_var > 0";
        if (noise_mode == OFDM_DESPREAD_NOISE_SEG && !d_sigma2) return "OFDM_DESPREAD_NOISE_SEG needs d_sigma2";
        if (!(std::isfinite(rho) && rho >= 0.f)) return "rho must be finite and >= 0";
    }
    if (!despread_wanted(out)) return "out is NULL or holds no pointer";
    if (out->bits) {
        if (!bits_mode_ok(bits_mode)) return "bits wanted: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
        if (bits_mode == OFDM_BITS_PACKED && (int64_t(M) * modulation) % 8 != 0) return "packed bits need M * bits per symbol % 8 == 0";
    }
    if (out->sym && out->sym == d_sym && seg_stride != rows * M) return "out->sym == d_sym needs seg_stride == rows * M";
    if (n_seg > SOFT_MAX_N || (n_seg > 0 && (seg_stride > SOFT_MAX_LEN / n_seg || (has_csi && csi_stride > SOFT_MAX_LEN / n_seg))))
        return "index range exceeded (batch beyond the kernels' index range)";
    DftPlan pl;
    dft_make_plan(M, pl);
    if (!dft_rows_in_range(pl, rows, n_seg)) return "index range exceeded (more than 2^31 - 1 workgroups)";
    return "";
}
// the plan for M and the tables of n_seg segments (frames: also their |H|^2 rows), or a refusal inside a capture
int despread_ensure(ofdm_rx* h, int32_t M, int64_t n_seg, hipStream_t s, const char* who, int* slot) {
    *slot = dft_plan_find(h->dft, M);
    if (*slot >= 0 && n_seg <= h->cap_ds_seg) return OFDM_OK;
    int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve_despread");
    if (rc == OFDM_OK) rc = ofdm_rx_reserve_despread(h, M, n_seg);
    if (rc == OFDM_OK) *slot = dft_plan_find(h->dft, M);
    return rc;
}
int despread_launch(ofdm_rx* h, int slot, const float* d_sym, int64_t n_seg, int64_t rows, int64_t seg_stride, const float* d_csi,
                    int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode, double noise_var, const double* d_sigma2,
                    int32_t bits_mode, const ofdm_despread_out* out, hipStream_t s) {
    DespreadArgs a{};
    a.pl = h->dft.pl[slot];
    a.tw = h->dft.d_tw[slot];
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_seg = n_seg;
    a.rows = rows;
    a.seg_stride = seg_stride;
    a.groups_per_seg = (rows + a.pl.rows_per_group - 1) / a.pl.rows_per_group;
    a.csi = d_csi;
    a.csi_stride = csi_stride;
    a.rho = rho;
    a.noise_mode = noise_mode;
    a.noise_var = noise_var;
    a.sigma2 = d_sigma2;
    a.mod = modulation;
    a.bits_mode = bits_mode;
    a.osym = reinterpret_cast<cf*>(out->sym);
    a.llr = out->llr;
    a.bits = out->bits;
    a.beta = out->beta;
    a.weight = out->weight;
    a.tab = h->ds_tab;
    HIP_TRY(launch_despread(a, s));
    return OFDM_OK;
}

// ---- receiver, B branches combined before the transform
bool mrc_despread_wanted(const ofdm_mrc_despread_out* o) { return o && (o->sym || o->llr || o->bits || o->beta || o->weight || o->comb); }
// what the arguments alone decide: what ofdm_combine_csi_frames and ofdm_dft_despread_frames refuse for the same argument; "" = fine
const char* mrc_despread_bad_args(int32_t n_branch, int64_t n_seg, int64_t rows, int32_t M, int64_t seg_stride, int64_t csi_stride,
                                  float rho, int32_t modulation, int32_t noise_mode, const double* h_noise_var, const double* d_sigma2,
                                  int32_t bits_mode, const ofdm_mrc_despread_out* out) {
    if (*dft_bad_size(M)) return dft_bad_size(M);
    if (noise_mode == OFDM_MRC_NOISE_EST)
        return "OFDM_MRC_NOISE_EST is refused (a spread signal has no constellation points per bin): pass OFDM_MRC_NOISE_GIVEN or "
               "OFDM_MRC_NOISE_SEG";
    const char* bad = mrc_bad_args(n_branch, n_seg, rows, M, seg_stride, csi_stride, rho, modulation, noise_mode, h_noise_var, d_sigma2,
                                   false);
    if (*bad) return bad;
    if (!mrc_despread_wanted(out)) return "out is NULL or holds no pointer";
    if (out->bits) {
        if (!bits_mode_ok(bits_mode)) return "bits wanted: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
        if (bits_mode == OFDM_BITS_PACKED && (int64_t(M) * modulation) % 8 != 0) return "packed bits need M * bits per symbol % 8 == 0";
    }
    DftPlan pl;
    dft_make_plan(M, pl);
    if (!dft_rows_in_range(pl, rows, n_seg)) return "index range exceeded (more than 2^31 - 1 workgroups)";
    return "";
}
// the plan for M, the table of the units and (frames > 0: the composite call) their |H|^2 rows, or a refusal inside a capture
int mrc_despread_ensure(ofdm_rx* h, int32_t M, int32_t n_branch, int64_t n_seg, bool composite, hipStream_t s, const char* who,
                        int* slot) {
    const int64_t units = n_branch * n_seg;
    *slot = dft_plan_find(h->dft, M);
    if (*slot >= 0 && units * M <= h->cap_md_tab && (!composite || units <= h->cap_md_units)) return OFDM_OK;
    int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve_mrc_despread");
    if (rc == OFDM_OK) rc = ofdm_rx_reserve_mrc_despread(h, M, n_branch, n_seg);
    if (rc == OFDM_OK) *slot = dft_plan_find(h->dft, M);
    return rc;
}
// d_sigma2 == null: the host array (OFDM_MRC_NOISE_GIVEN)
int mrc_despread_launch(ofdm_rx* h, int slot, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t seg_stride,
                        const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, const double* h_noise_var,
                        const double* d_sigma2, int32_t bits_mode, const ofdm_mrc_despread_out* out, hipStream_t s) {
    const DftPlan& pl = h->dft.pl[slot];
    MrcArgs t{};
    t.n_branch = n_branch;
    t.n_seg = n_seg;
    t.rows = rows;
    t.seg_stride = seg_stride;
    t.row_len = pl.M;
    t.seg_len = rows * pl.M;
    t.csi = d_csi;
    t.csi_stride = csi_stride;
    t.rho = rho;
    t.mod = modulation;
    t.sigma2 = d_sigma2;
    for (int b = 0; b < MRC_MAX_BRANCHES; ++b) t.noise_var[b] = (!d_sigma2 && b < n_branch) ? h_noise_var[b] : 0.0;
    t.tab = h->md_tab;
    HIP_TRY(launch_mrc_table(t, s));
    MrcDespreadArgs a{};
    a.pl = pl;
    a.tw = h->dft.d_tw[slot];
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_branch = n_branch;
    a.n_seg = n_seg;
    a.rows = rows;
    a.seg_stride = seg_stride;
    a.groups_per_seg = (rows + pl.rows_per_group - 1) / pl.rows_per_group;
    a.tab = h->md_tab;
    a.mod = modulation;
    a.bits_mode = bits_mode;
    a.osym = reinterpret_cast<cf*>(out->sym);
    a.llr = out->llr;
    a.bits = out->bits;
    a.beta = out->beta;
    a.weight = out->weight;
    a.comb = reinterpret_cast<cf*>(out->comb);
    HIP_TRY(launch_mrc_despread(a, s));
    return OFDM_OK;
}

}  // namespace

extern "C" {

int ofdm_dft_size_ok(int32_t M) { return dft_size_ok(M) ? 1 : 0; }

int ofdm_dft_plan_info(int32_t M, int32_t* n_pass, int32_t* radix8, int32_t* rows_per_group) {
    DftPlan pl;
    if (!dft_make_plan(M, pl)) return fail(OFDM_ERR_INVALID, "ofdm_dft_plan_info: %s", dft_bad_size(M));
    if (n_pass) *n_pass = pl.n_pass;
    if (radix8) *radix8 = 0;
    if (rows_per_group) *rows_per_group = pl.rows_per_group;
    return OFDM_OK;
}

int ofdm_tx_reserve_spread(ofdm_tx* h, int32_t M, int64_t n_rows) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: null handle");
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: %s", dft_bad_size(M));
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: negative count");
    if (n_rows > INT32_MAX) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = dft_plan_find(h->dft, M);
    if (slot < 0) {
        const int rc = dft_plan_build(h, M, &slot);
        if (rc != OFDM_OK) return rc;
    }
    if (n_rows <= h->cap_sp_rows) return OFDM_OK;
    const TxDev& d = h->dev;
    return regrow(h, {{&h->cap_sp_rows, n_rows}}, ws_buf(&h->sp_sym, size_t(n_rows) * d.Kd), ws_buf(&h->sp_grid, size_t(n_rows) * d.nfft),
                  ws_buf(&h->sp_time, size_t(n_rows) * d.L));
}

int ofdm_tx_dft_spread(ofdm_tx* h, const float* d_sym, int64_t n_rows, int32_t M, float* d_out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_dft_spread: null handle");
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "ofdm_tx_dft_spread: %s", dft_bad_size(M));
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_dft_spread: negative count");
    DftPlan pl;
    dft_make_plan(M, pl);
    if (n_rows > SOFT_MAX_LEN / M || !dft_rows_in_range(pl, n_rows, 1)) return fail(OFDM_ERR_INVALID, "ofdm_tx_dft_spread: index range exceeded");
    if (n_rows == 0) return OFDM_OK;
    if (!d_sym || !d_out) return fail(OFDM_ERR_INVALID, "ofdm_tx_dft_spread: null d_sym or d_out");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    int slot = -1;
    const int rc = tx_spread_ensure(h, M, 0, s, "ofdm_tx_dft_spread", &slot);
    if (rc != OFDM_OK) return rc;
    HIP_TRY(launch_dft_rows(h->dft.pl[slot], h->dft.d_tw[slot], reinterpret_cast<const cf*>(d_sym), reinterpret_cast<cf*>(d_out), n_rows,
                            0, s));
    return OFDM_OK;
}

int64_t ofdm_tx_modulate_frames_spread(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                                       float* d_iq, int64_t frame_stride, void* stream) {
    const char* who = "ofdm_tx_modulate_frames_spread";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (n_frames < 0 || n_sym < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (!bits_mode_ok(bits_mode)) return fail(OFDM_ERR_INVALID, "%s: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED", who);
    const TxDev& d = h->dev;
    const int SD = d.S + d.D;
    if (n_sym % SD != 0) return fail(OFDM_ERR_INVALID, "%s: n_sym must be a multiple of S + D = %d", who, SD);
    if (frame_stride != int64_t(n_sym) * d.L) return fail(OFDM_ERR_INVALID, "%s: frame_stride must equal n_sym*(nfft+cp)", who);
    if (*dft_bad_size(d.Kd)) return fail(OFDM_ERR_INVALID, "%s: num_data_bins=%d: %s", who, d.Kd, dft_bad_size(d.Kd));
    if (n_frames * int64_t(n_sym) > INT32_MAX) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    const int64_t data_per_frame = int64_t(n_sym / SD) * d.D, rows = n_frames * data_per_frame;
    const int64_t bits_per_frame = data_per_frame * d.Kd * d.bps;
    if (bits_mode == OFDM_BITS_PACKED && (bits_per_frame & 7)) return fail(OFDM_ERR_INVALID, "%s: packed bits need a whole number of bytes per frame", who);
    if (rows == 0) return 0;
    if (!d_bits || !d_iq) return fail(OFDM_ERR_INVALID, "%s: null d_bits or d_iq", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = -1;
    int rc = tx_spread_ensure(h, d.Kd, rows, pick_stream(h, stream), who, &slot);
    if (rc != OFDM_OK) return rc;
    float* sym = reinterpret_cast<float*>(h->sp_sym);
    float* grid = reinterpret_cast<float*>(h->sp_grid);
    float* time = reinterpret_cast<float*>(h->sp_time);
    rc = ofdm_tx_map(h, d_bits, bits_mode, rows * d.Kd, sym, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_dft_spread(h, sym, rows, d.Kd, sym, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_grid(h, sym, rows, grid, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_ifft_cp(h, grid, rows, 1, 1, time, stream);
    if (rc != OFDM_OK) return rc;
    return ofdm_tx_mux(h, time, rows, d_iq, stream);
}

int ofdm_rx_reserve_despread(ofdm_rx* h, int32_t M, int64_t n_seg) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: null handle");
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: %s", dft_bad_size(M));
    if (n_seg < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: negative count");
    if (n_seg > SOFT_MAX_N) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = dft_plan_find(h->dft, M);
    if (slot < 0) {
        const int rc = dft_plan_build(h, M, &slot);
        if (rc != OFDM_OK) return rc;
    }
    if (n_seg <= h->cap_ds_seg) return OFDM_OK;
    return regrow(h, {{&h->cap_ds_seg, n_seg}}, ws_buf(&h->ds_tab, size_t(n_seg)), ws_buf(&h->ds_a, size_t(n_seg) * h->dev.Kd));
}

int ofdm_dft_despread_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int32_t M, int64_t seg_stride,
                             const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode,
                             double noise_var, const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_dft_despread_frames: null handle");
    const char* bad = despread_bad_args(d_sym, n_seg, rows, M, seg_stride, d_csi != nullptr, csi_stride, rho, modulation, noise_mode,
                                        noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_dft_despread_frames: %s", bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "ofdm_dft_despread_frames: null d_sym");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    int slot = -1;
    const int rc = despread_ensure(h, M, n_seg, s, "ofdm_dft_despread_frames", &slot);
    if (rc != OFDM_OK) return rc;
    return despread_launch(h, slot, d_sym, n_seg, rows, seg_stride, d_csi, csi_stride, rho, modulation, noise_mode, noise_var, d_sigma2,
                           bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_despread(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                      float* d_eq, int32_t* d_tsr, int32_t noise_mode, double noise_var, const double* d_sigma2,
                                      int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_despread";
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    if (!d_eq) return fail(OFDM_ERR_INVALID, "%s: the despreading stage needs d_eq (it reads it)", who);
    const RxDev& d = h->dev;
    const int mod = h->cfg.modulation;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, n_frames, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad)
        bad = despread_bad_args(d_eq, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, true, d.Kd, d.inv_snr_data, mod, noise_mode, noise_var,
                                d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = n_frames > 0 && n_dsym > 0;
    int slot = -1;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = despread_ensure(h, d.Kd, n_frames, s, who, &slot);
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, n_frames, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !run) return r;
    HIP_TRY(launch_csi_frames(h->f_H, d.nfft, d.Kd, nullptr, d.Kd, n_frames, h->ds_a, d.Kd, s));
    const int rc = despread_launch(h, slot, d_eq, n_frames, n_dsym, n_dsym * d.Kd, h->ds_a, d.Kd, d.inv_snr_data, mod, noise_mode, noise_var,
                                   d_sigma2, bits_mode, out, s);
    return rc != OFDM_OK ? rc : r;
}

int ofdm_rx_reserve_mrc_despread(ofdm_rx* h, int32_t M, int32_t n_branch, int64_t n_seg) {
    const char* who = "ofdm_rx_reserve_mrc_despread";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "%s: %s", who, dft_bad_size(M));
    if (n_branch < 1 || n_branch > OFDM_MRC_MAX_BRANCHES) return fail(OFDM_ERR_INVALID, "%s: n_branch must lie in 1 .. OFDM_MRC_MAX_BRANCHES", who);
    if (n_seg < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (n_seg > SOFT_MAX_N / n_branch) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = dft_plan_find(h->dft, M);
    if (slot < 0) {
        const int rc = dft_plan_build(h, M, &slot);
        if (rc != OFDM_OK) return rc;
    }
    HIP_TRY(mrc_despread_prepare());
    const int64_t units = n_branch * n_seg;
    if (units * M > h->cap_md_tab) {
        const int rc = regrow(h, {{&h->cap_md_tab, units * M}}, ws_buf(&h->md_tab, size_t(units * M)));
        if (rc != OFDM_OK) return rc;
    }
    if (units <= h->cap_md_units) return OFDM_OK;
    return regrow(h, {{&h->cap_md_units, units}}, ws_buf(&h->md_a, size_t(units) * h->dev.Kd));
}

int ofdm_combine_despread_frames(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int32_t M,
                                 int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, int32_t modulation,
                                 int32_t noise_mode, const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                 const ofdm_mrc_despread_out* out, void* stream) {
    const char* who = "ofdm_combine_despread_frames";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const char* bad = mrc_despread_bad_args(n_branch, n_seg, rows, M, seg_stride, csi_stride, rho, modulation, noise_mode, h_noise_var,
                                            d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym || !d_csi) return fail(OFDM_ERR_INVALID, "%s: null d_sym or d_csi", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    int slot = -1;
    const int rc = mrc_despread_ensure(h, M, n_branch, n_seg, false, s, who, &slot);
    if (rc != OFDM_OK) return rc;
    return mrc_despread_launch(h, slot, d_sym, n_branch, n_seg, rows, seg_stride, d_csi, csi_stride, rho, modulation, h_noise_var,
                               noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_mrc_despread(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                          int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode,
                                          const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                          const ofdm_mrc_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_mrc_despread";
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    if (n_branch < 1 || n_branch > OFDM_MRC_MAX_BRANCHES)
        return fail(OFDM_ERR_INVALID, "%s: n_branch must lie in 1 .. OFDM_MRC_MAX_BRANCHES", who);
    if (n_frames > SOFT_MAX_N / n_branch) return fail(OFDM_ERR_INVALID, "%s: batch too large (n_branch * n_frames > 2^31)", who);
    if (!d_eq) return fail(OFDM_ERR_INVALID, "%s: the stage needs d_eq (it reads it)", who);
    const RxDev& d = h->dev;
    const int mod = h->cfg.modulation;
    const int64_t units = n_branch * n_frames;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, units, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad)
        bad = mrc_despread_bad_args(n_branch, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, d.Kd, d.inv_snr_data, mod, noise_mode, h_noise_var,
                                    d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = n_frames > 0 && n_dsym > 0;
    int slot = -1;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = mrc_despread_ensure(h, d.Kd, n_branch, n_frames, true, s, who, &slot);
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, units, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !run) return r;
    HIP_TRY(launch_csi_frames(h->f_H, d.nfft, d.Kd, nullptr, d.Kd, units, h->md_a, d.Kd, s));
    const int rc = mrc_despread_launch(h, slot, d_eq, n_branch, n_frames, n_dsym, n_dsym * d.Kd, h->md_a, d.Kd, d.inv_snr_data, mod,
                                       h_noise_var, noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
    return rc != OFDM_OK ? rc : r;
}

}  // extern "C"

// ---- multi-user allocations of DFT-spread OFDM (include/ofdm_mi355x.h, "multi-user allocations of DFT-spread OFDM"; DESIGN.md
// 9.2.17): the allocation set of both handles, the despreading stage that walks it, the transform precoder and the composites.
static_assert(OFDM_MAX_ALLOCS == DFT_MAX_ALLOCS, "the header's cap is the size of the kernels' tables");
void dft_alloc_free(DftAllocSet& a) {
    free_dev(&a.d_set, &a.d_tw);
    a = DftAllocSet{};
}

namespace {

// what the lists alone decide; "" = fine.  h_mod == null: the transmitter's list (no modulations)
const char* alloc_bad_list(int32_t n_alloc, const int32_t* start, const int32_t* M, const int32_t* mod, bool want_mod) {
    if (n_alloc < 0 || n_alloc > OFDM_MAX_ALLOCS) return "n_alloc must lie in 0 .. OFDM_MAX_ALLOCS";
    if (n_alloc > 0 && (!start || !M || (want_mod && !mod))) return "null array";
    for (int u = 0; u < n_alloc; ++u) {
        if (start[u] < 0) return "start < 0";
        if (*dft_bad_size(M[u])) return dft_bad_size(M[u]);
        if (int64_t(start[u]) + M[u] > DFT_MAX_M) return "start + M > 4096";
        if (want_mod && !soft_mod_ok(mod[u])) return "modulation must be 2, 4 or 6 bits per symbol (no BPSK soft metrics)";
    }
    for (int u = 0; u < n_alloc; ++u)
        for (int v = 0; v < u; ++v)
            if (start[u] < start[v] + M[v] && start[v] < start[u] + M[u]) return "two allocations overlap";
    return "";
}
// The set of a handle replaced (n_alloc == 0: cleared).  The new tables are on the device before the old ones go; after a
// failure the previous set is still in force.
template <class H>
int alloc_set_replace(H* h, int32_t n_alloc, const int32_t* start, const int32_t* M, const int32_t* mod) {
    HIP_TRY(hipSetDevice(h->cfg.device));
    DftAllocSet nw{};
    if (n_alloc > 0) {
        HIP_TRY(dft_alloc_prepare());
        std::vector<cf> tw;
        std::vector<size_t> off(size_t(n_alloc), 0);
        int64_t sym_before = 0, bit_before = 0;
        for (int u = 0; u < n_alloc; ++u) {
            DftAllocDesc& d = nw.h[u];
            dft_make_plan(M[u], d.pl);
            d.start = start[u];
            d.mod = mod ? mod[u] : 0;
            d.sym_before = sym_before;
            d.bit_before = bit_before;
            sym_before += M[u];
            bit_before += int64_t(M[u]) * d.mod;
            nw.max_end = std::max(nw.max_end, start[u] + M[u]);
            int same = -1;
            for (int v = 0; v < u && same < 0; ++v)
                if (M[v] == M[u]) same = v;
            if (same >= 0) {
                off[size_t(u)] = off[size_t(same)];
                continue;
            }
            off[size_t(u)] = tw.size();
            for (int j = 0; j < M[u]; ++j) {                // as dft_plan_build: fp64, rounded once
                const double ang = -2.0 * M_PI * double(j) / double(M[u]);
                tw.push_back(cf{float(std::cos(ang)), float(std::sin(ang))});
            }
            if (tw.size() & 1) tw.push_back(cf{0.f, 0.f});  // every table starts on 16 bytes
        }
        nw.n = n_alloc;
        // the runs below max_end that no allocation covers
        std::vector<int> order(size_t(n_alloc), 0);
        for (int u = 0; u < n_alloc; ++u) order[size_t(u)] = u;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return start[a] < start[b]; });
        int at = 0;
        for (int u : order) {
            if (start[u] > at) {
                nw.gap_start[nw.n_gap] = at;
                nw.gap_len[nw.n_gap++] = start[u] - at;
            }
            at = start[u] + M[u];
        }
        int rc = upload(&nw.d_tw, tw);
        if (rc == OFDM_OK) {
            for (int u = 0; u < n_alloc; ++u) nw.h[u].tw = nw.d_tw + off[size_t(u)];
            rc = upload(&nw.d_set, nw.h, size_t(n_alloc));
        }
        if (rc != OFDM_OK) {
            free_dev(&nw.d_set, &nw.d_tw);
            return rc;
        }
    }
    const int drained = drain(h);                           // work queued on a caller's stream may still read the old tables
    if (drained != OFDM_OK) {
        free_dev(&nw.d_set, &nw.d_tw);
        return drained;
    }
    free_dev(&h->alloc.d_set, &h->alloc.d_tw);
    h->alloc = nw;
    return OFDM_OK;
}

// what the arguments and the set decide (no device access); "" = fine
const char* despread_alloc_bad_args(const DftAllocSet& A, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len,
                                    int64_t seg_stride, bool has_csi, int64_t csi_stride, float rho, int32_t noise_mode,
                                    double noise_var, const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out) {
    if (A.n == 0) return "no allocation set (ofdm_rx_set_allocations)";
    if (n_seg < 0 || rows < 0) return "negative count";
    if (row_len < A.max_end) return "row_len < max(start + M) of the allocation set";
    if (row_len > SOFT_MAX_ROW || rows > SOFT_MAX_LEN / row_len) return "index range exceeded (rows * row_len)";
    if (seg_stride < rows * row_len) return "seg_stride < rows * row_len";
    if (has_csi && csi_stride < row_len) return "csi_stride < row_len";
    if (out && out->sym && out->sym == d_sym) return "out->sym == d_sym is refused: the layouts differ";
    int64_t groups = 0;
    for (int u = 0; u < A.n; ++u) {
        const DftPlan& pl = A.h[u].pl;
        const char* bad = despread_bad_args(d_sym, n_seg, rows, pl.M, seg_stride, has_csi, csi_stride, rho, A.h[u].mod, noise_mode, noise_var,
                                            d_sigma2, bits_mode, out);
        if (*bad) return bad;
        groups += n_seg * ((rows + pl.rows_per_group - 1) / pl.rows_per_group);     // each term fits (checked above)
        if (groups > DFT_MAX_GROUPS) return "index range exceeded (more than 2^31 - 1 workgroups)";
    }
    if (n_seg > DFT_MAX_GROUPS / A.n) return "index range exceeded (more than 2^31 - 1 workgroups)";
    return "";
}
int despread_alloc_ensure(ofdm_rx* h, int64_t n_seg, bool composite, hipStream_t s, const char* who) {
    if (h->alloc.n * n_seg <= h->cap_da_tab && (!composite || n_seg <= h->cap_da_seg)) return OFDM_OK;
    const int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve_despread_alloc");
    return rc != OFDM_OK ? rc : ofdm_rx_reserve_despread_alloc(h, n_seg);
}
int despread_alloc_launch(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride,
                          const float* d_csi, int64_t csi_stride, float rho, int32_t noise_mode, double noise_var, const double* d_sigma2,
                          int32_t bits_mode, const ofdm_despread_out* out, hipStream_t s) {
    DespreadAllocArgs a{};
    a.set = h->alloc.d_set;
    a.n_alloc = h->alloc.n;
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_seg = n_seg;
    a.rows = rows;
    a.row_len = row_len;
    a.seg_stride = seg_stride;
    a.csi = d_csi;
    a.csi_stride = csi_stride;
    a.rho = rho;
    a.noise_mode = noise_mode;
    a.noise_var = noise_var;
    a.sigma2 = d_sigma2;
    a.bits_mode = bits_mode;
    a.osym = reinterpret_cast<cf*>(out->sym);
    a.llr = out->llr;
    a.bits = out->bits;
    a.beta = out->beta;
    a.weight = out->weight;
    a.tab = h->da_tab;
    HIP_TRY(launch_despread_alloc(a, h->alloc.h, s));
    return OFDM_OK;
}
// the rows between the stages of ofdm_tx_modulate_frames_alloc: the buffers of ofdm_tx_reserve_spread, grown without a plan
int tx_alloc_ws(ofdm_tx* h, int64_t n_rows) {
    if (n_rows <= h->cap_sp_rows) return OFDM_OK;
    const TxDev& d = h->dev;
    return regrow(h, {{&h->cap_sp_rows, n_rows}}, ws_buf(&h->sp_sym, size_t(n_rows) * d.Kd), ws_buf(&h->sp_grid, size_t(n_rows) * d.nfft),
                  ws_buf(&h->sp_time, size_t(n_rows) * d.L));
}

}  // namespace

extern "C" {

int ofdm_alloc_layout(int32_t n_alloc, const int32_t* M, const int32_t* mod, int64_t n_seg, int64_t rows, int32_t bits_mode,
                      int64_t* sym_off, int64_t* llr_off, int64_t* bits_off, int64_t* totals) {
    const char* who = "ofdm_alloc_layout";
    if (n_alloc < 1 || n_alloc > OFDM_MAX_ALLOCS) return fail(OFDM_ERR_INVALID, "%s: n_alloc must lie in 1 .. OFDM_MAX_ALLOCS", who);
    if (!M || !mod) return fail(OFDM_ERR_INVALID, "%s: null array", who);
    if (n_seg < 0 || rows < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (bits_mode != OFDM_BITS_NONE && !bits_mode_ok(bits_mode))
        return fail(OFDM_ERR_INVALID, "%s: bits_mode must be OFDM_BITS_NONE, OFDM_BITS_PACKED or OFDM_BITS_UNPACKED", who);
    if (n_seg > SOFT_MAX_N || rows > SOFT_MAX_LEN || (n_seg > 0 && rows > SOFT_MAX_LEN / n_seg))
        return fail(OFDM_ERR_INVALID, "%s: index range exceeded", who);
    for (int u = 0; u < n_alloc; ++u) {
        if (*dft_bad_size(M[u])) return fail(OFDM_ERR_INVALID, "%s: %s", who, dft_bad_size(M[u]));
        if (!soft_mod_ok(mod[u])) return fail(OFDM_ERR_INVALID, "%s: modulation must be 2, 4 or 6 bits per symbol", who);
        if (bits_mode == OFDM_BITS_PACKED && (int64_t(M[u]) * mod[u]) % 8 != 0)
            return fail(OFDM_ERR_INVALID, "%s: packed bits need M * bits per symbol %% 8 == 0", who);
    }
    const int64_t sr = n_seg * rows;
    int64_t sym = 0, bit = 0;
    for (int u = 0; u < n_alloc; ++u) {
        if (sym_off) sym_off[u] = sr * sym;
        if (llr_off) llr_off[u] = sr * bit;
        if (bits_off) bits_off[u] = bits_mode == OFDM_BITS_NONE ? 0 : bits_mode == OFDM_BITS_PACKED ? sr * bit / 8 : sr * bit;
        sym += M[u];
        bit += int64_t(M[u]) * mod[u];
    }
    if (totals) {
        totals[0] = sr * sym;
        totals[1] = sr * bit;
        totals[2] = bits_mode == OFDM_BITS_NONE ? 0 : bits_mode == OFDM_BITS_PACKED ? sr * bit / 8 : sr * bit;
    }
    return OFDM_OK;
}

int ofdm_rx_set_allocations(ofdm_rx* h, int32_t n_alloc, const int32_t* h_start, const int32_t* h_M, const int32_t* h_mod) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_allocations: null handle");
    const char* bad = alloc_bad_list(n_alloc, h_start, h_M, h_mod, true);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_set_allocations: %s", bad);
    return alloc_set_replace(h, n_alloc, h_start, h_M, h_mod);
}

int ofdm_tx_set_allocations(ofdm_tx* h, int32_t n_alloc, const int32_t* h_start, const int32_t* h_M) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_set_allocations: null handle");
    const char* bad = alloc_bad_list(n_alloc, h_start, h_M, nullptr, false);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_set_allocations: %s", bad);
    return alloc_set_replace(h, n_alloc, h_start, h_M, nullptr);
}

int ofdm_rx_reserve_despread_alloc(ofdm_rx* h, int64_t n_seg) {
    const char* who = "ofdm_rx_reserve_despread_alloc";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (n_seg < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (h->alloc.n == 0) return fail(OFDM_ERR_INVALID, "%s: no allocation set (ofdm_rx_set_allocations)", who);
    if (n_seg > DFT_MAX_GROUPS / h->alloc.n) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(dft_alloc_prepare());
    const int64_t entries = h->alloc.n * n_seg;
    if (entries > h->cap_da_tab) {
        const int rc = regrow(h, {{&h->cap_da_tab, entries}}, ws_buf(&h->da_tab, size_t(entries)));
        if (rc != OFDM_OK) return rc;
    }
    if (n_seg <= h->cap_da_seg) return OFDM_OK;
    return regrow(h, {{&h->cap_da_seg, n_seg}}, ws_buf(&h->da_a, size_t(n_seg) * h->dev.Kd));
}

int ofdm_dft_despread_alloc_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int64_t row_len, int64_t seg_stride,
                                   const float* d_csi, int64_t csi_stride, float rho, int32_t noise_mode, double noise_var,
                                   const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    const char* who = "ofdm_dft_despread_alloc_frames";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const char* bad = despread_alloc_bad_args(h->alloc, d_sym, n_seg, rows, row_len, seg_stride, d_csi != nullptr, csi_stride, rho, noise_mode,
                                              noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "%s: null d_sym", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = despread_alloc_ensure(h, n_seg, false, s, who);
    if (rc != OFDM_OK) return rc;
    return despread_alloc_launch(h, d_sym, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, noise_mode, noise_var, d_sigma2,
                                 bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_despread_alloc(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                            float* d_eq, int32_t* d_tsr, int32_t noise_mode, double noise_var, const double* d_sigma2,
                                            int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_despread_alloc";
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    if (!d_eq) return fail(OFDM_ERR_INVALID, "%s: the despreading stage needs d_eq (it reads it)", who);
    const RxDev& d = h->dev;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, n_frames, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad)
        bad = despread_alloc_bad_args(h->alloc, d_eq, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, true, d.Kd, d.inv_snr_data, noise_mode, noise_var,
                                      d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = n_frames > 0 && n_dsym > 0;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = despread_alloc_ensure(h, n_frames, true, s, who);
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, n_frames, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !run) return r;
    HIP_TRY(launch_csi_frames(h->f_H, d.nfft, d.Kd, nullptr, d.Kd, n_frames, h->da_a, d.Kd, s));
    const int rc = despread_alloc_launch(h, d_eq, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, h->da_a, d.Kd, d.inv_snr_data, noise_mode, noise_var,
                                         d_sigma2, bits_mode, out, s);
    return rc != OFDM_OK ? rc : r;
}

int ofdm_tx_dft_spread_alloc(ofdm_tx* h, const float* d_sym, int64_t n_rows, int64_t row_len, float* d_out, void* stream) {
    const char* who = "ofdm_tx_dft_spread_alloc";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const DftAllocSet& A = h->alloc;
    if (A.n == 0) return fail(OFDM_ERR_INVALID, "%s: no allocation set (ofdm_tx_set_allocations)", who);
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (row_len < A.max_end) return fail(OFDM_ERR_INVALID, "%s: row_len < max(start + M) of the allocation set", who);
    if (row_len > SOFT_MAX_ROW || n_rows > SOFT_MAX_LEN / row_len || n_rows > DFT_MAX_GROUPS / (2 * A.n))
        return fail(OFDM_ERR_INVALID, "%s: index range exceeded", who);
    if (n_rows == 0) return OFDM_OK;
    if (!d_sym || !d_out) return fail(OFDM_ERR_INVALID, "%s: null d_sym or d_out", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    DftAllocRowsArgs a{};
    a.set = A.d_set;
    a.in = reinterpret_cast<const cf*>(d_sym);
    a.out = reinterpret_cast<cf*>(d_out);
    a.n_rows = n_rows;
    a.row_len = row_len;
    a.n_gap = A.n_gap;
    for (int g = 0; g < A.n_gap; ++g) {
        a.gap_start[g] = A.gap_start[g];
        a.gap_len[g] = A.gap_len[g];
    }
    if (row_len > A.max_end) {                              // the run behind the last allocation
        a.gap_start[a.n_gap] = A.max_end;
        a.gap_len[a.n_gap++] = int(row_len - A.max_end);
    }
    HIP_TRY(launch_dft_alloc_rows(a, A.h, A.n, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tx_reserve_spread_alloc(ofdm_tx* h, int64_t n_rows) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread_alloc: null handle");
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread_alloc: negative count");
    if (n_rows > INT32_MAX) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread_alloc: batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(dft_alloc_prepare());
    return tx_alloc_ws(h, n_rows);
}

int64_t ofdm_tx_modulate_frames_alloc(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                                      float* d_iq, int64_t frame_stride, void* stream) {
    const char* who = "ofdm_tx_modulate_frames_alloc";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (n_frames < 0 || n_sym < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (!bits_mode_ok(bits_mode)) return fail(OFDM_ERR_INVALID, "%s: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED", who);
    const TxDev& d = h->dev;
    const int SD = d.S + d.D;
    if (n_sym % SD != 0) return fail(OFDM_ERR_INVALID, "%s: n_sym must be a multiple of S + D = %d", who, SD);
    if (frame_stride != int64_t(n_sym) * d.L) return fail(OFDM_ERR_INVALID, "%s: frame_stride must equal n_sym*(nfft+cp)", who);
    if (h->alloc.n == 0) return fail(OFDM_ERR_INVALID, "%s: no allocation set (ofdm_tx_set_allocations)", who);
    if (h->alloc.max_end > d.Kd) return fail(OFDM_ERR_INVALID, "%s: the allocation set does not fit num_data_bins=%d", who, d.Kd);
    if (n_frames * int64_t(n_sym) > INT32_MAX) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    const int64_t data_per_frame = int64_t(n_sym / SD) * d.D, rows = n_frames * data_per_frame;
    const int64_t bits_per_frame = data_per_frame * d.Kd * d.bps;
    if (bits_mode == OFDM_BITS_PACKED && (bits_per_frame & 7)) return fail(OFDM_ERR_INVALID, "%s: packed bits need a whole number of bytes per frame", who);
    if (rows == 0) return 0;
    if (!d_bits || !d_iq) return fail(OFDM_ERR_INVALID, "%s: null d_bits or d_iq", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (rows > h->cap_sp_rows) {
        int rc = refuse_growth_in_capture(pick_stream(h, stream), who, "ofdm_tx_reserve_spread_alloc");
        if (rc == OFDM_OK) rc = tx_alloc_ws(h, rows);
        if (rc != OFDM_OK) return rc;
    }
    float* sym = reinterpret_cast<float*>(h->sp_sym);
    float* grid = reinterpret_cast<float*>(h->sp_grid);
    float* time = reinterpret_cast<float*>(h->sp_time);
    int rc = ofdm_tx_map(h, d_bits, bits_mode, rows * d.Kd, sym, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_dft_spread_alloc(h, sym, rows, d.Kd, sym, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_grid(h, sym, rows, grid, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_ifft_cp(h, grid, rows, 1, 1, time, stream);
    if (rc != OFDM_OK) return rc;
    return ofdm_tx_mux(h, time, rows, d_iq, stream);
}

}  // extern "C"

// ---- receive diversity for multi-user allocations of DFT-spread OFDM (include/ofdm_mi355x.h, "receive diversity for multi-user
// allocations of DFT-spread OFDM"): the stage of 9.2.16 over the allocation set of 9.2.17.  The set is the
// handle's (ofdm_rx_set_allocations); the workspace is a group of its own and does not depend on the set.
namespace {

// what the arguments and the set decide (no device access); "" = fine.  First what the arguments alone decide, then the set.
const char* mrc_despread_alloc_bad_args(const DftAllocSet& A, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows,
                                        int64_t row_len, int64_t seg_stride, int64_t csi_stride, float rho, int32_t noise_mode,
                                        const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                        const ofdm_mrc_despread_out* out) {
    if (noise_mode == OFDM_MRC_NOISE_EST)
        return "OFDM_MRC_NOISE_EST is refused (a spread signal has no constellation points per bin): pass OFDM_MRC_NOISE_GIVEN or "
               "OFDM_MRC_NOISE_SEG";
    // the modulations are the set's: 2 stands in where the combiner's checks ask for one
    const char* bad = mrc_bad_args(n_branch, n_seg, rows, row_len, seg_stride, csi_stride, rho, 2, noise_mode, h_noise_var, d_sigma2, false);
    if (*bad) return bad;
    if (!mrc_despread_wanted(out)) return "out is NULL or holds no pointer";
    if (out->bits && !bits_mode_ok(bits_mode)) return "bits wanted: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    if (d_sym && (out->sym == d_sym || out->comb == d_sym)) return "out->sym or out->comb == d_sym is refused: the layouts differ";
    // every allocation of any set takes at least one workgroup per segment: this much of the grid's limit the arguments decide
    if (rows > 0 && n_seg > DFT_MAX_GROUPS) return "index range exceeded (more than 2^31 - 1 workgroups)";
    if (A.n == 0) return "no allocation set (ofdm_rx_set_allocations)";
    if (row_len < A.max_end) return "row_len < max(start + M) of the allocation set";
    int64_t groups = 0;
    for (int u = 0; u < A.n; ++u) {
        const DftPlan& pl = A.h[u].pl;
        if (out->bits && bits_mode == OFDM_BITS_PACKED && (int64_t(pl.M) * A.h[u].mod) % 8 != 0)
            return "packed bits need M * bits per symbol % 8 == 0 of every allocation";
        if (!dft_rows_in_range(pl, rows, n_seg)) return "index range exceeded (more than 2^31 - 1 workgroups)";
        groups += n_seg * ((rows + pl.rows_per_group - 1) / pl.rows_per_group);     // each term fits (checked above)
        if (groups > DFT_MAX_GROUPS) return "index range exceeded (more than 2^31 - 1 workgroups)";
    }
    return "";
}
int mrc_despread_alloc_ensure(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t row_len, bool composite, hipStream_t s,
                              const char* who) {
    const int64_t units = n_branch * n_seg;
    if (units * row_len <= h->cap_ma_tab && (!composite || units * h->dev.Kd <= h->cap_ma_a)) return OFDM_OK;
    const int rc = refuse_growth_in_capture(s, who, "ofdm_rx_reserve_mrc_despread_alloc");
    return rc != OFDM_OK ? rc : ofdm_rx_reserve_mrc_despread_alloc(h, n_branch, n_seg, row_len);
}
// d_sigma2 == null: the host array (OFDM_MRC_NOISE_GIVEN)
int mrc_despread_alloc_launch(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len,
                              int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, const double* h_noise_var,
                              const double* d_sigma2, int32_t bits_mode, const ofdm_mrc_despread_out* out, hipStream_t s) {
    MrcArgs t{};                                            // the table over the whole rows: gaps are computed and never read
    t.n_branch = n_branch;
    t.n_seg = n_seg;
    t.rows = rows;
    t.seg_stride = seg_stride;
    t.row_len = int(row_len);
    t.seg_len = rows * row_len;
    t.csi = d_csi;
    t.csi_stride = csi_stride;
    t.rho = rho;
    t.mod = 2;                                              // not read by the table
    t.sigma2 = d_sigma2;
    for (int b = 0; b < MRC_MAX_BRANCHES; ++b) t.noise_var[b] = (!d_sigma2 && b < n_branch) ? h_noise_var[b] : 0.0;
    t.tab = h->ma_tab;
    HIP_TRY(launch_mrc_table(t, s));
    MrcDespreadAllocArgs a{};
    a.set = h->alloc.d_set;
    a.n_alloc = h->alloc.n;
    a.sym = reinterpret_cast<const cf*>(d_sym);
    a.n_branch = n_branch;
    a.n_seg = n_seg;
    a.rows = rows;
    a.row_len = row_len;
    a.seg_stride = seg_stride;
    a.tab = h->ma_tab;
    a.bits_mode = bits_mode;
    a.osym = reinterpret_cast<cf*>(out->sym);
    a.llr = out->llr;
    a.bits = out->bits;
    a.beta = out->beta;
    a.weight = out->weight;
    a.comb = reinterpret_cast<cf*>(out->comb);
    HIP_TRY(launch_mrc_despread_alloc(a, h->alloc.h, s));
    return OFDM_OK;
}

}  // namespace

extern "C" {

int ofdm_rx_reserve_mrc_despread_alloc(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t row_len) {
    const char* who = "ofdm_rx_reserve_mrc_despread_alloc";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (n_branch < 1 || n_branch > OFDM_MRC_MAX_BRANCHES) return fail(OFDM_ERR_INVALID, "%s: n_branch must lie in 1 .. OFDM_MRC_MAX_BRANCHES", who);
    if (n_seg < 0 || row_len < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (n_seg > SOFT_MAX_N / n_branch || row_len > SOFT_MAX_ROW) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    const int64_t units = n_branch * n_seg;
    if (units > 0 && (row_len > SOFT_MAX_LEN / units || h->dev.Kd > SOFT_MAX_LEN / units))
        return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(mrc_despread_alloc_prepare());
    if (units * row_len > h->cap_ma_tab) {
        const int rc = regrow(h, {{&h->cap_ma_tab, units * row_len}}, ws_buf(&h->ma_tab, size_t(units * row_len)));
        if (rc != OFDM_OK) return rc;
    }
    const int64_t floats = units * h->dev.Kd;
    if (floats <= h->cap_ma_a) return OFDM_OK;
    return regrow(h, {{&h->cap_ma_a, floats}}, ws_buf(&h->ma_a, size_t(floats)));
}

int ofdm_combine_despread_alloc_frames(ofdm_rx* h, const float* d_sym, int32_t n_branch, int64_t n_seg, int64_t rows, int64_t row_len,
                                       int64_t seg_stride, const float* d_csi, int64_t csi_stride, float rho, int32_t noise_mode,
                                       const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                       const ofdm_mrc_despread_out* out, void* stream) {
    const char* who = "ofdm_combine_despread_alloc_frames";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (!d_csi) return fail(OFDM_ERR_INVALID, "%s: d_csi is required (the combiner has no meaning without it)", who);
    const char* bad = mrc_despread_alloc_bad_args(h->alloc, d_sym, n_branch, n_seg, rows, row_len, seg_stride, csi_stride, rho, noise_mode,
                                                  h_noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "%s: null d_sym", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = mrc_despread_alloc_ensure(h, n_branch, n_seg, row_len, false, s, who);
    if (rc != OFDM_OK) return rc;
    return mrc_despread_alloc_launch(h, d_sym, n_branch, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho, h_noise_var,
                                     noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_mrc_despread_alloc(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                                int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode,
                                                const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                                const ofdm_mrc_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_mrc_despread_alloc";
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    if (n_branch < 1 || n_branch > OFDM_MRC_MAX_BRANCHES)
        return fail(OFDM_ERR_INVALID, "%s: n_branch must lie in 1 .. OFDM_MRC_MAX_BRANCHES", who);
    if (n_frames > SOFT_MAX_N / n_branch) return fail(OFDM_ERR_INVALID, "%s: batch too large (n_branch * n_frames > 2^31)", who);
    if (!d_eq) return fail(OFDM_ERR_INVALID, "%s: the stage needs d_eq (it reads it)", who);
    const RxDev& d = h->dev;
    const int64_t units = n_branch * n_frames;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    // the checks of the stages, made here first so that a bad call enqueues nothing
    const char* bad = demod_bad_args(d, units, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad)
        bad = mrc_despread_alloc_bad_args(h->alloc, d_eq, n_branch, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, d.Kd, d.inv_snr_data, noise_mode,
                                          h_noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = n_frames > 0 && n_dsym > 0;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = mrc_despread_alloc_ensure(h, n_branch, n_frames, d.Kd, true, s, who);
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, units, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !run) return r;
    HIP_TRY(launch_csi_frames(h->f_H, d.nfft, d.Kd, nullptr, d.Kd, units, h->ma_a, d.Kd, s));
    const int rc = mrc_despread_alloc_launch(h, d_eq, n_branch, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, h->ma_a, d.Kd, d.inv_snr_data,
                                             h_noise_var, noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
    return rc != OFDM_OK ? rc : r;
}

}  // extern "C"
