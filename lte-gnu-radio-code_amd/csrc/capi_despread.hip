// capi_despread.hip -- the receiver of DFT-spread OFDM on its handle, four families of one shape -- a reserve call, the stage on
// any device buffer, and the composite call that chains it behind ofdm_rx_demod_frames and the |H|^2 rows: despreading one size
// (include/ofdm_mi355x.h, "DFT-spread OFDM"), B receive branches combined before the transform ("receive
// diversity for DFT-spread OFDM"; 9.2.16), the handle's allocation set walked ("multi-user allocations of DFT-spread OFDM";
// 9.2.17), and B branches combined per allocation of that set ("receive diversity for multi-user allocations"; 9.2.18).  The
// plan cache and the set are in capi_dft.hip, the combiner's checks and table arguments in capi_mrc.hip.  The order in which
// each call refuses is its own, and pinned: tests/despread_refusal_cases.py.
#include <type_traits>

#include "capi_dft.hpp"

namespace {

// The rows a stage works on, as every stage call takes them: n_seg segments (combining: per branch) of `rows` rows of `len`
// entries -- M, or the row_len of the per-set stages -- with the channel powers of a row's entries.
struct Rows {
    const float* sym;
    int64_t n_seg, rows, len, seg_stride;
    const float* csi;
    int64_t csi_stride;
    float rho;
};
// the rows of a composite call: what ofdm_rx_demod_frames left in d_eq, with the |H|^2 rows of its frames
Rows frame_rows(const RxDev& d, const float* d_eq, int64_t n_frames, int64_t n_dsym, const float* csi) {
    return {d_eq, n_frames, n_dsym, d.Kd, n_dsym * d.Kd, csi, d.Kd, d.inv_snr_data};
}

// ---- the refusals more than one family makes; "" = fine
constexpr const char* TOO_MANY_GROUPS = "index range exceeded (more than 2^31 - 1 workgroups)";
constexpr const char* NOTHING_WANTED = "out is NULL or holds no pointer";
bool wanted(const ofdm_despread_out* o) { return o && (o->sym || o->llr || o->bits || o->beta || o->weight); }
bool wanted(const ofdm_mrc_despread_out* o) { return o && (o->sym || o->llr || o->bits || o->beta || o->weight || o->comb); }
// hard bits, where wanted, need a mode, and packed ones whole bytes per row of M symbols (M = 0: the sizes are a set's, asked below)
const char* bad_bits(const uint8_t* bits, int32_t bits_mode, int32_t M, int32_t modulation,
                     const char* not_whole = "packed bits need M * bits per symbol % 8 == 0") {
    if (!bits) return "";
    if (!bits_mode_ok(bits_mode)) return "bits wanted: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    return bits_mode == OFDM_BITS_PACKED && (int64_t(M) * modulation) % 8 != 0 ? not_whole : "";
}
const char* bad_est(int32_t noise_mode) {
    return noise_mode != OFDM_MRC_NOISE_EST ? ""
                                            : "OFDM_MRC_NOISE_EST is refused (a spread signal has no constellation points per bin): pass "
                                              "OFDM_MRC_NOISE_GIVEN or OFDM_MRC_NOISE_SEG";
}
// the workgroups of a set, one allocation after the other: false once their sum is beyond the grid (each term fits: checked before)
bool groups_fit(int64_t& groups, const DftPlan& pl, const Rows& r) {
    groups += r.n_seg * ((r.rows + pl.rows_per_group - 1) / pl.rows_per_group);
    return groups <= DFT_MAX_GROUPS;
}
// the opening of the composite calls that combine branches: that of the others, then the branches and the units
int mrc_stage_open(const ofdm_rx* h, bool bufs, int32_t n_branch, int64_t n_frames, int64_t frame_stride, int64_t frame_len, const char* who) {
    const int open = demod_stage_open(h, bufs, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    if (*mrc_bad_branches(n_branch)) return fail(OFDM_ERR_INVALID, "%s: %s", who, mrc_bad_branches(n_branch));
    if (n_frames > SOFT_MAX_N / n_branch) return fail(OFDM_ERR_INVALID, "%s: batch too large (n_branch * n_frames > 2^31)", who);
    return OFDM_OK;
}

// the fields the argument structs of the four launches share
template <class Args, class Out>
void stage_fill(Args& a, const Rows& r, int32_t bits_mode, const Out* out) {
    a.sym = reinterpret_cast<const cf*>(r.sym);
    a.n_seg = r.n_seg;
    a.rows = r.rows;
    a.seg_stride = r.seg_stride;
    a.bits_mode = bits_mode;
    a.osym = reinterpret_cast<cf*>(out->sym);
    a.llr = out->llr;
    a.bits = out->bits;
    a.beta = out->beta;
    a.weight = out->weight;
    if constexpr (std::is_same_v<Out, ofdm_mrc_despread_out>) a.comb = reinterpret_cast<cf*>(out->comb);
}
// ... and those of the two that take their noise per segment
template <class Args>
void noise_fill(Args& a, const Rows& r, int32_t noise_mode, double noise_var, const double* d_sigma2) {
    a.csi = r.csi;
    a.csi_stride = r.csi_stride;
    a.rho = r.rho;
    a.noise_mode = noise_mode;
    a.noise_var = noise_var;
    a.sigma2 = d_sigma2;
}
// the combiner's {c, t} table over the units of r into `tab`; d_sigma2 == null: the host array (OFDM_MRC_NOISE_GIVEN)
hipError_t mrc_table(const Rows& r, int32_t n_branch, int32_t modulation, const double* h_noise_var, const double* d_sigma2, float2* tab,
                     hipStream_t s) {
    return launch_mrc_table(mrc_table_args(n_branch, r.n_seg, r.rows, r.len, r.seg_stride, r.csi, r.csi_stride, r.rho, modulation,
                                           h_noise_var, d_sigma2, tab), s);
}

// The composite calls behind their opening: d_eq, the checks of both stages (made here first so that a bad call enqueues
// nothing), ofdm_rx_demod_frames over the units (n_frames, or n_branch * n_frames), their |H|^2 rows, the family's stage.
// needs: who needs d_eq; bad_args(d, n_dsym): the stage's refusal; ensure(s): its plan and workspace; csi(): the family's
// |H|^2 rows -- asked behind ensure, which frees and reallocates them; launch(n_dsym, rows, s).
template <class Bad, class Ensure, class Csi, class Launch>
int64_t demod_then_stage(ofdm_rx* h, const char* who, const char* needs, const float* d_iq, int64_t n_frames, int64_t units,
                         int64_t frame_stride, int64_t frame_len, float* d_eq, int32_t* d_tsr, void* stream, Bad bad_args, Ensure ensure,
                         Csi csi, Launch launch) {
    if (!d_eq) return fail(OFDM_ERR_INVALID, "%s: %s needs d_eq (it reads it)", who, needs);
    const RxDev& d = h->dev;
    const int64_t n_dsym = frame_data_symbols(d, frame_len);
    const char* bad = demod_bad_args(d, units, n_dsym, nullptr, OFDM_BITS_NONE);
    if (!*bad) bad = bad_args(d, n_dsym);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    hipStream_t s = pick_stream(h, stream);
    const bool run = n_frames > 0 && n_dsym > 0;
    if (run) {                                              // grow first: nothing is enqueued unless the whole call can run
        HIP_TRY(hipSetDevice(h->cfg.device));
        const int rc = ensure(s);
        if (rc != OFDM_OK) return rc;
    }
    const int64_t r = ofdm_rx_demod_frames(h, d_iq, units, frame_stride, frame_len, d_eq, nullptr, OFDM_BITS_NONE, d_tsr, stream);
    if (r < 0 || !run) return r;
    float* a = csi();
    HIP_TRY(launch_csi_frames(h->f_H, d.nfft, d.Kd, nullptr, d.Kd, units, a, d.Kd, s));
    const int rc = launch(n_dsym, a, s);
    return rc != OFDM_OK ? rc : r;
}

// ---- one size
// what the arguments alone decide (no read of the handle, no device access); "" = fine
const char* despread_bad_args(const Rows& r, bool has_csi, int32_t modulation, int32_t noise_mode, double noise_var,
                              const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out) {
    const int32_t M = int32_t(r.len);
    if (*dft_bad_size(M)) return dft_bad_size(M);
    if (r.n_seg < 0 || r.rows < 0) return "negative count";
    if (r.rows > SOFT_MAX_LEN / M) return "index range exceeded (rows * M)";
    if (r.seg_stride < r.rows * M) return "seg_stride < rows * M";
    if (!soft_mod_ok(modulation)) return "modulation must be 2, 4 or 6 bits per symbol (no BPSK soft metrics)";
    if (has_csi) {
        if (r.csi_stride < M) return "csi_stride < M";
        if (noise_mode != OFDM_DESPREAD_NOISE_RHO && noise_mode != OFDM_DESPREAD_NOISE_GIVEN && noise_mode != OFDM_DESPREAD_NOISE_SEG)
            return "noise_mode must be OFDM_DESPREAD_NOISE_RHO, OFDM_DESPREAD_NOISE_GIVEN or OFDM_DESPREAD_NOISE_SEG";
        if (noise_mode == OFDM_DESPREAD_NOISE_GIVEN && !(std::isfinite(noise_var) && noise_var > 0.0))
            return "OFDM_DESPREAD_NOISE_GIVEN needs a finite noise_var > 0";
        if (noise_mode == OFDM_DESPREAD_NOISE_SEG && !d_sigma2) return "OFDM_DESPREAD_NOISE_SEG needs d_sigma2";
        if (!(std::isfinite(r.rho) && r.rho >= 0.f)) return "rho must be finite and >= 0";
    }
    if (!wanted(out)) return NOTHING_WANTED;
    if (*bad_bits(out->bits, bits_mode, M, modulation)) return bad_bits(out->bits, bits_mode, M, modulation);
    if (out->sym && out->sym == r.sym && r.seg_stride != r.rows * M) return "out->sym == d_sym needs seg_stride == rows * M";
    if (r.n_seg > SOFT_MAX_N ||
        (r.n_seg > 0 && (r.seg_stride > SOFT_MAX_LEN / r.n_seg || (has_csi && r.csi_stride > SOFT_MAX_LEN / r.n_seg))))
        return "index range exceeded (batch beyond the kernels' index range)";
    DftPlan pl;
    dft_make_plan(M, pl);
    return dft_rows_in_range(pl, r.rows, r.n_seg) ? "" : TOO_MANY_GROUPS;
}
// the plan for M and the tables of n_seg segments (frames: also their |H|^2 rows), or a refusal inside a capture
int despread_ensure(ofdm_rx* h, int32_t M, int64_t n_seg, hipStream_t s, const char* who, int* slot) {
    return dft_plan_ensure(h->dft, M, n_seg <= h->cap_ds_seg, s, who, "ofdm_rx_reserve_despread",
                           [&] { return ofdm_rx_reserve_despread(h, M, n_seg); }, slot);
}
int despread_launch(ofdm_rx* h, int slot, const Rows& r, int32_t modulation, int32_t noise_mode, double noise_var,
                    const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out, hipStream_t s) {
    DespreadArgs a{};
    stage_fill(a, r, bits_mode, out);
    noise_fill(a, r, noise_mode, noise_var, d_sigma2);
    a.pl = h->dft.pl[slot];
    a.tw = h->dft.d_tw[slot];
    a.groups_per_seg = (r.rows + a.pl.rows_per_group - 1) / a.pl.rows_per_group;
    a.mod = modulation;
    a.tab = h->ds_tab;
    HIP_TRY(launch_despread(a, s));
    return OFDM_OK;
}

// ---- B branches combined before the transform
// what the arguments alone decide: what ofdm_combine_csi_frames and ofdm_dft_despread_frames refuse for the same argument; "" = fine
const char* mrc_despread_bad_args(const Rows& r, int32_t n_branch, int32_t modulation, int32_t noise_mode, const double* h_noise_var,
                                  const double* d_sigma2, int32_t bits_mode, const ofdm_mrc_despread_out* out) {
    const int32_t M = int32_t(r.len);
    if (*dft_bad_size(M)) return dft_bad_size(M);
    if (*bad_est(noise_mode)) return bad_est(noise_mode);
    const char* bad = mrc_bad_args(n_branch, r.n_seg, r.rows, M, r.seg_stride, r.csi_stride, r.rho, modulation, noise_mode, h_noise_var,
                                   d_sigma2, false);
    if (*bad) return bad;
    if (!wanted(out)) return NOTHING_WANTED;
    if (*bad_bits(out->bits, bits_mode, M, modulation)) return bad_bits(out->bits, bits_mode, M, modulation);
    DftPlan pl;
    dft_make_plan(M, pl);
    return dft_rows_in_range(pl, r.rows, r.n_seg) ? "" : TOO_MANY_GROUPS;
}
// the plan for M, the table of the units and (composite) their |H|^2 rows, or a refusal inside a capture
int mrc_despread_ensure(ofdm_rx* h, int32_t M, int32_t n_branch, int64_t n_seg, bool composite, hipStream_t s, const char* who,
                        int* slot) {
    const int64_t units = n_branch * n_seg;
    return dft_plan_ensure(h->dft, M, units * M <= h->cap_md_tab && (!composite || units <= h->cap_md_units), s, who,
                           "ofdm_rx_reserve_mrc_despread", [&] { return ofdm_rx_reserve_mrc_despread(h, M, n_branch, n_seg); }, slot);
}
// d_sigma2 == null: the host array (OFDM_MRC_NOISE_GIVEN)
int mrc_despread_launch(ofdm_rx* h, int slot, const Rows& r, int32_t n_branch, int32_t modulation, const double* h_noise_var,
                        const double* d_sigma2, int32_t bits_mode, const ofdm_mrc_despread_out* out, hipStream_t s) {
    HIP_TRY(mrc_table(r, n_branch, modulation, h_noise_var, d_sigma2, h->md_tab, s));
    MrcDespreadArgs a{};
    stage_fill(a, r, bits_mode, out);
    a.pl = h->dft.pl[slot];
    a.tw = h->dft.d_tw[slot];
    a.n_branch = n_branch;
    a.groups_per_seg = (r.rows + a.pl.rows_per_group - 1) / a.pl.rows_per_group;
    a.tab = h->md_tab;
    a.mod = modulation;
    HIP_TRY(launch_mrc_despread(a, s));
    return OFDM_OK;
}

// ---- the allocation set walked
// what the arguments and the set decide (no device access); "" = fine
const char* despread_alloc_bad_args(const DftAllocSet& A, const Rows& r, bool has_csi, int32_t noise_mode, double noise_var,
                                    const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out) {
    if (A.n == 0) return "no allocation set (ofdm_rx_set_allocations)";
    if (r.n_seg < 0 || r.rows < 0) return "negative count";
    if (r.len < A.max_end) return "row_len < max(start + M) of the allocation set";
    if (r.len > SOFT_MAX_ROW || r.rows > SOFT_MAX_LEN / r.len) return "index range exceeded (rows * row_len)";
    if (r.seg_stride < r.rows * r.len) return "seg_stride < rows * row_len";
    if (has_csi && r.csi_stride < r.len) return "csi_stride < row_len";
    if (out && out->sym && out->sym == r.sym) return "out->sym == d_sym is refused: the layouts differ";
    int64_t groups = 0;
    for (int u = 0; u < A.n; ++u) {
        Rows ru = r;
        ru.len = A.h[u].pl.M;
        const char* bad = despread_bad_args(ru, has_csi, A.h[u].mod, noise_mode, noise_var, d_sigma2, bits_mode, out);
        if (*bad) return bad;
        if (!groups_fit(groups, A.h[u].pl, r)) return TOO_MANY_GROUPS;
    }
    return r.n_seg > DFT_MAX_GROUPS / A.n ? TOO_MANY_GROUPS : "";
}
int despread_alloc_ensure(ofdm_rx* h, int64_t n_seg, bool composite, hipStream_t s, const char* who) {
    return grow_outside_capture(h->alloc.n * n_seg <= h->cap_da_tab && (!composite || n_seg <= h->cap_da_seg), s, who,
                                "ofdm_rx_reserve_despread_alloc", [&] { return ofdm_rx_reserve_despread_alloc(h, n_seg); });
}
int despread_alloc_launch(ofdm_rx* h, const Rows& r, int32_t noise_mode, double noise_var, const double* d_sigma2, int32_t bits_mode,
                          const ofdm_despread_out* out, hipStream_t s) {
    DespreadAllocArgs a{};
    stage_fill(a, r, bits_mode, out);
    noise_fill(a, r, noise_mode, noise_var, d_sigma2);
    a.set = h->alloc.d_set;
    a.n_alloc = h->alloc.n;
    a.row_len = r.len;
    a.tab = h->da_tab;
    HIP_TRY(launch_despread_alloc(a, h->alloc.h, s));
    return OFDM_OK;
}

// ---- B branches combined per allocation of the set: the stage of 9.2.16 over the set of 9.2.17.  The workspace is a group of
// its own and does not depend on the set.
// what the arguments and the set decide (no device access); "" = fine.  First what the arguments alone decide, then the set.
const char* mrc_despread_alloc_bad_args(const DftAllocSet& A, const Rows& r, int32_t n_branch, int32_t noise_mode,
                                        const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                        const ofdm_mrc_despread_out* out) {
    if (*bad_est(noise_mode)) return bad_est(noise_mode);
    // the modulations are the set's: 2 stands in where the combiner's checks ask for one
    const char* bad = mrc_bad_args(n_branch, r.n_seg, r.rows, r.len, r.seg_stride, r.csi_stride, r.rho, 2, noise_mode, h_noise_var, d_sigma2,
                                   false);
    if (*bad) return bad;
    if (!wanted(out)) return NOTHING_WANTED;
    if (*bad_bits(out->bits, bits_mode, 0, 0)) return bad_bits(out->bits, bits_mode, 0, 0);
    if (r.sym && (out->sym == r.sym || out->comb == r.sym)) return "out->sym or out->comb == d_sym is refused: the layouts differ";
    // every allocation of any set takes at least one workgroup per segment: this much of the grid's limit the arguments decide
    if (r.rows > 0 && r.n_seg > DFT_MAX_GROUPS) return TOO_MANY_GROUPS;
    if (A.n == 0) return "no allocation set (ofdm_rx_set_allocations)";
    if (r.len < A.max_end) return "row_len < max(start + M) of the allocation set";
    int64_t groups = 0;
    for (int u = 0; u < A.n; ++u) {
        const DftPlan& pl = A.h[u].pl;
        bad = bad_bits(out->bits, bits_mode, pl.M, A.h[u].mod, "packed bits need M * bits per symbol % 8 == 0 of every allocation");
        if (*bad) return bad;
        if (!dft_rows_in_range(pl, r.rows, r.n_seg) || !groups_fit(groups, pl, r)) return TOO_MANY_GROUPS;
    }
    return "";
}
int mrc_despread_alloc_ensure(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t row_len, bool composite, hipStream_t s,
                              const char* who) {
    const int64_t units = n_branch * n_seg;
    return grow_outside_capture(units * row_len <= h->cap_ma_tab && (!composite || units * h->dev.Kd <= h->cap_ma_a), s, who,
                                "ofdm_rx_reserve_mrc_despread_alloc",
                                [&] { return ofdm_rx_reserve_mrc_despread_alloc(h, n_branch, n_seg, row_len); });
}
// d_sigma2 == null: the host array (OFDM_MRC_NOISE_GIVEN)
int mrc_despread_alloc_launch(ofdm_rx* h, const Rows& r, int32_t n_branch, const double* h_noise_var, const double* d_sigma2,
                              int32_t bits_mode, const ofdm_mrc_despread_out* out, hipStream_t s) {
    // the table over the whole rows: gaps are computed and never read; the modulation is not read by the table
    HIP_TRY(mrc_table(r, n_branch, 2, h_noise_var, d_sigma2, h->ma_tab, s));
    MrcDespreadAllocArgs a{};
    stage_fill(a, r, bits_mode, out);
    a.set = h->alloc.d_set;
    a.n_alloc = h->alloc.n;
    a.n_branch = n_branch;
    a.row_len = r.len;
    a.tab = h->ma_tab;
    HIP_TRY(launch_mrc_despread_alloc(a, h->alloc.h, s));
    return OFDM_OK;
}

}  // namespace

extern "C" {

int ofdm_rx_reserve_despread(ofdm_rx* h, int32_t M, int64_t n_seg) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: null handle");
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: %s", dft_bad_size(M));
    if (n_seg < 0) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: negative count");
    if (n_seg > SOFT_MAX_N) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_despread: batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = -1;
    const int rc = dft_plan_get(h, M, &slot);
    if (rc != OFDM_OK || n_seg <= h->cap_ds_seg) return rc;
    return regrow(h, {{&h->cap_ds_seg, n_seg}}, ws_buf(&h->ds_tab, size_t(n_seg)), ws_buf(&h->ds_a, size_t(n_seg) * h->dev.Kd));
}

int ofdm_dft_despread_frames(ofdm_rx* h, const float* d_sym, int64_t n_seg, int64_t rows, int32_t M, int64_t seg_stride,
                             const float* d_csi, int64_t csi_stride, float rho, int32_t modulation, int32_t noise_mode,
                             double noise_var, const double* d_sigma2, int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    const char* who = "ofdm_dft_despread_frames";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    const Rows r{d_sym, n_seg, rows, M, seg_stride, d_csi, csi_stride, rho};
    const char* bad = despread_bad_args(r, d_csi != nullptr, modulation, noise_mode, noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "%s: null d_sym", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    int slot = -1;
    const int rc = despread_ensure(h, M, n_seg, s, who, &slot);
    if (rc != OFDM_OK) return rc;
    return despread_launch(h, slot, r, modulation, noise_mode, noise_var, d_sigma2, bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_despread(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                      float* d_eq, int32_t* d_tsr, int32_t noise_mode, double noise_var, const double* d_sigma2,
                                      int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_despread";
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    const int mod = h->cfg.modulation;
    int slot = -1;
    return demod_then_stage(
        h, who, "the despreading stage", d_iq, n_frames, n_frames, frame_stride, frame_len, d_eq, d_tsr, stream,
        [&](const RxDev& d, int64_t n_dsym) {
            return despread_bad_args(frame_rows(d, d_eq, n_frames, n_dsym, nullptr), true, mod, noise_mode, noise_var, d_sigma2, bits_mode, out);
        },
        [&](hipStream_t s) { return despread_ensure(h, h->dev.Kd, n_frames, s, who, &slot); }, [&] { return h->ds_a; },
        [&](int64_t n_dsym, const float* csi, hipStream_t s) {
            return despread_launch(h, slot, frame_rows(h->dev, d_eq, n_frames, n_dsym, csi), mod, noise_mode, noise_var, d_sigma2, bits_mode,
                                   out, s);
        });
}

int ofdm_rx_reserve_mrc_despread(ofdm_rx* h, int32_t M, int32_t n_branch, int64_t n_seg) {
    const char* who = "ofdm_rx_reserve_mrc_despread";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "%s: %s", who, dft_bad_size(M));
    if (*mrc_bad_branches(n_branch)) return fail(OFDM_ERR_INVALID, "%s: %s", who, mrc_bad_branches(n_branch));
    if (n_seg < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (n_seg > SOFT_MAX_N / n_branch) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = -1;
    int rc = dft_plan_get(h, M, &slot);
    if (rc != OFDM_OK) return rc;
    HIP_TRY(mrc_despread_prepare());
    const int64_t units = n_branch * n_seg;
    if (units * M > h->cap_md_tab) {
        rc = regrow(h, {{&h->cap_md_tab, units * M}}, ws_buf(&h->md_tab, size_t(units * M)));
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
    const Rows r{d_sym, n_seg, rows, M, seg_stride, d_csi, csi_stride, rho};
    const char* bad = mrc_despread_bad_args(r, n_branch, modulation, noise_mode, h_noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym || !d_csi) return fail(OFDM_ERR_INVALID, "%s: null d_sym or d_csi", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    int slot = -1;
    const int rc = mrc_despread_ensure(h, M, n_branch, n_seg, false, s, who, &slot);
    if (rc != OFDM_OK) return rc;
    return mrc_despread_launch(h, slot, r, n_branch, modulation, h_noise_var, noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr,
                               bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_mrc_despread(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                          int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode,
                                          const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                          const ofdm_mrc_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_mrc_despread";
    const int open = mrc_stage_open(h, d_iq != nullptr, n_branch, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    const int mod = h->cfg.modulation;
    int slot = -1;
    return demod_then_stage(
        h, who, "the stage", d_iq, n_frames, n_branch * n_frames, frame_stride, frame_len, d_eq, d_tsr, stream,
        [&](const RxDev& d, int64_t n_dsym) {
            return mrc_despread_bad_args(frame_rows(d, d_eq, n_frames, n_dsym, nullptr), n_branch, mod, noise_mode, h_noise_var, d_sigma2,
                                         bits_mode, out);
        },
        [&](hipStream_t s) { return mrc_despread_ensure(h, h->dev.Kd, n_branch, n_frames, true, s, who, &slot); }, [&] { return h->md_a; },
        [&](int64_t n_dsym, const float* csi, hipStream_t s) {
            return mrc_despread_launch(h, slot, frame_rows(h->dev, d_eq, n_frames, n_dsym, csi), n_branch, mod, h_noise_var,
                                       noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
        });
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
    const Rows r{d_sym, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho};
    const char* bad = despread_alloc_bad_args(h->alloc, r, d_csi != nullptr, noise_mode, noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "%s: null d_sym", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = despread_alloc_ensure(h, n_seg, false, s, who);
    if (rc != OFDM_OK) return rc;
    return despread_alloc_launch(h, r, noise_mode, noise_var, d_sigma2, bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_despread_alloc(ofdm_rx* h, const float* d_iq, int64_t n_frames, int64_t frame_stride, int64_t frame_len,
                                            float* d_eq, int32_t* d_tsr, int32_t noise_mode, double noise_var, const double* d_sigma2,
                                            int32_t bits_mode, const ofdm_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_despread_alloc";
    const int open = demod_stage_open(h, d_iq != nullptr, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    return demod_then_stage(
        h, who, "the despreading stage", d_iq, n_frames, n_frames, frame_stride, frame_len, d_eq, d_tsr, stream,
        [&](const RxDev& d, int64_t n_dsym) {
            return despread_alloc_bad_args(h->alloc, frame_rows(d, d_eq, n_frames, n_dsym, nullptr), true, noise_mode, noise_var, d_sigma2,
                                           bits_mode, out);
        },
        [&](hipStream_t s) { return despread_alloc_ensure(h, n_frames, true, s, who); }, [&] { return h->da_a; },
        [&](int64_t n_dsym, const float* csi, hipStream_t s) {
            return despread_alloc_launch(h, frame_rows(h->dev, d_eq, n_frames, n_dsym, csi), noise_mode, noise_var, d_sigma2, bits_mode, out, s);
        });
}

int ofdm_rx_reserve_mrc_despread_alloc(ofdm_rx* h, int32_t n_branch, int64_t n_seg, int64_t row_len) {
    const char* who = "ofdm_rx_reserve_mrc_despread_alloc";
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (*mrc_bad_branches(n_branch)) return fail(OFDM_ERR_INVALID, "%s: %s", who, mrc_bad_branches(n_branch));
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
    const Rows r{d_sym, n_seg, rows, row_len, seg_stride, d_csi, csi_stride, rho};
    const char* bad = mrc_despread_alloc_bad_args(h->alloc, r, n_branch, noise_mode, h_noise_var, d_sigma2, bits_mode, out);
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    if (n_seg == 0 || rows == 0) return OFDM_OK;
    if (!d_sym) return fail(OFDM_ERR_INVALID, "%s: null d_sym", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = pick_stream(h, stream);
    const int rc = mrc_despread_alloc_ensure(h, n_branch, n_seg, row_len, false, s, who);
    if (rc != OFDM_OK) return rc;
    return mrc_despread_alloc_launch(h, r, n_branch, h_noise_var, noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
}

int64_t ofdm_rx_demod_frames_mrc_despread_alloc(ofdm_rx* h, const float* d_iq, int32_t n_branch, int64_t n_frames, int64_t frame_stride,
                                                int64_t frame_len, float* d_eq, int32_t* d_tsr, int32_t noise_mode,
                                                const double* h_noise_var, const double* d_sigma2, int32_t bits_mode,
                                                const ofdm_mrc_despread_out* out, void* stream) {
    const char* who = "ofdm_rx_demod_frames_mrc_despread_alloc";
    const int open = mrc_stage_open(h, d_iq != nullptr, n_branch, n_frames, frame_stride, frame_len, who);
    if (open != OFDM_OK) return open;
    return demod_then_stage(
        h, who, "the stage", d_iq, n_frames, n_branch * n_frames, frame_stride, frame_len, d_eq, d_tsr, stream,
        [&](const RxDev& d, int64_t n_dsym) {
            return mrc_despread_alloc_bad_args(h->alloc, frame_rows(d, d_eq, n_frames, n_dsym, nullptr), n_branch, noise_mode, h_noise_var,
                                               d_sigma2, bits_mode, out);
        },
        [&](hipStream_t s) { return mrc_despread_alloc_ensure(h, n_branch, n_frames, h->dev.Kd, true, s, who); }, [&] { return h->ma_a; },
        [&](int64_t n_dsym, const float* csi, hipStream_t s) {
            return mrc_despread_alloc_launch(h, frame_rows(h->dev, d_eq, n_frames, n_dsym, csi), n_branch, h_noise_var,
                                             noise_mode == OFDM_MRC_NOISE_SEG ? d_sigma2 : nullptr, bits_mode, out, s);
        });
}

}  // extern "C"
