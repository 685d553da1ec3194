// capi_dft_tx.hip -- the transmitter of DFT-spread OFDM on its handle: the transform precoder of one size
// (include/ofdm_mi355x.h, "DFT-spread OFDM") and of the handle's allocation set ("multi-user allocations of
// DFT-spread OFDM"), each with its reserve call and its composite transmitter.  The plan cache and the set
// itself are in capi_dft.hip.
#include "capi_dft.hpp"

namespace {

// the rows between the stages of the composite transmitters, grown
int tx_spread_ws(ofdm_tx* h, int64_t n_rows) {
    if (n_rows <= h->cap_sp_rows) return OFDM_OK;
    const TxDev& d = h->dev;
    return regrow(h, {{&h->cap_sp_rows, n_rows}}, ws_buf(&h->sp_sym, size_t(n_rows) * d.Kd), ws_buf(&h->sp_grid, size_t(n_rows) * d.nfft),
                  ws_buf(&h->sp_time, size_t(n_rows) * d.L));
}
int tx_spread_ensure(ofdm_tx* h, int32_t M, int64_t ws_rows, hipStream_t s, const char* who, int* slot) {
    return dft_plan_ensure(h->dft, M, ws_rows <= h->cap_sp_rows, s, who, "ofdm_tx_reserve_spread",
                           [&] { return ofdm_tx_reserve_spread(h, M, ws_rows); }, slot);
}
// The composite transmitters: map, spread, grid, IFFT + CP, mux over the handle's rows.  set_bad(): the call's own refusal of
// what the handle holds (it has set the error text), or OFDM_OK; grow(rows, s): its plan, and the rows; spread(sym, rows).
template <class SetBad, class Grow, class Spread>
int64_t tx_modulate_spread(ofdm_tx* h, const char* who, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                           float* d_iq, int64_t frame_stride, void* stream, SetBad set_bad, Grow grow, Spread spread) {
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    if (n_frames < 0 || n_sym < 0) return fail(OFDM_ERR_INVALID, "%s: negative count", who);
    if (!bits_mode_ok(bits_mode)) return fail(OFDM_ERR_INVALID, "%s: bits_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED", who);
    const TxDev& d = h->dev;
    const int SD = d.S + d.D;
    if (n_sym % SD != 0) return fail(OFDM_ERR_INVALID, "%s: n_sym must be a multiple of S + D = %d", who, SD);
    if (frame_stride != int64_t(n_sym) * d.L) return fail(OFDM_ERR_INVALID, "%s: frame_stride must equal n_sym*(nfft+cp)", who);
    if (const int rc = set_bad()) return rc;
    if (n_frames * int64_t(n_sym) > INT32_MAX) return fail(OFDM_ERR_INVALID, "%s: batch too large", who);
    const int64_t data_per_frame = int64_t(n_sym / SD) * d.D, rows = n_frames * data_per_frame;
    const int64_t bits_per_frame = data_per_frame * d.Kd * d.bps;
    if (bits_mode == OFDM_BITS_PACKED && (bits_per_frame & 7)) return fail(OFDM_ERR_INVALID, "%s: packed bits need a whole number of bytes per frame", who);
    if (rows == 0) return 0;
    if (!d_bits || !d_iq) return fail(OFDM_ERR_INVALID, "%s: null d_bits or d_iq", who);
    HIP_TRY(hipSetDevice(h->cfg.device));
    int rc = grow(rows, pick_stream(h, stream));
    if (rc != OFDM_OK) return rc;
    float* sym = reinterpret_cast<float*>(h->sp_sym);
    float* grid = reinterpret_cast<float*>(h->sp_grid);
    float* time = reinterpret_cast<float*>(h->sp_time);
    rc = ofdm_tx_map(h, d_bits, bits_mode, rows * d.Kd, sym, stream);
    if (rc == OFDM_OK) rc = spread(sym, rows);
    if (rc == OFDM_OK) rc = ofdm_tx_grid(h, sym, rows, grid, stream);
    if (rc == OFDM_OK) rc = ofdm_tx_ifft_cp(h, grid, rows, 1, 1, time, stream);
    if (rc != OFDM_OK) return rc;
    return ofdm_tx_mux(h, time, rows, d_iq, stream);
}

}  // namespace

extern "C" {

int ofdm_tx_reserve_spread(ofdm_tx* h, int32_t M, int64_t n_rows) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: null handle");
    if (*dft_bad_size(M)) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: %s", dft_bad_size(M));
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: negative count");
    if (n_rows > INT32_MAX) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread: batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    int slot = -1;
    const int rc = dft_plan_get(h, M, &slot);
    return rc != OFDM_OK ? rc : tx_spread_ws(h, n_rows);
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
    return tx_modulate_spread(
        h, who, d_bits, bits_mode, n_frames, n_sym, d_iq, frame_stride, stream,
        [&] {
            const int Kd = h->dev.Kd;
            return *dft_bad_size(Kd) ? fail(OFDM_ERR_INVALID, "%s: num_data_bins=%d: %s", who, Kd, dft_bad_size(Kd)) : OFDM_OK;
        },
        [&](int64_t rows, hipStream_t s) {
            int slot = -1;
            return tx_spread_ensure(h, h->dev.Kd, rows, s, who, &slot);
        },
        [&](float* sym, int64_t rows) { return ofdm_tx_dft_spread(h, sym, rows, h->dev.Kd, sym, stream); });
}

int ofdm_tx_reserve_spread_alloc(ofdm_tx* h, int64_t n_rows) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread_alloc: null handle");
    if (n_rows < 0) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread_alloc: negative count");
    if (n_rows > INT32_MAX) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_spread_alloc: batch too large");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(dft_alloc_prepare());
    return tx_spread_ws(h, n_rows);
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

int64_t ofdm_tx_modulate_frames_alloc(ofdm_tx* h, const uint8_t* d_bits, int32_t bits_mode, int64_t n_frames, int32_t n_sym,
                                      float* d_iq, int64_t frame_stride, void* stream) {
    const char* who = "ofdm_tx_modulate_frames_alloc";
    return tx_modulate_spread(
        h, who, d_bits, bits_mode, n_frames, n_sym, d_iq, frame_stride, stream,
        [&] {
            if (h->alloc.n == 0) return fail(OFDM_ERR_INVALID, "%s: no allocation set (ofdm_tx_set_allocations)", who);
            const int Kd = h->dev.Kd;
            return h->alloc.max_end > Kd ? fail(OFDM_ERR_INVALID, "%s: the allocation set does not fit num_data_bins=%d", who, Kd) : OFDM_OK;
        },
        [&](int64_t rows, hipStream_t s) {                  // the buffers of ofdm_tx_reserve_spread, grown without a plan
            return grow_outside_capture(rows <= h->cap_sp_rows, s, who, "ofdm_tx_reserve_spread_alloc", [&] { return tx_spread_ws(h, rows); });
        },
        [&](float* sym, int64_t rows) { return ofdm_tx_dft_spread_alloc(h, sym, rows, h->dev.Kd, sym, stream); });
}

}  // extern "C"
