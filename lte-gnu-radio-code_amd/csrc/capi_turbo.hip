// capi_turbo.hip -- the LTE turbo code on the frame-batched path (definition: include/ofdm_mi355x.h): the
// host-only block count and interleaver check, the encode call of the transmitter handle, reserve and decode of the receiver handle.
// Behind them the same for its rate matching: block count and geometry on the host, the rate-matching encoder,
// the de-matching call and the two reserve calls.
#include "capi_internal.hpp"

namespace {
constexpr const char* TURBO_BAD_K = "K must be a multiple of 8 with 40 <= K <= 6144";
// K, the counts and the interleaver, in the order the calls report them; "" = fine.  The permutation check is O(K) host work.
const char* turbo_bad_geometry(int64_t n_seg, int64_t blocks_per_seg, int64_t K, int64_t f1, int64_t f2) {
    if (!turbo_valid_k(K)) return TURBO_BAD_K;
    if (n_seg < 0 || blocks_per_seg < 0) return "negative count";
    if (n_seg > MAX_BLOCKS || blocks_per_seg > MAX_BLOCKS || (blocks_per_seg > 0 && n_seg > MAX_BLOCKS / blocks_per_seg))
        return "batch beyond the kernels' index range";
    if (f1 < 0 || f1 >= K || f2 < 0 || f2 >= K) return "f1 and f2 must lie in 0 .. K-1";
    if (!turbo_qpp_valid(K, f1, f2)) return "(f1 i + f2 i^2) mod K is not a permutation of 0 .. K-1";
    return "";
}
// the rate-matching geometry on top of K: Ncb (0 = Kw) and E against the buffer's non-NULL entries; "" = fine
constexpr const char* TURBO_RM_BAD_NCB = "Ncb must be 0 or lie in Kpi .. 3 Kpi, Kpi = 32 ceil((K + 4) / 32)";
bool turbo_rm_ncb_ok(int32_t K, int64_t Ncb) { return Ncb == 0 || (Ncb >= turbo_rm_kpi(K) && Ncb <= 3 * turbo_rm_kpi(K)); }
const char* turbo_rm_bad_geometry(int32_t K, int64_t E, int64_t Ncb, int32_t rv, const int32_t* d_rv) {
    if (!turbo_rm_ncb_ok(K, Ncb)) return TURBO_RM_BAD_NCB;
    if (E < 1 || E > int64_t(TURBO_RM_MAX_COPIES) * turbo_rm_geom(K, 1, int(Ncb)).navail) return "E must lie in 1 .. 16 Navail";
    if (!d_rv && (rv < 0 || rv > 3)) return "rv must lie in 0 .. 3";
    return "";
}
bool turbo_wanted(const ofdm_turbo_out* o) { return o && (o->bits || o->llr); }
constexpr const char* TURBO_SHORT_STRIDE = "seg_stride < blocks_per_seg * (3K + 12)";
// both decoders share the handle's workspace: it holds `need` floats afterwards, and only grows
int turbo_grow(ofdm_rx* h, int64_t need) {
    if (need <= h->cap_turbo) return OFDM_OK;
    return regrow(h, {{&h->cap_turbo, need}}, ws_buf(&h->t_ws, size_t(need)));
}
const char* turbo_bad_reserve(int64_t n_blocks, int32_t K) {
    if (!turbo_valid_k(K)) return TURBO_BAD_K;
    if (n_blocks < 0) return "negative count";
    if (n_blocks > MAX_BLOCKS) return "batch beyond the kernel's index range";
    return "";
}
bool turbo_es_wanted(const ofdm_turbo_es_out* o) { return o && (o->bits || o->llr || o->iters || o->crc_ok); }
}  // namespace

extern "C" {

int64_t ofdm_turbo_blocks(int64_t seg_bits, int32_t K) {
    if (!turbo_valid_k(K)) return fail(OFDM_ERR_INVALID, "ofdm_turbo_blocks: %s", TURBO_BAD_K);
    if (seg_bits < 0) return fail(OFDM_ERR_INVALID, "ofdm_turbo_blocks: negative seg_bits");
    return seg_bits / (3 * int64_t(K) + 12);
}

int ofdm_turbo_qpp_check(int32_t K, int32_t f1, int32_t f2) {
    const char* bad = turbo_bad_geometry(0, 0, K, f1, f2);
    return *bad ? fail(OFDM_ERR_INVALID, "ofdm_turbo_qpp_check: %s", bad) : OFDM_OK;
}

int ofdm_tx_turbo_encode_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                                int32_t K, int32_t f1, int32_t f2, uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_turbo_encode_frames: null handle");
    const char* bad = turbo_bad_geometry(n_seg, blocks_per_seg, K, f1, f2);
    if (!*bad)
        bad = enc_bad_args(info_mode, coded_mode, n_seg, seg_bits, int64_t(blocks_per_seg) * (3 * int64_t(K) + 12),
                           "seg_bits < blocks_per_seg * (3K + 12)");
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_turbo_encode_frames: %s", bad);
    if (n_seg == 0 || seg_bits == 0) return OFDM_OK;
    if (!d_coded || (blocks_per_seg > 0 && !d_info)) return fail(OFDM_ERR_INVALID, "ofdm_tx_turbo_encode_frames: null buffer");
    TurboEncArgs a{};
    enc_fill(a, d_info, info_mode, n_seg, blocks_per_seg, d_coded, coded_mode, seg_bits);
    a.q = turbo_qpp(K, f1, f2);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_turbo_encode(a, pick_stream(h, stream)));
    return OFDM_OK;
}

// Sizes the workspace for n_blocks blocks of K bits (it only grows) and loads the decoder's code object.  Growing waits for
// the device, so it cannot happen inside a capture: ofdm_turbo_decode_frames refuses there and names this call.
int ofdm_rx_reserve_turbo(ofdm_rx* h, int64_t n_blocks, int32_t K) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_turbo: null handle");
    const char* bad = turbo_bad_reserve(n_blocks, K);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_turbo: %s", bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(turbo_decode_prepare());
    return turbo_grow(h, turbo_ws_floats(n_blocks, K));
}

int ofdm_turbo_decode_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, int32_t K,
                             int32_t f1, int32_t f2, int32_t n_iter, const ofdm_turbo_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_turbo_decode_frames: null handle");
    const char* bad = turbo_bad_geometry(n_seg, blocks_per_seg, K, f1, f2);
    if (!*bad) {
        if (n_iter < 1 || n_iter > TURBO_ITER_MAX) bad = "n_iter must lie in 1 .. 16";
        else bad = dec_bad_args(n_seg, seg_stride, int64_t(blocks_per_seg) * (3 * int64_t(K) + 12), TURBO_SHORT_STRIDE, out);
    }
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_turbo_decode_frames: %s", bad);
    if (n_seg == 0 || blocks_per_seg == 0 || !turbo_wanted(out)) return OFDM_OK;
    if (!d_llr) return fail(OFDM_ERR_INVALID, "ofdm_turbo_decode_frames: null d_llr");
    hipStream_t s = pick_stream(h, stream);
    const int64_t n_blocks = n_seg * blocks_per_seg;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int rc = grow_outside_capture(turbo_ws_floats(n_blocks, K) <= h->cap_turbo, s, "ofdm_turbo_decode_frames", "ofdm_rx_reserve_turbo",
                                        [&] { return ofdm_rx_reserve_turbo(h, n_blocks, K); });
    if (rc != OFDM_OK) return rc;
    TurboDecArgs a{};
    dec_fill(a, d_llr, n_seg, seg_stride, blocks_per_seg, out);
    a.n_iter = n_iter;
    a.ext = h->t_ws;
    a.ckpt = h->t_ws + n_blocks * K;
    a.llr_out = out->llr;
    a.q = turbo_qpp(K, f1, f2);
    HIP_TRY(launch_turbo_decode(a, s));
    return OFDM_OK;
}

// ---- early termination by CRC: the same workspace with a second K-float array per block
int ofdm_rx_reserve_turbo_es(ofdm_rx* h, int64_t n_blocks, int32_t K) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_turbo_es: null handle");
    const char* bad = turbo_bad_reserve(n_blocks, K);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_turbo_es: %s", bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(turbo_decode_es_prepare());
    return turbo_grow(h, turbo_es_ws_floats(n_blocks, K));
}

int ofdm_turbo_decode_es_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, int32_t K,
                                int32_t f1, int32_t f2, int32_t crc_kind, int32_t min_iter, int32_t max_iter,
                                const ofdm_turbo_es_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_turbo_decode_es_frames: null handle");
    const char* bad = turbo_bad_geometry(n_seg, blocks_per_seg, K, f1, f2);
    if (!*bad) {
        if (crc_kind < OFDM_CRC24A || crc_kind > OFDM_CRC8) bad = "crc_kind must be OFDM_CRC24A, OFDM_CRC24B, OFDM_CRC16 or OFDM_CRC8";
        else if (min_iter < 1 || max_iter > TURBO_ITER_MAX || min_iter > max_iter) bad = "1 <= min_iter <= max_iter <= 16 does not hold";
        else if (*(bad = dec_bad_args(n_seg, seg_stride, int64_t(blocks_per_seg) * (3 * int64_t(K) + 12), TURBO_SHORT_STRIDE, out))) {}
        else if (out && out->stat_stride != 0 && out->stat_stride < blocks_per_seg) bad = "stat_stride must be 0 or >= blocks_per_seg";
        else if (out && !batch_items_ok(n_seg, out->stat_stride)) bad = "batch beyond the kernel's index range";
    }
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_turbo_decode_es_frames: %s", bad);
    if (n_seg == 0 || blocks_per_seg == 0 || !turbo_es_wanted(out)) return OFDM_OK;
    if (!d_llr) return fail(OFDM_ERR_INVALID, "ofdm_turbo_decode_es_frames: null d_llr");
    hipStream_t s = pick_stream(h, stream);
    const int64_t n_blocks = n_seg * blocks_per_seg;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int rc = grow_outside_capture(turbo_es_ws_floats(n_blocks, K) <= h->cap_turbo, s, "ofdm_turbo_decode_es_frames",
                                        "ofdm_rx_reserve_turbo_es", [&] { return ofdm_rx_reserve_turbo_es(h, n_blocks, K); });
    if (rc != OFDM_OK) return rc;
    TurboDecEsArgs a{};
    dec_fill(a, d_llr, n_seg, seg_stride, blocks_per_seg, out);
    a.min_iter = min_iter;
    a.max_iter = max_iter;
    a.crc_kind = crc_kind;
    a.ext = h->t_ws;
    a.post = a.ext + n_blocks * K;
    a.ckpt = a.post + n_blocks * K;
    a.llr_out = out->llr;
    a.iters = out->iters;
    a.crc_ok = out->crc_ok;
    a.stat_stride = out->stat_stride ? out->stat_stride : blocks_per_seg;
    a.q = turbo_qpp(K, f1, f2);
    HIP_TRY(launch_turbo_decode_es(a, s));
    return OFDM_OK;
}

// ---- rate matching (TS 36.212 5.1.4.1)
int64_t ofdm_turbo_rm_blocks(int64_t seg_bits, int32_t K, int32_t E) {
    if (!turbo_valid_k(K)) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rm_blocks: %s", TURBO_BAD_K);
    if (E < 1 || E > TURBO_RM_MAX_COPIES * (3 * int64_t(K) + 12)) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rm_blocks: E must lie in 1 .. 16 (3K + 12)");
    if (seg_bits < 0) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rm_blocks: negative seg_bits");
    return seg_bits / E;
}

int ofdm_turbo_rm_info(int32_t K, int32_t Ncb, int32_t rv, int32_t* k0, int32_t* n_avail) {
    if (!turbo_valid_k(K)) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rm_info: %s", TURBO_BAD_K);
    const char* bad = turbo_rm_bad_geometry(K, 1, Ncb, rv, nullptr);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rm_info: %s", bad);
    const TurboRmGeom g = turbo_rm_geom(K, 1, Ncb);
    if (k0) *k0 = turbo_rm_k0(K, g.Ncb, rv);
    if (n_avail) *n_avail = g.navail;
    return OFDM_OK;
}

int ofdm_tx_reserve_turbo_rm(ofdm_tx* h) { return prepare_only(h, "ofdm_tx_reserve_turbo_rm", turbo_rm_prepare); }
int ofdm_rx_reserve_turbo_rm(ofdm_rx* h) { return prepare_only(h, "ofdm_rx_reserve_turbo_rm", turbo_rm_prepare); }

int ofdm_tx_turbo_encode_rm_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                                   int32_t K, int32_t f1, int32_t f2, int32_t E, int32_t Ncb, int32_t rv, const int32_t* d_rv,
                                   uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_turbo_encode_rm_frames: null handle");
    const char* bad = turbo_bad_geometry(n_seg, blocks_per_seg, K, f1, f2);
    if (!*bad) bad = turbo_rm_bad_geometry(K, E, Ncb, rv, d_rv);
    if (!*bad) bad = enc_bad_args(info_mode, coded_mode, n_seg, seg_bits, int64_t(blocks_per_seg) * E, "seg_bits < blocks_per_seg * E");
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_turbo_encode_rm_frames: %s", bad);
    if (n_seg == 0 || seg_bits == 0) return OFDM_OK;
    if (!d_coded || (blocks_per_seg > 0 && !d_info)) return fail(OFDM_ERR_INVALID, "ofdm_tx_turbo_encode_rm_frames: null buffer");
    TurboEncRmArgs a{};
    enc_fill(a, d_info, info_mode, n_seg, blocks_per_seg, d_coded, coded_mode, seg_bits);
    a.q = turbo_qpp(K, f1, f2);
    a.g = turbo_rm_geom(K, E, Ncb);
    a.rv = rv;
    a.rv_dev = d_rv;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_turbo_encode_rm(a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_turbo_rate_dematch_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                                   int32_t K, int32_t E, int32_t Ncb, int32_t rv, const int32_t* d_rv, int32_t accumulate,
                                   float* d_out, int64_t out_stride, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rate_dematch_frames: null handle");
    const int64_t per = 3 * int64_t(K) + 12;
    const char* bad = "";
    if (!turbo_valid_k(K)) bad = TURBO_BAD_K;
    else if (n_seg < 0 || blocks_per_seg < 0) bad = "negative count";
    else if (*(bad = turbo_rm_bad_geometry(K, E, Ncb, rv, d_rv))) {}
    else if (seg_stride < int64_t(blocks_per_seg) * E) bad = "seg_stride < blocks_per_seg * E";
    else if (out_stride < int64_t(blocks_per_seg) * per) bad = "out_stride < blocks_per_seg * (3K + 12)";
    // one thread per output LLR in workgroups of 256: the grid's x range bounds n_seg * blocks_per_seg * (3K + 12)
    else if (!batch_items_ok(n_seg, seg_stride) || !batch_items_ok(n_seg, out_stride) || n_seg > MAX_BLOCKS ||
             (blocks_per_seg > 0 && n_seg > MAX_BLOCKS * int64_t(256) / per / blocks_per_seg))
        bad = "batch beyond the kernel's index range";
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rate_dematch_frames: %s", bad);
    if (n_seg == 0 || blocks_per_seg == 0) return OFDM_OK;
    if (!d_llr || !d_out) return fail(OFDM_ERR_INVALID, "ofdm_turbo_rate_dematch_frames: null buffer");
    TurboDematchArgs a{};
    a.llr = d_llr;
    a.seg_stride = seg_stride;
    a.n_blocks = n_seg * blocks_per_seg;
    a.blocks_per_seg = blocks_per_seg;
    a.K = K;
    a.out = d_out;
    a.out_stride = out_stride;
    a.accumulate = accumulate;
    a.g = turbo_rm_geom(K, E, Ncb);
    a.rv = rv;
    a.rv_dev = d_rv;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_turbo_dematch(a, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
