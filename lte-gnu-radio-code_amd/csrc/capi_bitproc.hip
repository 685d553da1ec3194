// capi_bitproc.hip -- LTE CRC and Gold-sequence scrambling on the frame-batched path (definition: include/ofdm_mi355x.h, DESIGN.md
// 9.2.5): the host-only CRC and sequence routines, CRC attach and scrambling on the transmitter handle, descrambling of LLRs and
// the CRC check on the receiver handle, and the two reserve calls.
#include "capi_internal.hpp"

namespace {
// "" = fine
const char* crc_bad_geometry(int32_t kind, int64_t A) {
    if (kind < OFDM_CRC24A || kind > OFDM_CRC8) return "kind must be OFDM_CRC24A, OFDM_CRC24B, OFDM_CRC16 or OFDM_CRC8";
    if (A < CRC_A_MIN || A > CRC_A_MAX || A % 8) return "A must be a multiple of 8 with 8 <= A <= 2040";
    if (A + crc_bits(kind) > CRC_K_MAX) return "A + L must not exceed 2048";
    return "";
}
const char* crc_bad_args(int32_t kind, int64_t A, int64_t n_blocks, int32_t mode_a, int32_t mode_b, uint32_t mask, const uint32_t* d_mask) {
    const char* bad = crc_bad_geometry(kind, A);
    if (*bad) return bad;
    if (n_blocks < 0) return "negative count";
    if (n_blocks > MAX_BLOCKS) return "batch beyond the kernel's index range";
    if (!bits_mode_ok(mode_a) || !bits_mode_ok(mode_b)) return "bit modes must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    if (!d_mask && (mask >> crc_bits(kind))) return "scalar mask has bits at or above L";
    return "";
}
// n_seg segments of seg_bits scrambled bits at strides of stride_a / stride_b elements
const char* gold_bad_args(int64_t n_seg, int64_t seg_bits, int64_t stride_a, int64_t stride_b) {
    if (n_seg < 0 || seg_bits < 0) return "negative count";
    if (seg_bits >= GOLD_MAX_BITS) return "seg_bits must be below 2^31 - 1600";
    if (stride_a < seg_bits || stride_b < seg_bits) return "stride shorter than seg_bits";
    if (!batch_items_ok(n_seg, stride_a) || !batch_items_ok(n_seg, stride_b)) return "batch beyond the kernel's index range";
    return "";
}
// the fields attach and check share
CrcArgs crc_args(int32_t kind, int32_t A, int64_t n_blocks, uint32_t mask, const uint32_t* d_mask, int32_t info_mode, int32_t payload_mode) {
    CrcArgs a{};
    a.kind = kind;
    a.A = A;
    a.n_blocks = n_blocks;
    a.mask = mask;
    a.mask_dev = d_mask;
    a.info_mode = info_mode;
    a.payload_mode = payload_mode;
    return a;
}
}  // namespace

extern "C" {

int32_t ofdm_crc_bits(int32_t kind) {
    if (kind < OFDM_CRC24A || kind > OFDM_CRC8) return fail(OFDM_ERR_INVALID, "ofdm_crc_bits: unknown kind %d", int(kind));
    return crc_bits(kind);
}

int ofdm_crc_compute(int32_t kind, const uint8_t* host_bits_packed, int32_t A, uint32_t* crc) {
    const char* bad = crc_bad_geometry(kind, A);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_crc_compute: %s", bad);
    if (!host_bits_packed || !crc) return fail(OFDM_ERR_INVALID, "ofdm_crc_compute: null argument");
    *crc = crc_host(kind, host_bits_packed, A);
    return OFDM_OK;
}

int ofdm_crc_compute_long(int32_t kind, const uint8_t* host_bits_packed, int64_t n_bits, uint32_t* crc) {
    if (kind < OFDM_CRC24A || kind > OFDM_CRC8) return fail(OFDM_ERR_INVALID, "ofdm_crc_compute_long: kind must be OFDM_CRC24A, OFDM_CRC24B, OFDM_CRC16 or OFDM_CRC8");
    if (n_bits < 8 || n_bits > (int64_t(1) << 30) || n_bits % 8) return fail(OFDM_ERR_INVALID, "ofdm_crc_compute_long: n_bits must be a multiple of 8 with 8 <= n_bits <= 2^30");
    if (!host_bits_packed || !crc) return fail(OFDM_ERR_INVALID, "ofdm_crc_compute_long: null argument");
    *crc = crc_long_host(kind, host_bits_packed, n_bits >> 3);
    return OFDM_OK;
}

int ofdm_gold_bits(uint32_t c_init, int64_t first, int64_t n, uint8_t* host_out) {
    if (first < 0 || n < 0) return fail(OFDM_ERR_INVALID, "ofdm_gold_bits: negative count");
    if (first > GOLD_MAX_BITS || n > GOLD_MAX_BITS - first) return fail(OFDM_ERR_INVALID, "ofdm_gold_bits: first + n beyond 2^31 - 1600");
    if (n == 0) return OFDM_OK;
    if (!host_out) return fail(OFDM_ERR_INVALID, "ofdm_gold_bits: null host_out");
    gold_bits_host(c_init, first, n, host_out);
    return OFDM_OK;
}

int ofdm_tx_reserve_bitproc(ofdm_tx* h) { return prepare_only(h, "ofdm_tx_reserve_bitproc", bitproc_prepare); }
int ofdm_rx_reserve_bitproc(ofdm_rx* h) { return prepare_only(h, "ofdm_rx_reserve_bitproc", bitproc_prepare); }

int ofdm_tx_crc_attach_frames(ofdm_tx* h, const uint8_t* d_payload, int32_t payload_mode, int64_t n_blocks, int32_t A, int32_t kind,
                              uint32_t mask, const uint32_t* d_mask, uint8_t* d_info, int32_t info_mode, void* stream) {
    const char* bad = crc_bad_args(kind, A, n_blocks, payload_mode, info_mode, mask, d_mask);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_crc_attach_frames: %s", bad);
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_crc_attach_frames: null handle");
    if (n_blocks == 0) return OFDM_OK;
    if (!d_payload || !d_info) return fail(OFDM_ERR_INVALID, "ofdm_tx_crc_attach_frames: null buffer");
    CrcArgs a = crc_args(kind, A, n_blocks, mask, d_mask, info_mode, payload_mode);
    a.payload_in = d_payload;
    a.info_out = d_info;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_crc(a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_crc_check_frames(ofdm_rx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_blocks, int32_t A, int32_t kind,
                          uint32_t mask, const uint32_t* d_mask, const ofdm_crc_out* out, void* stream) {
    const int32_t payload_mode = out && out->payload ? out->payload_mode : info_mode;
    const char* bad = crc_bad_args(kind, A, n_blocks, info_mode, payload_mode, mask, d_mask);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_crc_check_frames: %s", bad);
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_crc_check_frames: null handle");
    if (n_blocks == 0 || !out || (!out->ok && !out->syndrome && !out->payload)) return OFDM_OK;
    if (!d_info) return fail(OFDM_ERR_INVALID, "ofdm_crc_check_frames: null d_info");
    CrcArgs a = crc_args(kind, A, n_blocks, mask, d_mask, info_mode, payload_mode);
    a.info_in = d_info;
    a.ok = out->ok;
    a.syndrome = out->syndrome;
    a.payload_out = out->payload;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_crc(a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tx_scramble_frames(ofdm_tx* h, const uint8_t* d_in, int32_t mode, int64_t n_seg, int64_t seg_bits, const uint32_t* d_cinit,
                            uint8_t* d_out, void* stream) {
    const char* bad = gold_bad_args(n_seg, seg_bits, seg_bits, seg_bits);
    if (!*bad && !bits_mode_ok(mode)) bad = "mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    if (!*bad && mode == OFDM_BITS_PACKED && (seg_bits & 7)) bad = "packed bits need seg_bits % 8 == 0";
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_scramble_frames: %s", bad);
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_scramble_frames: null handle");
    if (n_seg == 0 || seg_bits == 0) return OFDM_OK;
    if (!d_in || !d_out || !d_cinit) return fail(OFDM_ERR_INVALID, "ofdm_tx_scramble_frames: null buffer");
    GoldArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.in_stride = a.out_stride = mode == OFDM_BITS_PACKED ? seg_bits >> 3 : seg_bits;
    a.n_seg = n_seg;
    a.seg_bits = seg_bits;
    a.cinit = d_cinit;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_gold_bits(a, mode == OFDM_BITS_PACKED, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_descramble_llr_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int64_t seg_bits,
                               const uint32_t* d_cinit, float* d_out, int64_t out_stride, void* stream) {
    const char* bad = gold_bad_args(n_seg, seg_bits, seg_stride, out_stride);
    if (!*bad && d_llr && d_out == d_llr && out_stride != seg_stride) bad = "in place needs out_stride == seg_stride";
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_descramble_llr_frames: %s", bad);
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_descramble_llr_frames: null handle");
    if (n_seg == 0 || seg_bits == 0) return OFDM_OK;
    if (!d_llr || !d_out || !d_cinit) return fail(OFDM_ERR_INVALID, "ofdm_descramble_llr_frames: null buffer");
    GoldArgs a{};
    a.in = d_llr;
    a.out = d_out;
    a.in_stride = seg_stride;
    a.out_stride = out_stride;
    a.n_seg = n_seg;
    a.seg_bits = seg_bits;
    a.cinit = d_cinit;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_gold_llr(a, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
