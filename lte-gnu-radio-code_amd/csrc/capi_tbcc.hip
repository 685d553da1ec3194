// capi_tbcc.hip -- the LTE tail-biting convolutional code on the frame-batched path (definition: include/ofdm_mi355x.h, DESIGN.md
// 9.2.3) and its rate matching (TS 36.212 5.1.4.2): the host-only block counts, the two encode calls of the
// transmitter handle, and reserve, the two decodes and the de-matching call of the receiver handle.
#include "capi_internal.hpp"

namespace {
// K and the counts, in the order the calls report them; "" = fine
const char* tbcc_bad_geometry(int64_t n_seg, int64_t blocks_per_seg, int64_t K) {
    if (!tbcc_valid_k(K)) return "K must be a multiple of 8 with 24 <= K <= 2048";
    if (n_seg < 0 || blocks_per_seg < 0) return "negative count";
    if (blocks_per_seg > MAX_BLOCKS || (blocks_per_seg > 0 && n_seg > MAX_BLOCKS / blocks_per_seg))
        return "batch beyond the kernels' index range";
    return "";
}
// the same with rate matching: E coded bits per block
const char* tbcc_rm_bad_geometry(int64_t n_seg, int64_t blocks_per_seg, int64_t K, int64_t E) {
    const char* bad = tbcc_bad_geometry(n_seg, blocks_per_seg, K);
    if (*bad) return bad;
    if (!tbcc_valid_e(K, E)) return "E must lie in 1 .. 48K";
    return "";
}
bool tbcc_wanted(const ofdm_tbcc_out* o) { return o && (o->bits || o->metric || o->tb_ok); }
template <class Args>
void tbcc_dec_fill(Args& a, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, int32_t K, const ofdm_tbcc_out* out) {
    dec_fill(a, d_llr, n_seg, seg_stride, blocks_per_seg, out);
    a.K = K;
    a.metric = out->metric;
    a.tb_ok = out->tb_ok;
}
}  // namespace

extern "C" {

int64_t ofdm_tbcc_blocks(int64_t seg_bits, int32_t K) {
    if (!tbcc_valid_k(K)) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_blocks: K must be a multiple of 8 with 24 <= K <= 2048");
    if (seg_bits < 0) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_blocks: negative seg_bits");
    return seg_bits / (3 * int64_t(K));
}

int64_t ofdm_tbcc_rm_blocks(int64_t seg_bits, int32_t K, int32_t E) {
    const char* bad = tbcc_rm_bad_geometry(0, 0, K, E);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rm_blocks: %s", bad);
    if (seg_bits < 0) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rm_blocks: negative seg_bits");
    return seg_bits / E;
}

int ofdm_tx_tbcc_encode_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                               int32_t K, uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_tbcc_encode_frames: null handle");
    const char* bad = tbcc_bad_geometry(n_seg, blocks_per_seg, K);
    if (!*bad) bad = enc_bad_args(info_mode, coded_mode, n_seg, seg_bits, int64_t(blocks_per_seg) * 3 * K, "seg_bits < blocks_per_seg * 3K");
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_tbcc_encode_frames: %s", bad);
    if (n_seg == 0 || seg_bits == 0) return OFDM_OK;
    if (!d_coded || (blocks_per_seg > 0 && !d_info)) return fail(OFDM_ERR_INVALID, "ofdm_tx_tbcc_encode_frames: null buffer");
    TbccEncArgs a{};
    enc_fill(a, d_info, info_mode, n_seg, blocks_per_seg, d_coded, coded_mode, seg_bits);
    a.K = K;
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tbcc_encode(a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tx_tbcc_encode_rm_frames(ofdm_tx* h, const uint8_t* d_info, int32_t info_mode, int64_t n_seg, int32_t blocks_per_seg,
                                  int32_t K, int32_t E, uint8_t* d_coded, int32_t coded_mode, int64_t seg_bits, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_tbcc_encode_rm_frames: null handle");
    const char* bad = tbcc_rm_bad_geometry(n_seg, blocks_per_seg, K, E);
    if (!*bad) bad = enc_bad_args(info_mode, coded_mode, n_seg, seg_bits, int64_t(blocks_per_seg) * E, "seg_bits < blocks_per_seg * E");
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_tbcc_encode_rm_frames: %s", bad);
    if (n_seg == 0 || seg_bits == 0) return OFDM_OK;
    if (!d_coded || (blocks_per_seg > 0 && !d_info)) return fail(OFDM_ERR_INVALID, "ofdm_tx_tbcc_encode_rm_frames: null buffer");
    TbccEncRmArgs a{};
    enc_fill(a, d_info, info_mode, n_seg, blocks_per_seg, d_coded, coded_mode, seg_bits);
    a.K = K;
    a.g = tbcc_rm_geom(K, E);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tbcc_encode_rm(a, pick_stream(h, stream)));
    return OFDM_OK;
}

// The decoder keeps its survivors in LDS and has no device workspace, so there is nothing to allocate: the call checks the
// geometry a later decode will use and loads the code objects of both decoders (plain and rate-matched), which is the one piece
// of set-up a first launch would otherwise do inside a capture.
int ofdm_rx_reserve_tbcc(ofdm_rx* h, int64_t n_blocks, int32_t K) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_tbcc: null handle");
    const char* bad = tbcc_bad_geometry(1, n_blocks, K);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_rx_reserve_tbcc: %s", bad);
    return prepare_only(h, "ofdm_rx_reserve_tbcc", tbcc_decode_prepare);
}

int ofdm_tbcc_decode_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg, int32_t K,
                            const ofdm_tbcc_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_decode_frames: null handle");
    const char* bad = tbcc_bad_geometry(n_seg, blocks_per_seg, K);
    if (!*bad) bad = dec_bad_args(n_seg, seg_stride, int64_t(blocks_per_seg) * 3 * K, "seg_stride < blocks_per_seg * 3K", out);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_decode_frames: %s", bad);
    if (n_seg == 0 || blocks_per_seg == 0 || !tbcc_wanted(out)) return OFDM_OK;
    if (!d_llr) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_decode_frames: null d_llr");
    TbccDecArgs a{};
    tbcc_dec_fill(a, d_llr, n_seg, seg_stride, blocks_per_seg, K, out);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tbcc_decode(a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tbcc_rate_dematch_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                                  int32_t K, int32_t E, float* d_out, int64_t out_stride, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rate_dematch_frames: null handle");
    const char* bad = tbcc_rm_bad_geometry(n_seg, blocks_per_seg, K, E);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rate_dematch_frames: %s", bad);
    if (seg_stride < int64_t(blocks_per_seg) * E)
        return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rate_dematch_frames: seg_stride < blocks_per_seg * E");
    if (out_stride < int64_t(blocks_per_seg) * 3 * K)
        return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rate_dematch_frames: out_stride < blocks_per_seg * 3K");
    // one thread per output LLR in workgroups of 256: the grid's x range bounds n_seg * blocks_per_seg * 3K
    if (!batch_items_ok(n_seg, seg_stride) || !batch_items_ok(n_seg, out_stride) ||
        n_seg * int64_t(blocks_per_seg) > MAX_BLOCKS * int64_t(256) / (3 * K))
        return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rate_dematch_frames: batch beyond the kernel's index range");
    if (n_seg == 0 || blocks_per_seg == 0) return OFDM_OK;
    if (!d_llr || !d_out) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_rate_dematch_frames: null buffer");
    TbccDematchArgs a{};
    a.llr = d_llr;
    a.seg_stride = seg_stride;
    a.n_blocks = n_seg * blocks_per_seg;
    a.blocks_per_seg = blocks_per_seg;
    a.K = K;
    a.out = d_out;
    a.out_stride = out_stride;
    a.g = tbcc_rm_geom(K, E);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tbcc_dematch(a, pick_stream(h, stream)));
    return OFDM_OK;
}

int ofdm_tbcc_decode_rm_frames(ofdm_rx* h, const float* d_llr, int64_t n_seg, int64_t seg_stride, int32_t blocks_per_seg,
                               int32_t K, int32_t E, const ofdm_tbcc_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_decode_rm_frames: null handle");
    const char* bad = tbcc_rm_bad_geometry(n_seg, blocks_per_seg, K, E);
    if (!*bad) bad = dec_bad_args(n_seg, seg_stride, int64_t(blocks_per_seg) * E, "seg_stride < blocks_per_seg * E", out);
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_decode_rm_frames: %s", bad);
    if (n_seg == 0 || blocks_per_seg == 0 || !tbcc_wanted(out)) return OFDM_OK;
    if (!d_llr) return fail(OFDM_ERR_INVALID, "ofdm_tbcc_decode_rm_frames: null d_llr");
    TbccDecRmArgs a{};
    tbcc_dec_fill(a, d_llr, n_seg, seg_stride, blocks_per_seg, K, out);
    a.g = tbcc_rm_geom(K, E);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(launch_tbcc_decode_rm(a, pick_stream(h, stream)));
    return OFDM_OK;
}

}  // extern "C"
