// capi_tb.hip -- the transport-block layer of the LTE data channel on the frame-batched path (definition:
// include/ofdm_mi355x.h): the segmentation and rate-matching arithmetic on the host
// and the two calls that run a whole transport block -- segment, encode per group, concatenate on the transmitter handle;
// de-match per group, decode per K, desegment on the receiver handle.  The encoder, the de-matcher and the decoder are reached
// through their own public calls (capi_turbo.hip); everything those calls would refuse is refused here first, so that an
// argument error never leaves a half-enqueued transport block behind.
#include "capi_internal.hpp"

namespace {

// "" = fine; fills *o (zeroed first).  G == 0: the segmentation fields and the groups of one K each.
const char* tb_plan(int64_t A, int64_t Z, int64_t G, int64_t q, int64_t N_IR, ofdm_tb_geom* o) {
    std::memset(o, 0, sizeof *o);
    if (Z == 0) Z = TURBO_K_MAX;
    if (!turbo_k_is_lte(Z)) return "Z must be 0 or one of LTE's 188 block sizes";
    if (A < TB_A_MIN || A > TB_A_MAX || A % 8) return "A must be a multiple of 8 with 8 <= A <= 2^20 - 24";
    const int64_t B = A + 24;
    const int64_t L = B <= Z ? 0 : 24;
    const int64_t C = L ? (B + Z - 25) / (Z - 24) : 1;
    const int64_t Bp = B + L * C;
    const int64_t Kp = turbo_k_next((Bp + C - 1) / C);       // <= Z: B <= C (Z - 24)
    int64_t Km = 0, Cm = 0;
    if (C > 1) {
        Km = turbo_k_prev(int(Kp));
        Cm = (C * Kp - Bp) / (Km ? Kp - Km : 8);
        if (Cm > 0 && !Km) return "this segmentation needs a block size below 40";
    }
    const int64_t Cp = C - Cm;
    o->A = int32_t(A), o->Z = int32_t(Z), o->B = int32_t(B), o->L = int32_t(L), o->C = int32_t(C);
    o->K_plus = int32_t(Kp), o->K_minus = int32_t(Km), o->C_plus = int32_t(Cp), o->C_minus = int32_t(Cm);
    o->F = int32_t(Cp * Kp + Cm * Km - Bp);
    o->soft_floats = Cm * (3 * Km + 12) + Cp * (3 * Kp + 12);
    int64_t e_cut = C;                                       // blocks r < e_cut have E0
    if (G != 0) {
        if (G < 0 || G > INT32_MAX) return "G must lie in 1 .. 2^31 - 1";
        if (q < 1 || G % q) return "q must be >= 1 and divide G";
        if (N_IR < 0) return "negative N_IR";
        const int64_t Gq = G / q;
        o->G = int32_t(G), o->q = int32_t(q), o->gamma = int32_t(Gq % C);
        o->E0 = int32_t(q * (Gq / C));
        o->E1 = o->gamma ? int32_t(o->E0 + q) : o->E0;
        e_cut = C - o->gamma;
        for (int which = 0; which < 2; ++which) {
            const int64_t K = which ? Kp : Km;
            if (which == 0 && Cm == 0) continue;
            const int64_t kpi = turbo_rm_kpi(int(K));
            const int64_t ncb = N_IR ? std::min(N_IR / C, 3 * kpi) : 3 * kpi;
            if (ncb < kpi) return "N_IR / C is below Kpi of a code block";
            (which ? o->Ncb_plus : o->Ncb_minus) = int32_t(ncb);
        }
    }
    const int64_t cut[4] = {0, std::min(Cm, e_cut), std::max(Cm, e_cut), C};
    int64_t cw = 0, soft = 0;
    for (int i = 0; i < 3; ++i) {
        const int64_t first = cut[i], count = cut[i + 1] - cut[i];
        if (count <= 0) continue;
        auto& g = o->group[o->n_groups++];
        g.first = int32_t(first), g.count = int32_t(count);
        g.K = int32_t(first < Cm ? Km : Kp);
        g.E = G ? (first < e_cut ? o->E0 : o->E1) : 0;
        g.cw_bit_offset = cw, g.soft_offset = soft;
        cw += count * g.E, soft += count * (3 * int64_t(g.K) + 12);
        if (G) {
            const int ncb = first < Cm ? o->Ncb_minus : o->Ncb_plus;
            if (g.E < 1 || g.E > int64_t(TURBO_RM_MAX_COPIES) * turbo_rm_geom(g.K, 1, ncb).navail) return "every E_r must lie in 1 .. 16 Navail of its block";
        }
    }
    return "";
}

constexpr int64_t TB_MAX_ITEMS = int64_t(1) << 38;           // n_tb * the longest per-block row: inside every limit of the calls behind

// what both calls check about the geometry and the batch, in the order they report it; fills *g
const char* tb_bad_call(int64_t n_tb, int32_t A, int32_t Z, int64_t G, int32_t q, int64_t N_IR, int32_t f1m, int32_t f2m, int32_t f1p,
                        int32_t f2p, int32_t rv, const int32_t* d_rv, int64_t row_a, int64_t row_b, ofdm_tb_geom* g) {
    if (G == 0) return "G must lie in 1 .. 2^31 - 1";
    const char* bad = tb_plan(A, Z, G, q, N_IR, g);
    if (*bad) return bad;
    if (n_tb < 0) return "negative count";
    if (g->C_minus > 0 && !turbo_qpp_valid(g->K_minus, f1m, f2m)) return "(f1_minus, f2_minus) is no permutation of 0 .. K_minus - 1";
    if (!turbo_qpp_valid(g->K_plus, f1p, f2p)) return "(f1_plus, f2_plus) is no permutation of 0 .. K_plus - 1";
    if (!d_rv && (rv < 0 || rv > 3)) return "rv must lie in 0 .. 3";
    const int64_t row = std::max(std::max(row_a, row_b), std::max<int64_t>(g->soft_floats, g->G));
    if (n_tb > MAX_BLOCKS / g->C || row > TB_MAX_ITEMS || (n_tb > 0 && row > TB_MAX_ITEMS / n_tb)) return "batch beyond the kernels' index range";
    return "";
}

int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }

TbSeg tb_seg(const ofdm_tb_geom& g) {
    TbSeg s{};
    s.A8 = g.A >> 3, s.L8 = g.L >> 3, s.C = g.C, s.Cm = g.C_minus, s.Km8 = g.K_minus >> 3, s.Kp8 = g.K_plus >> 3, s.F8 = g.F >> 3;
    return s;
}

// transmit workspace: the packed code blocks of every group, then every group's encoder output, one bit per byte
struct TxLayout {
    int64_t info[3], enc[3], bytes;
};
TxLayout tx_layout(const ofdm_tb_geom& g, int64_t n_tb) {
    TxLayout l{};
    int64_t at = 0;
    for (int i = 0; i < g.n_groups; ++i) {
        l.info[i] = at;
        at = align16(at + n_tb * g.group[i].count * (g.group[i].K >> 3));
    }
    for (int i = 0; i < g.n_groups; ++i) {
        l.enc[i] = at;
        at = align16(at + n_tb * g.group[i].count * g.group[i].E);
    }
    l.bytes = at;
    return l;
}
// receive workspace: the decoder's packed bits, K- blocks first
struct RxLayout {
    int64_t bits[2], bytes;
};
RxLayout rx_layout(const ofdm_tb_geom& g, int64_t n_tb) {
    RxLayout l{};
    l.bits[0] = 0;
    l.bits[1] = align16(n_tb * g.C_minus * (g.K_minus >> 3));
    l.bytes = align16(l.bits[1] + n_tb * g.C_plus * (g.K_plus >> 3));
    return l;
}
int64_t rx_turbo_floats(const ofdm_tb_geom& g, int64_t n_tb) {
    const int64_t p = turbo_ws_floats(n_tb * g.C_plus, g.K_plus);
    return g.C_minus ? std::max(p, turbo_ws_floats(n_tb * g.C_minus, g.K_minus)) : p;
}

int64_t rx_turbo_es_floats(const ofdm_tb_geom& g, int64_t n_tb) {
    const int64_t p = turbo_es_ws_floats(n_tb * g.C_plus, g.K_plus);
    return g.C_minus ? std::max(p, turbo_es_ws_floats(n_tb * g.C_minus, g.K_minus)) : p;
}

template <class H>
int tb_grow(H* h, int64_t bytes) {
    if (bytes <= h->cap_tb) return OFDM_OK;
    return regrow(h, {{&h->cap_tb, bytes}}, ws_buf(&h->tb_ws, size_t(bytes)));
}

int rx_reserve_tb(ofdm_rx* h, int64_t n_tb, int32_t A, int32_t Z, bool es, const char* who) {
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", who);
    ofdm_tb_geom g;
    const char* bad = tb_plan(A, Z, 0, 0, 0, &g);
    if (!*bad && (n_tb < 0 || n_tb > MAX_BLOCKS / g.C || (n_tb > 0 && g.soft_floats > TB_MAX_ITEMS / n_tb)))
        bad = "negative count or a batch beyond the kernels' index range";
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", who, bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(tb_prepare());
    HIP_TRY(turbo_rm_prepare());
    auto reserve = es ? ofdm_rx_reserve_turbo_es : ofdm_rx_reserve_turbo;
    int rc = OFDM_OK;
    if (g.C_minus) rc = reserve(h, n_tb * g.C_minus, g.K_minus);
    if (rc == OFDM_OK) rc = reserve(h, n_tb * g.C_plus, g.K_plus);
    return rc != OFDM_OK ? rc : tb_grow(h, rx_layout(g, n_tb).bytes);
}

// what tells ofdm_tb_decode_frames (min_iter == max_iter == n_iter through the fixed decoder) from ofdm_tb_decode_es_frames
struct TbDecode {
    const char* who;
    const char* reserve_name;
    bool es;
    int32_t min_iter, max_iter;
    uint8_t* cb_iters;       // [n_tb][C], or null
};

int tb_decode(ofdm_rx* h, const float* d_llr, int64_t n_tb, int64_t llr_stride, int32_t A, int32_t Z, int64_t G, int32_t q, int64_t N_IR,
              int32_t f1_minus, int32_t f2_minus, int32_t f1_plus, int32_t f2_plus, int32_t rv, const int32_t* d_rv, const TbDecode& d,
              int32_t accumulate, float* d_soft, int64_t soft_stride, const ofdm_tb_out* out, void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "%s: null handle", d.who);
    ofdm_tb_geom g;
    const char* bad = tb_bad_call(n_tb, A, Z, G, q, N_IR, f1_minus, f2_minus, f1_plus, f2_plus, rv, d_rv, llr_stride, soft_stride, &g);
    if (!*bad) {
        if (!d.es && (d.max_iter < 1 || d.max_iter > TURBO_ITER_MAX)) bad = "n_iter must lie in 1 .. 16";
        else if (d.es && (d.min_iter < 1 || d.max_iter > TURBO_ITER_MAX || d.min_iter > d.max_iter)) bad = "1 <= min_iter <= max_iter <= 16 does not hold";
        else if (llr_stride < G) bad = "llr_stride < G";
        else if (soft_stride < g.soft_floats) bad = "soft_stride < sum (3 K_r + 12)";
        else if (!out) bad = "null out";
        else if (out->payload && !bits_mode_ok(out->payload_mode)) bad = "payload_mode must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
    }
    if (*bad) return fail(OFDM_ERR_INVALID, "%s: %s", d.who, bad);
    if (n_tb == 0) return OFDM_OK;
    if (!d_llr || !d_soft) return fail(OFDM_ERR_INVALID, "%s: null buffer", d.who);
    const bool decode = out->payload || out->tb_ok || out->cb_ok || out->syndrome || d.cb_iters;
    hipStream_t s = pick_stream(h, stream);
    HIP_TRY(hipSetDevice(h->cfg.device));
    const RxLayout l = rx_layout(g, n_tb);
    if (decode && (l.bytes > h->cap_tb || (d.es ? rx_turbo_es_floats(g, n_tb) : rx_turbo_floats(g, n_tb)) > h->cap_turbo)) {
        int rc = refuse_growth_in_capture(s, d.who, d.reserve_name);
        if (rc == OFDM_OK) rc = rx_reserve_tb(h, n_tb, A, Z, d.es, d.reserve_name);
        if (rc != OFDM_OK) return rc;
    }
    for (int i = 0; i < g.n_groups; ++i) {
        const auto& x = g.group[i];
        const int rc = ofdm_turbo_rate_dematch_frames(h, d_llr + x.cw_bit_offset, n_tb, llr_stride, x.count, x.K, x.E,
                                                      x.first < g.C_minus ? g.Ncb_minus : g.Ncb_plus, rv, d_rv, accumulate,
                                                      d_soft + x.soft_offset, soft_stride, s);
        if (rc != OFDM_OK) return rc;
    }
    if (!decode) return OFDM_OK;
    TbSegArgs sa{};
    sa.g = tb_seg(g);
    for (int which = 0; which < 2; ++which) {
        const int count = which ? g.C_plus : g.C_minus, K = which ? g.K_plus : g.K_minus;
        if (!count) continue;
        const int first = which ? g.C_minus : 0;
        const float* soft = d_soft + (which ? int64_t(g.C_minus) * (3 * int64_t(g.K_minus) + 12) : 0);
        const int32_t f1 = which ? f1_plus : f1_minus, f2 = which ? f2_plus : f2_minus;
        int rc;
        if (d.es) {
            ofdm_turbo_es_out to{};
            to.bits = h->tb_ws + l.bits[which];
            to.bits_mode = OFDM_BITS_PACKED;
            to.iters = d.cb_iters ? d.cb_iters + first : nullptr;
            to.stat_stride = g.C;
            rc = ofdm_turbo_decode_es_frames(h, soft, n_tb, soft_stride, count, K, f1, f2, g.L ? OFDM_CRC24B : OFDM_CRC24A, d.min_iter,
                                             d.max_iter, &to, s);
        } else {
            ofdm_turbo_out to{};
            to.bits = h->tb_ws + l.bits[which];
            to.bits_mode = OFDM_BITS_PACKED;
            rc = ofdm_turbo_decode_frames(h, soft, n_tb, soft_stride, count, K, f1, f2, d.max_iter, &to, s);
        }
        if (rc != OFDM_OK) return rc;
        sa.range[sa.n_ranges++] = TbRange{first, count, K >> 3, l.bits[which]};
    }
    sa.n_tb = n_tb;
    sa.ws = h->tb_ws;
    sa.payload_mode = out->payload_mode;
    sa.payload_out = out->payload;
    sa.tb_ok = out->tb_ok;
    sa.cb_ok = out->cb_ok;
    sa.syndrome = out->syndrome;
    HIP_TRY(launch_tb_desegment(sa, s));
    return OFDM_OK;
}

}  // namespace

extern "C" {

int32_t ofdm_turbo_k_next(int32_t bits) {
    const int K = turbo_k_next(bits);
    return K ? K : fail(OFDM_ERR_INVALID, "ofdm_turbo_k_next: no block size holds %d bits", int(bits));
}

int ofdm_tb_geometry(int32_t A, int32_t Z, int64_t G, int32_t q, int64_t N_IR, ofdm_tb_geom* out) {
    if (!out) return fail(OFDM_ERR_INVALID, "ofdm_tb_geometry: null out");
    const char* bad = tb_plan(A, Z, G, q, N_IR, out);
    return *bad ? fail(OFDM_ERR_INVALID, "ofdm_tb_geometry: %s", bad) : OFDM_OK;
}

int ofdm_tx_reserve_tb(ofdm_tx* h, int64_t n_tb, int32_t A, int32_t Z, int64_t G, int32_t q) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_tb: null handle");
    ofdm_tb_geom g;
    const char* bad = G == 0 ? "G must lie in 1 .. 2^31 - 1" : tb_plan(A, Z, G, q, 0, &g);
    if (!*bad && (n_tb < 0 || n_tb > MAX_BLOCKS / g.C || (n_tb > 0 && std::max<int64_t>(g.soft_floats, g.G) > TB_MAX_ITEMS / n_tb)))
        bad = "negative count or a batch beyond the kernels' index range";
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_reserve_tb: %s", bad);
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(tb_prepare());
    HIP_TRY(turbo_rm_prepare());
    return tb_grow(h, tx_layout(g, n_tb).bytes);
}

int ofdm_rx_reserve_tb(ofdm_rx* h, int64_t n_tb, int32_t A, int32_t Z) { return rx_reserve_tb(h, n_tb, A, Z, false, "ofdm_rx_reserve_tb"); }
int ofdm_rx_reserve_tb_es(ofdm_rx* h, int64_t n_tb, int32_t A, int32_t Z) { return rx_reserve_tb(h, n_tb, A, Z, true, "ofdm_rx_reserve_tb_es"); }

int ofdm_tx_tb_encode_frames(ofdm_tx* h, const uint8_t* d_payload, int32_t payload_mode, int64_t n_tb, int32_t A, int32_t Z,
                             int64_t G, int32_t q, int64_t N_IR, int32_t f1_minus, int32_t f2_minus, int32_t f1_plus,
                             int32_t f2_plus, int32_t rv, const int32_t* d_rv, uint8_t* d_cw, int32_t cw_mode, int64_t cw_bits,
                             void* stream) {
    if (!h) return fail(OFDM_ERR_INVALID, "ofdm_tx_tb_encode_frames: null handle");
    ofdm_tb_geom g;
    const char* bad = tb_bad_call(n_tb, A, Z, G, q, N_IR, f1_minus, f2_minus, f1_plus, f2_plus, rv, d_rv, cw_bits, 0, &g);
    if (!*bad) {
        if (!bits_mode_ok(payload_mode) || !bits_mode_ok(cw_mode)) bad = "bit modes must be OFDM_BITS_PACKED or OFDM_BITS_UNPACKED";
        else if (cw_bits < G) bad = "cw_bits < G";
        else if (cw_mode == OFDM_BITS_PACKED && (cw_bits & 7)) bad = "packed codewords need cw_bits % 8 == 0";
    }
    if (*bad) return fail(OFDM_ERR_INVALID, "ofdm_tx_tb_encode_frames: %s", bad);
    if (n_tb == 0) return OFDM_OK;
    if (!d_payload || !d_cw) return fail(OFDM_ERR_INVALID, "ofdm_tx_tb_encode_frames: null buffer");
    hipStream_t s = pick_stream(h, stream);
    HIP_TRY(hipSetDevice(h->cfg.device));
    const TxLayout l = tx_layout(g, n_tb);
    if (l.bytes > h->cap_tb) {
        int rc = refuse_growth_in_capture(s, "ofdm_tx_tb_encode_frames", "ofdm_tx_reserve_tb");
        if (rc == OFDM_OK) rc = tb_grow(h, l.bytes);
        if (rc != OFDM_OK) return rc;
    }
    TbSegArgs sa{};
    sa.g = tb_seg(g);
    sa.n_ranges = g.n_groups;
    for (int i = 0; i < g.n_groups; ++i) sa.range[i] = TbRange{g.group[i].first, g.group[i].count, g.group[i].K >> 3, l.info[i]};
    sa.n_tb = n_tb;
    sa.ws = h->tb_ws;
    sa.payload_mode = payload_mode;
    sa.payload_in = d_payload;
    HIP_TRY(launch_tb_segment(sa, s));
    TbConcatArgs ca{};
    ca.n_groups = g.n_groups;
    for (int i = 0; i < g.n_groups; ++i) {
        const auto& x = g.group[i];
        const bool minus = x.first < g.C_minus;
        const int64_t bits = int64_t(x.count) * x.E;
        const int rc = ofdm_tx_turbo_encode_rm_frames(h, h->tb_ws + l.info[i], OFDM_BITS_PACKED, n_tb, x.count, x.K, minus ? f1_minus : f1_plus,
                                                      minus ? f2_minus : f2_plus, x.E, minus ? g.Ncb_minus : g.Ncb_plus, rv, d_rv,
                                                      h->tb_ws + l.enc[i], OFDM_BITS_UNPACKED, bits, s);
        if (rc != OFDM_OK) return rc;
        ca.bits[i] = bits, ca.off[i] = x.cw_bit_offset, ca.base[i] = l.enc[i];
    }
    ca.n_tb = n_tb, ca.G = G, ca.cw_bits = cw_bits;
    ca.ws = h->tb_ws;
    ca.cw = d_cw;
    ca.cw_mode = cw_mode;
    HIP_TRY(launch_tb_concat(ca, s));
    return OFDM_OK;
}

int ofdm_tb_decode_frames(ofdm_rx* h, const float* d_llr, int64_t n_tb, int64_t llr_stride, int32_t A, int32_t Z, int64_t G,
                          int32_t q, int64_t N_IR, int32_t f1_minus, int32_t f2_minus, int32_t f1_plus, int32_t f2_plus,
                          int32_t rv, const int32_t* d_rv, int32_t n_iter, int32_t accumulate, float* d_soft, int64_t soft_stride,
                          const ofdm_tb_out* out, void* stream) {
    TbDecode d{"ofdm_tb_decode_frames", "ofdm_rx_reserve_tb", false, n_iter, n_iter, nullptr};
    return tb_decode(h, d_llr, n_tb, llr_stride, A, Z, G, q, N_IR, f1_minus, f2_minus, f1_plus, f2_plus, rv, d_rv, d, accumulate, d_soft,
                     soft_stride, out, stream);
}

int ofdm_tb_decode_es_frames(ofdm_rx* h, const float* d_llr, int64_t n_tb, int64_t llr_stride, int32_t A, int32_t Z, int64_t G,
                             int32_t q, int64_t N_IR, int32_t f1_minus, int32_t f2_minus, int32_t f1_plus, int32_t f2_plus,
                             int32_t rv, const int32_t* d_rv, int32_t min_iter, int32_t max_iter, int32_t accumulate, float* d_soft,
                             int64_t soft_stride, const ofdm_tb_es_out* out, void* stream) {
    TbDecode d{"ofdm_tb_decode_es_frames", "ofdm_rx_reserve_tb_es", true, min_iter, max_iter, out ? out->cb_iters : nullptr};
    ofdm_tb_out o{};
    if (out) o = ofdm_tb_out{out->payload, out->payload_mode, out->tb_ok, out->cb_ok, out->syndrome};
    return tb_decode(h, d_llr, n_tb, llr_stride, A, Z, G, q, N_IR, f1_minus, f2_minus, f1_plus, f2_plus, rv, d_rv, d, accumulate, d_soft,
                     soft_stride, out ? &o : nullptr, stream);
}

}  // extern "C"
