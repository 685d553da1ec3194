// capi_dft.hip -- DFT-spread OFDM, what both handles hold and what has no handle: the plan cache, the allocation set with the two
// ofdm_*_set_allocations calls ("multi-user allocations of DFT-spread OFDM"), and the queries about sizes,
// plans and output layouts.  The transmitter is in capi_dft_tx.hip, the four receiver families are in capi_despread.hip; what
// the three share is declared in capi_dft.hpp (definition of the calls: include/ofdm_mi355x.h, "DFT-spread OFDM").
#include "capi_dft.hpp"

static_assert(OFDM_MAX_ALLOCS == DFT_MAX_ALLOCS, "the header's cap is the size of the kernels' tables");
void dft_plans_free(DftPlanCache& c) {
    for (int i = 0; i < c.n; ++i) free_dev(&c.d_tw[i]);
    c.n = 0;
}
void dft_alloc_free(DftAllocSet& a) {
    free_dev(&a.d_set, &a.d_tw);
    a = DftAllocSet{};
}
int dft_plan_find(DftPlanCache& c, int M) {
    for (int i = 0; i < c.n; ++i)
        if (c.pl[i].M == M) {
            c.used[i] = ++c.tick;
            return i;
        }
    return -1;
}

namespace {

// builds the plan for M (a size that is ok) into the cache; the least recently used one makes room
template <class H>
int dft_plan_build(H* h, int M, int* slot) {
    DftPlanCache& c = h->dft;
    DftPlan pl;
    dft_make_plan(M, pl);
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
    const int rc = upload(&c.d_tw[c.n], make_twiddles(M));   // e^(-2 pi i j / M): fp64, rounded once
    if (rc != OFDM_OK) {
        free_dev(&c.d_tw[c.n]);
        return rc;
    }
    c.pl[c.n] = pl;
    c.used[c.n] = ++c.tick;
    *slot = c.n++;
    return OFDM_OK;
}
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
            const std::vector<cf> t = make_twiddles(M[u]);  // the table of dft_plan_build
            tw.insert(tw.end(), t.begin(), t.end());
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

}  // namespace

template <class H>
int dft_plan_get(H* h, int M, int* slot) {
    *slot = dft_plan_find(h->dft, M);
    return *slot >= 0 ? OFDM_OK : dft_plan_build(h, M, slot);
}
template int dft_plan_get(ofdm_rx*, int, int*);
template int dft_plan_get(ofdm_tx*, int, int*);

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

}  // extern "C"
