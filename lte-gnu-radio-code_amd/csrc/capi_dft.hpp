// capi_dft.hpp -- what the three host units of DFT-spread OFDM share: capi_dft.hip (the plan cache and the allocation set, which
// defines what is declared here), capi_dft_tx.hip (the transmitter) and capi_despread.hip (the four receiver families).
#pragma once
#include "capi_internal.hpp"

#pragma GCC visibility push(hidden)
int dft_plan_find(DftPlanCache& c, int M);       // the slot of M's plan, or -1
// Find, else build (the least recently used plan makes room: a build can move slots, so a slot from before it is stale).
template <class H>
int dft_plan_get(H* h, int M, int* slot);
#pragma GCC visibility pop

namespace {

const char* dft_bad_size(int32_t M) { return dft_size_ok(M) ? "" : "M must be 2^a 3^b 5^c in 1 .. 4096"; }
bool dft_rows_in_range(const DftPlan& pl, int64_t rows, int64_t n_seg) {
    const int64_t groups = (rows + pl.rows_per_group - 1) / pl.rows_per_group;
    return n_seg <= 0 || groups <= DFT_MAX_GROUPS / n_seg;
}
// The ensure step of a call that needs the plan for M and a workspace: both there, or both through `reserve` -- outside a
// capture -- and the slot found again behind it.
template <class Reserve>
int dft_plan_ensure(DftPlanCache& c, int M, bool ws_fits, hipStream_t s, const char* who, const char* reserve_name, Reserve reserve,
                    int* slot) {
    *slot = dft_plan_find(c, M);
    if (*slot >= 0 && ws_fits) return OFDM_OK;
    const int rc = grow_outside_capture(false, s, who, reserve_name, reserve);
    if (rc == OFDM_OK) *slot = dft_plan_find(c, M);
    return rc;
}

}  // namespace
