// tx_grid.hpp -- how many workgroups the fused transmit kernel (tx_modulate_kernel) is launched with.  Plain host arithmetic, no
// HIP: launch_mod_nk (tx_kernels.hip) calls it with what the runtime reports, tests/host/tx_grid_host_test.cpp with every edge.
#pragma once
#include <algorithm>
#include <cstdint>

#ifndef OFDM_TX_GRID_MULT
#define OFDM_TX_GRID_MULT 16
#endif

namespace ofdm {

// wgs       workgroups the launch has work for: ceil(symbols / slots)
// resident  workgroups the chip holds at once (compute units x the occupancy the runtime reports for the kernel)
// slots     symbols a workgroup handles side by side (Plan<N>::SLOTS)
// SD        length S + D of the sync/data pattern
inline int64_t tx_modulate_grid(int64_t wgs, int64_t resident, int slots, int64_t SD) {
    if (wgs <= 0) return 0;
    // Exactly the workgroups that are resident at once, the rest is looped: a grid larger than that runs in waves of workgroups,
    // and the last, partly filled wave of a looping kernel costs a whole loop's time on a fraction of the chip (2 048 workgroups
    // with 1 536 resident: +50 %) ...
    // ... unless the launch is large enough for MANY such waves of workgroups: then the tail is a sixteenth of the work and the
    // dispatcher's refilling of freed slots beats the fixed assignment (+2-8 % at the bench's batch sizes; a workgroup still walks
    // >= 16 symbols, so its tables stay amortised; at 512 frames the exactly-resident grid is as good or better and is kept)
    int64_t g = std::min<int64_t>(wgs, wgs >= resident * OFDM_TX_GRID_MULT * 16 ? resident * OFDM_TX_GRID_MULT : resident);
    // A workgroup walks symbols first, first + stride, ...: with a stride that is a multiple of the [S, D] pattern length it would
    // meet the same position of the pattern every time.  That matters only where a workgroup holds one symbol, since only there are
    // sync symbols copied instead of transformed (a quarter of the workgroups would do nothing but copy): keep the grid coprime
    // with the pattern length.  One of any SD consecutive integers is 1 mod SD, so this takes fewer than SD steps.
    // With several symbols per workgroup every symbol costs the same and the stride g * slots could not be made coprime with an
    // SD that shares a factor with slots anyway: the grid stays as it is.
    if (g < wgs && slots == 1) {
        auto gcd = [](int64_t x, int64_t y) { while (y) { const int64_t r_ = x % y; x = y; y = r_; } return x; };
        while (g > 1 && gcd(g, SD) != 1) --g;
    }
    return g;
}

}  // namespace ofdm
