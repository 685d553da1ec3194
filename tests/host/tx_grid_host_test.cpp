// Host-side check of csrc/tx_grid.hpp (no GPU): the workgroup count of the fused transmit kernel over every edge of its
// arguments.  Prints one line per violated property and returns 1 if there was any; tests/test_tx_grid_host.py runs it.
//
// -DTX_GRID_TEST_PARENT_FORMULA swaps in the expression the launcher used before the grid choice became a function of its own
// (coprimality asked of g * slots): with slots sharing a factor with S + D that loop only ends at 1, and the pytest file shows
// that the properties below catch it.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "../../lte-gnu-radio-code_amd/csrc/tx_grid.hpp"

static int64_t gcd64(int64_t x, int64_t y) {
    while (y) {
        const int64_t r = x % y;
        x = y;
        y = r;
    }
    return x;
}

static int64_t grid_under_test(int64_t wgs, int64_t resident, int slots, int64_t SD) {
#ifdef TX_GRID_TEST_PARENT_FORMULA
    if (wgs == 0) return 0;
    int64_t g0 = std::min<int64_t>(wgs, wgs >= resident * OFDM_TX_GRID_MULT * 16 ? resident * OFDM_TX_GRID_MULT : resident);
    if (g0 < wgs)
        while (g0 > 1 && gcd64(g0 * slots, SD) != 1) --g0;
    return g0;
#else
    return ofdm::tx_modulate_grid(wgs, resident, slots, SD);
#endif
}

int main() {
    int bad = 0;
    long cases = 0;
    auto fail = [&](const char* what, int64_t wgs, int64_t resident, int slots, int64_t SD, int64_t base, int64_t g) {
        std::printf("FAIL %s: slots=%d SD=%lld resident=%lld wgs=%lld base=%lld g=%lld\n", what, slots, (long long)SD,
                    (long long)resident, (long long)wgs, (long long)base, (long long)g);
        ++bad;
    };
    const int64_t sds[] = {2, 3, 4, 5, 6, 7, 8, 9, 70000};
    for (int slots : {1, 2, 4, 8})
        for (int64_t SD : sds)
            for (int64_t resident : {1, 2, 255, 256, 1024, 4096, 8192})
                for (int64_t wgs : {int64_t(0), int64_t(1), resident - 1, resident, resident + 1, 3 * resident + 1, 256 * resident,
                                    256 * resident + 1}) {
                    ++cases;
                    // the unadjusted value, restated: the resident workgroups, or OFDM_TX_GRID_MULT times as many from
                    // 16 * OFDM_TX_GRID_MULT * resident workgroups of work on
                    const bool large = wgs >= resident * OFDM_TX_GRID_MULT * 16;
                    const int64_t cap = large ? resident * OFDM_TX_GRID_MULT : resident;
                    const int64_t base = wgs < cap ? wgs : cap;
                    const int64_t g = grid_under_test(wgs, resident, slots, SD);
                    if (g < 0 || g > wgs || (wgs >= 1 && g < 1)) fail("range", wgs, resident, slots, SD, base, g);
                    if (wgs <= resident) {
                        if (g != wgs) fail("one trip", wgs, resident, slots, SD, base, g);
                    } else if (!(g > base - SD)) {
                        fail("within SD of base", wgs, resident, slots, SD, base, g);
                    }
                    if (slots == 1 && g < wgs && gcd64(g, SD) != 1) fail("coprime", wgs, resident, slots, SD, base, g);
                }
    std::printf("%ld cases, %d violations\n", cases, bad);
    return bad ? 1 : 0;
}
