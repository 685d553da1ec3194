// Host-side lane-by-lane execution of csrc/dft_mixed.hpp (no GPU): every plan's index logic, butterflies and twiddles, checked
// against numpy.fft in tests/test_dft_mixed_host.py.
// usage: dft_mixed_host_test in.bin out.bin M1 [M2 ...]
//   in.bin  complex64 little-endian: M1 points, then M2 points, ...
//   out.bin per size: the forward transform (M bins), then the inverse transform of the same input (M points), both with 1/sqrt(M)
//   stdout  one line per size: M n_pass lanes rows_per_group pad row_elems radix...
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lte-gnu-radio-code_amd/csrc/dft_mixed.hpp"

using namespace ofdm;

// what a workgroup does with one row: the lanes take turns where the device has a barrier
static void transform(const DftPlan& pl, const std::vector<cf>& tw, const cf* in, cf* out, bool inverse) {
    std::vector<cf> lds(size_t(pl.row_elems), cf{0.f, 0.f});
    for (int i = 0; i < pl.M; ++i) lds[size_t(dft_phys(i, pl.pad))] = inverse ? cconj(in[i]) : in[i];
    std::vector<cf> regs(size_t(pl.lanes) * DFT_MAX_REGS);
    auto V = [&](int t) -> cf(&)[DFT_MAX_REGS] { return *reinterpret_cast<cf(*)[DFT_MAX_REGS]>(&regs[size_t(t) * DFT_MAX_REGS]); };
    int s = 1;
    for (int p = 0; p < pl.n_pass; ++p) {
        const int r = pl.radix[p];
        if (pl.M <= DFT_SMALL_M) {                                    // the class the device launches for this size
            for (int t = 0; t < pl.lanes; ++t) dft_pass_load_rt<DFT_SMALL_M>(pl, r, s, t, lds.data(), tw.data(), V(t));
            for (int t = 0; t < pl.lanes; ++t) dft_pass_store_rt<DFT_SMALL_M>(pl, r, s, t, lds.data(), V(t));
        } else {
            for (int t = 0; t < pl.lanes; ++t) dft_pass_load_rt<DFT_MAX_M>(pl, r, s, t, lds.data(), tw.data(), V(t));
            for (int t = 0; t < pl.lanes; ++t) dft_pass_store_rt<DFT_MAX_M>(pl, r, s, t, lds.data(), V(t));
        }
        s *= r;
    }
    for (int i = 0; i < pl.M; ++i) {
        const cf x = lds[size_t(dft_phys(i, pl.pad))] * pl.scale;
        out[i] = inverse ? cconj(x) : x;
    }
}

int main(int argc, char** argv) {
    if (argc < 4) return 1;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    for (int a = 3; a < argc; ++a) {
        const int M = atoi(argv[a]);
        DftPlan pl;
        if (!dft_make_plan(M, pl)) return 3;
        const size_t n = size_t(M);
        std::vector<cf> x(n), y(n), tw(n);
        if (fread(x.data(), sizeof(cf), size_t(M), fi) != size_t(M)) return 4;
        for (int j = 0; j < M; ++j) {
            const double ang = -2.0 * M_PI * j / M;
            tw[size_t(j)] = cf{float(cos(ang)), float(sin(ang))};
        }
        for (int dir = 0; dir < 2; ++dir) {
            transform(pl, tw, x.data(), y.data(), dir == 1);
            fwrite(y.data(), sizeof(cf), size_t(M), fo);
        }
        printf("%d %d %d %d %d %d", pl.M, pl.n_pass, pl.lanes, pl.rows_per_group, pl.pad, pl.row_elems);
        for (int p = 0; p < pl.n_pass; ++p) printf(" %d", pl.radix[p]);
        printf("\n");
    }
    fclose(fi);
    fclose(fo);
    return 0;
}
