// dft_mixed.hpp -- mixed-radix DFT of one row of M = 2^a 3^b 5^c <= 4096 complex points in LDS (gfx950): the transform behind
// DFT-spread OFDM (dft_spread.hip).
//
// A row is transformed by T cooperating lanes (a power of two, T >= M/4 up to 256) in Stockham autosort passes of radix 3, 5, 4
// and 2, decimation in frequency, so that no digit-reversal pass is needed.  With s = the product of the radices already done,
// butterfly b < M/R of a radix-R pass is (p, q) = (b / s, b % s):
//     reads   x[b + (M/R) k]                       k < R    consecutive lanes read consecutive elements in every pass
//     writes  y[q + s (R p + k)] = W_M^(s p k) * sum_j x_j W_R^(j k)
// x and y are the SAME buffer: every lane first reads all its butterflies into registers (dft_pass_load), the row's lanes meet
// at a barrier, then every lane writes (dft_pass_store).  Twiddles come from one table W_M^j = e^(-2 pi i j / M), j < M, built
// on the host in fp64 and rounded once; s p k < M, so the index needs no reduction.  The transform itself is always the
// forward one: the inverse is conj(forward(conj(x))), which the callers fold into their load and store (the conjugated
// table, applied to the data instead).  The 1 / sqrt(M) of both directions is the caller's as well (DftPlan::scale).
//
// LDS layout: element i of a row lives at i + pad * (i >> 5).  Reads are unit-stride over the lanes in every pass, so only the
// writes can collide.  Odd radices run first: once s has an odd factor the runs q + s R p of 16 consecutive lanes fall on
// distinct 8-byte slots.  A power of two has no odd factor, and there the radix-4 writes of 16 lanes (s = 1, 2, 4) span 64
// elements with period 4 s: the second 32 would land on the first.  pad = 6 moves them by 6 slots, into the holes of all three
// patterns (6 = 2 mod 4, 6..7 mod 8, 6..9 mod 16).  Every other M has pad = 0: a pad would only misalign its reads.
//
// Everything here is __host__ __device__: tests/host/dft_mixed_host_test.cpp runs every plan lane by lane on the CPU.
#pragma once
#include "fft_core.hpp"

namespace ofdm {

constexpr int DFT_MAX_M = 4096;
constexpr int DFT_MAX_PASS = 8;          // 3^7 = 2187 has the most passes
constexpr int DFT_THREADS = 256;         // lanes of a workgroup: rows_per_group rows of T lanes
constexpr int DFT_PAD_POW2 = 6;
constexpr int DFT_LDS_ELEMS = DFT_MAX_M + DFT_PAD_POW2 * (DFT_MAX_M >> 5);   // 4864 complex = 38 KB

struct DftPlan {
    int M;
    int n_pass;
    int radix[DFT_MAX_PASS];
    int lanes;               // T
    int rows_per_group;      // DFT_THREADS / T
    int pad;                 // 8-byte slots added per 32 elements
    int row_elems;           // LDS elements of a row, pad included
    float scale;             // float(1 / sqrt(M))
};

// Butterflies a lane may own in a radix-R pass of a plan with M <= CAP: ceil(ceil(CAP / R) / 256).  The passes are compiled
// twice, for M <= DFT_SMALL_M and for every M: a lane that may hold 20 complex values costs 186 VGPRs (two waves per SIMD),
// one that holds at most 10 costs about 100 (four), and the small class has the sizes of the numerologies (60 ... 1200).
constexpr int DFT_SMALL_M = 2048;
template <int R, int CAP>
struct DftLaneWork {
    static constexpr int MAXB = ((CAP + R - 1) / R + DFT_THREADS - 1) / DFT_THREADS;
    static constexpr int REGS = MAXB * R;
};
constexpr int DFT_MAX_REGS = 20;         // the largest REGS (radix 5, CAP = DFT_MAX_M)

OFDM_HD bool dft_size_ok(int M) {
    if (M < 1 || M > DFT_MAX_M) return false;
    while (M % 2 == 0) M /= 2;
    while (M % 3 == 0) M /= 3;
    while (M % 5 == 0) M /= 5;
    return M == 1;
}

// false: M is not of the form 2^a 3^b 5^c in 1 .. 4096
inline bool dft_make_plan(int M, DftPlan& pl) {
    pl = DftPlan{};
    if (!dft_size_ok(M)) return false;
    pl.M = M;
    int m = M, np = 0;
    while (m % 3 == 0) { pl.radix[np++] = 3; m /= 3; }
    while (m % 5 == 0) { pl.radix[np++] = 5; m /= 5; }
    const bool pow2 = m == M;
    while (m % 4 == 0) { pl.radix[np++] = 4; m /= 4; }
    if (m == 2) pl.radix[np++] = 2;
    pl.n_pass = np;
    int T = 1;
    while (T < DFT_THREADS && 4 * T < M) T *= 2;
    pl.lanes = T;
    pl.rows_per_group = DFT_THREADS / T;
    pl.pad = pow2 && M >= 64 ? DFT_PAD_POW2 : 0;
    pl.row_elems = M + pl.pad * ((M + 31) >> 5);
    pl.scale = float(1.0 / __builtin_sqrt(double(M)));
    return true;
}

OFDM_HD int dft_phys(int i, int pad) { return i + pad * (i >> 5); }

// forward butterflies, in place
OFDM_HD cf dft_mul_mi(cf a) { return cf{a.y, -a.x}; }            // -i a
OFDM_HD void dft_bfly2(cf* v) {
    const cf a = v[0], b = v[1];
    v[0] = a + b;
    v[1] = a - b;
}
OFDM_HD void dft_bfly3(cf* v) {
    constexpr float S3 = 0.86602540378443865f;                   // sin(pi / 3)
    const cf t1 = v[1] + v[2];
    const cf t2 = v[0] - t1 * 0.5f;
    const cf t3 = dft_mul_mi((v[1] - v[2]) * S3);
    v[0] = v[0] + t1;
    v[1] = t2 + t3;
    v[2] = t2 - t3;
}
OFDM_HD void dft_bfly4(cf* v) {
    const cf t0 = v[0] + v[2], t1 = v[0] - v[2], t2 = v[1] + v[3], t3 = dft_mul_mi(v[1] - v[3]);
    v[0] = t0 + t2;
    v[1] = t1 + t3;
    v[2] = t0 - t2;
    v[3] = t1 - t3;
}
OFDM_HD void dft_bfly5(cf* v) {
    constexpr float C1 = 0.30901699437494742f, C2 = -0.80901699437494742f;   // cos(2 pi / 5), cos(4 pi / 5)
    constexpr float S1 = 0.95105651629515357f, S2 = 0.58778525229247313f;    // sin(2 pi / 5), sin(4 pi / 5)
    const cf t1 = v[1] + v[4], t2 = v[2] + v[3], t3 = v[1] - v[4], t4 = v[2] - v[3];
    const cf m1 = v[0] + t1 * C1 + t2 * C2, m2 = v[0] + t1 * C2 + t2 * C1;
    const cf n1 = dft_mul_mi(t3 * S1 + t4 * S2), n2 = dft_mul_mi(t3 * S2 - t4 * S1);
    v[0] = v[0] + t1 + t2;
    v[1] = m1 + n1;
    v[4] = m1 - n1;
    v[2] = m2 + n2;
    v[3] = m2 - n2;
}
template <int R>
OFDM_HD void dft_bfly(cf* v) {
    if constexpr (R == 2) dft_bfly2(v);
    if constexpr (R == 3) dft_bfly3(v);
    if constexpr (R == 4) dft_bfly4(v);
    if constexpr (R == 5) dft_bfly5(v);
}

// First half of a radix-R pass for one lane of the row at `row`: its butterflies b = lane, lane + T, ... read, transformed
// and multiplied by their twiddles, left in v (R per butterfly).  s = the product of the radices of the earlier passes.
template <int R, int CAP>
OFDM_HD void dft_pass_load(const DftPlan& pl, int s, int lane, const cf* row, const cf* tw, cf (&v)[DFT_MAX_REGS]) {
    const int nb = pl.M / R;
#pragma unroll
    for (int i = 0; i < DftLaneWork<R, CAP>::MAXB; ++i) {
        const int b = lane + i * pl.lanes;
        if (b < nb) {
            cf* x = &v[i * R];
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = row[dft_phys(b + nb * k, pl.pad)];
            dft_bfly<R>(x);
            const int sp = (b / s) * s;                              // s p
#pragma unroll
            for (int k = 1; k < R; ++k) x[k] = cmul(x[k], tw[sp * k]);
        }
    }
}
// Second half, after every lane of the row has finished dft_pass_load
template <int R, int CAP>
OFDM_HD void dft_pass_store(const DftPlan& pl, int s, int lane, cf* row, const cf (&v)[DFT_MAX_REGS]) {
    const int nb = pl.M / R;
#pragma unroll
    for (int i = 0; i < DftLaneWork<R, CAP>::MAXB; ++i) {
        const int b = lane + i * pl.lanes;
        if (b < nb) {
            const int p = b / s, q = b - p * s;
#pragma unroll
            for (int k = 0; k < R; ++k) row[dft_phys(q + s * (R * p + k), pl.pad)] = v[i * R + k];
        }
    }
}
// the two halves by the plan's radix (the switch is uniform over the workgroup); CAP >= pl.M
template <int CAP>
OFDM_HD void dft_pass_load_rt(const DftPlan& pl, int r, int s, int lane, const cf* row, const cf* tw, cf (&v)[DFT_MAX_REGS]) {
    switch (r) {
        case 2: dft_pass_load<2, CAP>(pl, s, lane, row, tw, v); break;
        case 3: dft_pass_load<3, CAP>(pl, s, lane, row, tw, v); break;
        case 4: dft_pass_load<4, CAP>(pl, s, lane, row, tw, v); break;
        default: dft_pass_load<5, CAP>(pl, s, lane, row, tw, v); break;
    }
}
template <int CAP>
OFDM_HD void dft_pass_store_rt(const DftPlan& pl, int r, int s, int lane, cf* row, const cf (&v)[DFT_MAX_REGS]) {
    switch (r) {
        case 2: dft_pass_store<2, CAP>(pl, s, lane, row, v); break;
        case 3: dft_pass_store<3, CAP>(pl, s, lane, row, v); break;
        case 4: dft_pass_store<4, CAP>(pl, s, lane, row, v); break;
        default: dft_pass_store<5, CAP>(pl, s, lane, row, v); break;
    }
}

}  // namespace ofdm
