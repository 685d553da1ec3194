// demap_hard.hpp -- hard decisions of the de-mappers (gfx950): BitRecovery's rule per constellation, the packed v_cmp / v_addc
// chains and the bit stores.  Shared by the fused demod kernel (rx_demod.hpp), the pilot stage (rx_pilot.hip) and the stand-alone
// de-mappers (rx_demap.hip).
#pragma once
#include "ofdm_device.hpp"

namespace ofdm {

// BitRecovery's hard decision for float32 inputs (oracle/ofdm_oracle.py:demap_hard has the derivation):
//   QPSK axis bit = 1  iff  -sqrt2 <= x < 0  or  x > sqrt2   ==  (x < 0) xor (|x| > sqrt2_f32)
// valid whenever NEITHER coordinate of the symbol is exactly zero.
__device__ __forceinline__ unsigned qpsk_axis_bit(float x) {
    constexpr float t = 1.41421354f;   // largest float32 below sqrt(2)
    return unsigned(x < 0.f) ^ unsigned(fabsf(x) > t);
}

// A symbol ON an axis (or at the origin) is equidistant, in exact arithmetic, from two (four) constellation points.  The
// reference decides such ties by what its fp64 arithmetic happens to produce (BitRecovery.py:45-52,82-98,105-157), so this
// slow path repeats that arithmetic literally, in double:
//   CDAT  = exp(j 2pi/8 [1,-1,3,5]) as float64 (:45-52) -- not symmetric in the last bit: (bcd,bcc) (bcd,-bcc) (-bcc,bcd) (-bce,-bcc)
//   dist  = |z - CDAT_k| the way NumPy's AVX-512 complex-abs kernel forms it (the recorded reference run, tests/golden/
//           ref_bitrecovery.npz):  max * sqrt(fma(r, r, 1)), r = min / max   -- all correctly rounded IEEE operations
//   k*    = first arg-min (:87);  e = z - CDAT_k* (:93-98)
//   quadrant of z in the reference's order ++, -+, --, +- with >= / <= (first match wins, :106-125) picks which of the
//           metrics -f/2 |e| and -f/2 (K - |e|), K = 1.414213562373095 (:57), is llrp0 / llrp1
//   bit   = int(0.5 (sign(llrp1 - llrp0) + 1)) (:155-156)  ==  [ x(llrp1) < x(llrp0) ]  with x = |e| or K - |e|
//           (the common factor -f/2 is negative; the two x differ by 0, 2 or 4 ulp on a tie, so the products never collapse)
__device__ __noinline__ unsigned qpsk_bits_on_axis(float zx, float zy) {
    constexpr double A = 0x1.6a09e667f3bcdp-1, B = 0x1.6a09e667f3bccp-1, Cc = 0x1.6a09e667f3bcep-1;
    const double cx[4] = {A, A, -B, -Cc};
    const double cy[4] = {B, -B, A, -B};
    constexpr double K = 0x1.6a09e667f3bccp+0;             // the literal 1.414213562373095
    const double x = double(zx), y = double(zy);
    int kbest = 0;
    double dbest = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double ax = fabs(x - cx[k]), ay = fabs(y - cy[k]);
        const double mx = fmax(ax, ay), mn = fmin(ay, ax);
        const double r = mn / mx;                           // mx >= 0.29: no 0/0 here
        const double d = sqrt(fma(r, r, 1.0)) * mx;
        if (k == 0 || d < dbest) {
            dbest = d;
            kbest = k;
        }
    }
    const double ex = fabs(x - cx[kbest]), ey = fabs(y - cy[kbest]);
    const bool q1 = x >= 0.0 && y >= 0.0;
    const bool q2 = !q1 && x <= 0.0 && y >= 0.0;
    const bool q3 = !q1 && !q2 && x <= 0.0 && y <= 0.0;
    const bool q4 = !q1 && !q2 && !q3 && x >= 0.0 && y <= 0.0;
    const bool re_pos = q1 || q4, im_pos = q1 || q2;
    const double fr = K - ex, fi = K - ey;
    const unsigned b0 = re_pos ? (fr < ex) : (ex < fr);
    const unsigned b1 = im_pos ? (fi < ey) : (ey < fi);
    return (b0 << 1) | b1;
}

// bits of one symbol, b0 in the most significant of MOD bits
template <int MOD>
__device__ __forceinline__ unsigned hard_bits(cf z) {
    if constexpr (MOD == 2) {
        if (z.x == 0.f || z.y == 0.f) return qpsk_bits_on_axis(z.x, z.y);      // NaN compares false: closed form below
        return (qpsk_axis_bit(z.x) << 1) | qpsk_axis_bit(z.y);
    } else if constexpr (MOD == 1) {
        return z.x > 0.f;
    } else if constexpr (MOD == 4) {
        constexpr float t = 0.63245553203367588f;   // 2/sqrt(10)
        return (unsigned(z.x < 0.f) << 3) | (unsigned(z.y < 0.f) << 2) | (unsigned(fabsf(z.x) > t) << 1) |
               unsigned(fabsf(z.y) > t);
    } else {
        constexpr float a = 0.61721339984836765f;    // 4/sqrt(42)
        constexpr float c = 0.30860669992418382f;    // 2/sqrt(42)
        return (unsigned(z.x < 0.f) << 5) | (unsigned(z.y < 0.f) << 4) | (unsigned(fabsf(z.x) > a) << 3) |
               (unsigned(fabsf(z.y) > a) << 2) | (unsigned(fabsf(fabsf(z.x) - a) > c) << 1) |
               unsigned(fabsf(fabsf(z.y) - a) > c);
    }
}
__device__ __forceinline__ unsigned hard_bits_rt(cf z, int mod) {
    return mod == 2 ? hard_bits<2>(z) : mod == 1 ? hard_bits<1>(z) : mod == 4 ? hard_bits<4>(z) : hard_bits<6>(z);
}

// Hard bits of 4 consecutive symbols, MSB-first, as one integer (4*MOD bits): the packed de-mapper's inner loop.
// Each decision is a v_cmp into its own SGPR pair and one v_addc_co_u32 that shifts the bit into the word
// (w = 2w + carry): 2 VALU per bit instead of cmp + cndmask + shift + or, and no s_nop between a compare and its
// consumer (gfx950 needs wait states between a VALU writing an SGPR mask and a VALU reading it, so compares are
// issued four to six at a time).  Same float compares as hard_bits<MOD>: results are bit-identical.
template <int MOD, bool ASMB = true>
__device__ __forceinline__ unsigned pack4(const cf (&z)[4]) {
    unsigned w = 0;
    if constexpr (!ASMB) {
        w = (((((hard_bits<MOD>(z[0]) << MOD) | hard_bits<MOD>(z[1])) << MOD) | hard_bits<MOD>(z[2])) << MOD) | hard_bits<MOD>(z[3]);
    } else if constexpr (MOD == 4) {
        constexpr float t = 0.63245553203367588f;   // 2/sqrt(10)
        unsigned long long m0, m1, m2, m3;
#define OFDM_Q16(RE, IM)                                   \
    "v_cmp_gt_f32_e64 %1, 0, " RE "\n\t"                   \
    "v_cmp_gt_f32_e64 %2, 0, " IM "\n\t"                   \
    "v_cmp_gt_f32_e64 %3, |" RE "|, %13\n\t"               \
    "v_cmp_gt_f32_e64 %4, |" IM "|, %13\n\t"               \
    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"             \
    "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"             \
    "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"             \
    "v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\t"
        asm(OFDM_Q16("%5", "%6") OFDM_Q16("%7", "%8") OFDM_Q16("%9", "%10") OFDM_Q16("%11", "%12")
            : "+v"(w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
            : "v"(z[0].x), "v"(z[0].y), "v"(z[1].x), "v"(z[1].y), "v"(z[2].x), "v"(z[2].y), "v"(z[3].x), "v"(z[3].y), "s"(t));
#undef OFDM_Q16
    } else if constexpr (MOD == 6) {
        constexpr float a = 0.61721339984836765f;    // 4/sqrt(42)
        constexpr float c = 0.30860669992418382f;    // 2/sqrt(42)
        unsigned long long m0, m1, m2, m3, m4, m5;
        float tr, ti;
#define OFDM_Q64(RE, IM)                                   \
    "v_sub_f32_e64 %7, |" RE "|, %17\n\t"                  \
    "v_sub_f32_e64 %8, |" IM "|, %17\n\t"                  \
    "v_cmp_gt_f32_e64 %1, 0, " RE "\n\t"                   \
    "v_cmp_gt_f32_e64 %2, 0, " IM "\n\t"                   \
    "v_cmp_gt_f32_e64 %3, |" RE "|, %17\n\t"               \
    "v_cmp_gt_f32_e64 %4, |" IM "|, %17\n\t"               \
    "v_cmp_gt_f32_e64 %5, |%7|, %18\n\t"                   \
    "v_cmp_gt_f32_e64 %6, |%8|, %18\n\t"                   \
    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"             \
    "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"             \
    "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"             \
    "v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\t"             \
    "v_addc_co_u32_e64 %0, %5, %0, %0, %5\n\t"             \
    "v_addc_co_u32_e64 %0, %6, %0, %0, %6\n\t"
        asm(OFDM_Q64("%9", "%10") OFDM_Q64("%11", "%12") OFDM_Q64("%13", "%14") OFDM_Q64("%15", "%16")
            : "+v"(w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&v"(tr), "=&v"(ti)
            : "v"(z[0].x), "v"(z[0].y), "v"(z[1].x), "v"(z[1].y), "v"(z[2].x), "v"(z[2].y), "v"(z[3].x), "v"(z[3].y), "s"(a), "s"(c));
#undef OFDM_Q64
    } else if constexpr (MOD == 2) {
        constexpr float t = 1.41421354f;             // largest float32 below sqrt(2): BitRecovery's outlier edge
        // a coordinate that is exactly zero (a tie of the reference's nearest-point search) takes the literal path.  The
        // product of a group with a zero is 0, or NaN when another coordinate is inf / NaN or the product overflows first
        // (inf * 0): !(|p| > 0) is one compare, as == 0 was, and true for both.
        if (!(fabsf(z[0].x * z[0].y * z[1].x * z[1].y) > 0.f) || !(fabsf(z[2].x * z[2].y * z[3].x * z[3].y) > 0.f)) {
            bool tie = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) tie |= (z[e].x == 0.f) | (z[e].y == 0.f);
            if (tie)
                return (((((hard_bits<2>(z[0]) << 2) | hard_bits<2>(z[1])) << 2) | hard_bits<2>(z[2])) << 2) | hard_bits<2>(z[3]);
        }
        unsigned long long m0, m1, m2, m3, m4, m5, m6, m7;
        // two symbols per group: bit = (x < 0) xor (|x| > sqrt2)
#define OFDM_QPSK2(RE0, IM0, RE1, IM1)                     \
    "v_cmp_gt_f32_e64 %1, 0, " RE0 "\n\t"                  \
    "v_cmp_gt_f32_e64 %2, |" RE0 "|, %17\n\t"              \
    "v_cmp_gt_f32_e64 %3, 0, " IM0 "\n\t"                  \
    "v_cmp_gt_f32_e64 %4, |" IM0 "|, %17\n\t"              \
    "v_cmp_gt_f32_e64 %5, 0, " RE1 "\n\t"                  \
    "v_cmp_gt_f32_e64 %6, |" RE1 "|, %17\n\t"              \
    "v_cmp_gt_f32_e64 %7, 0, " IM1 "\n\t"                  \
    "v_cmp_gt_f32_e64 %8, |" IM1 "|, %17\n\t"              \
    "s_xor_b64 %1, %1, %2\n\t"                             \
    "s_xor_b64 %3, %3, %4\n\t"                             \
    "s_xor_b64 %5, %5, %6\n\t"                             \
    "s_xor_b64 %7, %7, %8\n\t"                             \
    "s_nop 1\n\t"                                          \
    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"             \
    "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"             \
    "v_addc_co_u32_e64 %0, %5, %0, %0, %5\n\t"             \
    "v_addc_co_u32_e64 %0, %7, %0, %0, %7\n\t"
        asm(OFDM_QPSK2("%9", "%10", "%11", "%12") OFDM_QPSK2("%13", "%14", "%15", "%16")
            : "+v"(w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
            : "v"(z[0].x), "v"(z[0].y), "v"(z[1].x), "v"(z[1].y), "v"(z[2].x), "v"(z[2].y), "v"(z[3].x), "v"(z[3].y), "s"(t)
            : "scc");
#undef OFDM_QPSK2
    } else {
        w = (((((hard_bits<MOD>(z[0]) << MOD) | hard_bits<MOD>(z[1])) << MOD) | hard_bits<MOD>(z[2])) << MOD) | hard_bits<MOD>(z[3]);
    }
    return w;
}

// The same for 2 consecutive symbols (2*MOD bits): the dense output mapping hands a lane pairs of list entries.
template <int MOD, bool ASMB = true>
__device__ __forceinline__ unsigned pack2(const cf (&z)[2]) {
    unsigned w = 0;
    if constexpr (!ASMB || MOD == 1) {
        w = (hard_bits<MOD>(z[0]) << MOD) | hard_bits<MOD>(z[1]);
    } else if constexpr (MOD == 4) {
        constexpr float t = 0.63245553203367588f;   // 2/sqrt(10)
        unsigned long long m0, m1, m2, m3;
#define OFDM_Q16(RE, IM)                                   \
    "v_cmp_gt_f32_e64 %1, 0, " RE "\n\t"                   \
    "v_cmp_gt_f32_e64 %2, 0, " IM "\n\t"                   \
    "v_cmp_gt_f32_e64 %3, |" RE "|, %9\n\t"                \
    "v_cmp_gt_f32_e64 %4, |" IM "|, %9\n\t"                \
    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"             \
    "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"             \
    "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"             \
    "v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\t"
        asm(OFDM_Q16("%5", "%6") OFDM_Q16("%7", "%8")
            : "+v"(w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3)
            : "v"(z[0].x), "v"(z[0].y), "v"(z[1].x), "v"(z[1].y), "s"(t));
#undef OFDM_Q16
    } else if constexpr (MOD == 6) {
        constexpr float a = 0.61721339984836765f;    // 4/sqrt(42)
        constexpr float c = 0.30860669992418382f;    // 2/sqrt(42)
        unsigned long long m0, m1, m2, m3, m4, m5;
        float tr, ti;
#define OFDM_Q64(RE, IM)                                   \
    "v_sub_f32_e64 %7, |" RE "|, %13\n\t"                  \
    "v_sub_f32_e64 %8, |" IM "|, %13\n\t"                  \
    "v_cmp_gt_f32_e64 %1, 0, " RE "\n\t"                   \
    "v_cmp_gt_f32_e64 %2, 0, " IM "\n\t"                   \
    "v_cmp_gt_f32_e64 %3, |" RE "|, %13\n\t"               \
    "v_cmp_gt_f32_e64 %4, |" IM "|, %13\n\t"               \
    "v_cmp_gt_f32_e64 %5, |%7|, %14\n\t"                   \
    "v_cmp_gt_f32_e64 %6, |%8|, %14\n\t"                   \
    "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"             \
    "v_addc_co_u32_e64 %0, %2, %0, %0, %2\n\t"             \
    "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"             \
    "v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\t"             \
    "v_addc_co_u32_e64 %0, %5, %0, %0, %5\n\t"             \
    "v_addc_co_u32_e64 %0, %6, %0, %0, %6\n\t"
        asm(OFDM_Q64("%9", "%10") OFDM_Q64("%11", "%12")
            : "+v"(w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&v"(tr), "=&v"(ti)
            : "v"(z[0].x), "v"(z[0].y), "v"(z[1].x), "v"(z[1].y), "s"(a), "s"(c));
#undef OFDM_Q64
    } else {                                         // MOD == 2
        constexpr float t = 1.41421354f;             // largest float32 below sqrt(2): BitRecovery's outlier edge
        // a coordinate that is exactly zero (a tie of the reference's nearest-point search) takes the literal path
        // (0 or NaN product: see pack4)
        if (!(fabsf(z[0].x * z[0].y * z[1].x * z[1].y) > 0.f)) {
            const bool tie = (z[0].x == 0.f) | (z[0].y == 0.f) | (z[1].x == 0.f) | (z[1].y == 0.f);
            if (tie) return (hard_bits<2>(z[0]) << 2) | hard_bits<2>(z[1]);
        }
        unsigned long long m0, m1, m2, m3, m4, m5, m6, m7;
        asm("v_cmp_gt_f32_e64 %1, 0, %9\n\t"
            "v_cmp_gt_f32_e64 %2, |%9|, %13\n\t"
            "v_cmp_gt_f32_e64 %3, 0, %10\n\t"
            "v_cmp_gt_f32_e64 %4, |%10|, %13\n\t"
            "v_cmp_gt_f32_e64 %5, 0, %11\n\t"
            "v_cmp_gt_f32_e64 %6, |%11|, %13\n\t"
            "v_cmp_gt_f32_e64 %7, 0, %12\n\t"
            "v_cmp_gt_f32_e64 %8, |%12|, %13\n\t"
            "s_xor_b64 %1, %1, %2\n\t"
            "s_xor_b64 %3, %3, %4\n\t"
            "s_xor_b64 %5, %5, %6\n\t"
            "s_xor_b64 %7, %7, %8\n\t"
            "s_nop 1\n\t"
            "v_addc_co_u32_e64 %0, %1, %0, %0, %1\n\t"
            "v_addc_co_u32_e64 %0, %3, %0, %0, %3\n\t"
            "v_addc_co_u32_e64 %0, %5, %0, %0, %5\n\t"
            "v_addc_co_u32_e64 %0, %7, %0, %0, %7\n\t"
            : "+v"(w), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
            : "v"(z[0].x), "v"(z[0].y), "v"(z[1].x), "v"(z[1].y), "s"(t)
            : "scc");
    }
    return w;
}

// one-bit-per-byte output of the PAIR of list entries sym0, sym0 + 1 held by one lane (dense output mapping)
template <int MOD>
__device__ __forceinline__ void store_bits_pair_unpacked(uint8_t* row, unsigned sym0, const cf (&z)[2]) {
    uint8_t* o = row + sym0 * unsigned(MOD);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const unsigned hb = hard_bits<MOD>(z[e]);
#pragma unroll
        for (int b = 0; b < MOD; ++b) o[e * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
    }
}

// the 4*MOD bits `w` of the list entries sym0 .. sym0 + 3 (sym0 % 4 == 0), MSB first, as MOD/2 bytes
// `row` = address of the row's first byte (the caller folds everything wave-uniform into it), sym0 = entry index within the row
template <int MOD>
__device__ __forceinline__ void store_packed4(uint8_t* row, unsigned sym0, unsigned w) {
    uint8_t* o = row + (sym0 >> 2) * unsigned(MOD / 2);
    if constexpr (MOD == 2) {
        o[0] = uint8_t(w);
    } else if constexpr (MOD == 4) {
        *reinterpret_cast<uint16_t*>(o) = uint16_t(((w & 0xffu) << 8) | (w >> 8));
    } else {
        o[0] = uint8_t(w >> 16);
        o[1] = uint8_t(w >> 8);
        o[2] = uint8_t(w);
    }
}

// writes the bits of 4 (or `cnt`) consecutive list entries starting at list index idx of output row `orow`
template <int MOD, int BMODE, bool ASMB = true>
__device__ __forceinline__ void store_bits(uint8_t* bits, int64_t sym0, const cf (&z)[4], int cnt) {
    if constexpr (BMODE == 1) {            // packed MSB-first: 4 symbols -> MOD/2 bytes (host guarantees Kd % 4 == 0, MOD even)
        store_packed4<MOD>(bits + (sym0 >> 2) * (MOD / 2), 0u, pack4<MOD, ASMB>(z));
    } else if constexpr (BMODE == 2) {     // one bit per byte
        uint8_t* o = bits + sym0 * MOD;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < cnt) {
                const unsigned hb = hard_bits<MOD>(z[e]);
#pragma unroll
                for (int b = 0; b < MOD; ++b) o[e * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
            }
        }
    }
}

}  // namespace ofdm
