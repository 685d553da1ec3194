// rx_pilot.hip -- gfx950 kernels of the pilot-aided phase-tracking stage (ofdm_pilot_track_frames).
//
//   pilot_track_kernel  per row of K equalised symbols: pilot sum U, rotator c = conj(U)/|U| (+ a phase line over the pilot
//                       offsets in slope mode), de-rotated data row without the pilot entries, hard bits, cpe, slope
//   pilot_cfo_kernel    per segment: arg of the sum of U[s+1] conj(U[s]) over consecutive rows of one pattern -> carrier offset
//
// No reference code exists for this stage; the definition is include/ofdm_mi355x.h (tests/pilot_ref.py restates it in fp64).
// The stage is memory-bound: a row is read once (the pilot entries a second time, from cache) and written once.  Nothing is
// added atomically and every sum has an order that depends on the row or on the segment's geometry only.
#include "rx_demod.hpp"

namespace ofdm {

namespace {

// v of lane ^ 1 (quad_perm:[1,0,3,2]).  Every lane of the wave has to be active.
__device__ __forceinline__ unsigned lane_xor1(unsigned v) {
    return unsigned(__builtin_amdgcn_update_dpp(0, int(v), 0xB1, 0xF, 0xF, false));
}

// Work split: a row belongs to a group of G = 2^g_log2 lanes of ONE wave (G = 64 for rows of 128 data entries and more, so that
// a 64-point row of 56 entries leaves no half-empty wave), a group walks rows_per_group consecutive rows, and the grid holds
// exactly as many workgroups as that takes: a workgroup's share is about 16 KB whatever the row length.  A lane owns the PAIR of
// consecutive outputs (2q, 2q+1), q = pass*G + lane-in-group: the outputs leave as one aligned 16 B store per lane, the inputs
// -- shifted against the outputs by the number of pilots passed so far -- arrive as two 8 B loads whose addresses come from
// the src table (the second load of a line is an L1 hit).  The group's first lanes fetch the pilots BEFORE the first batch of the
// row is requested, and the batch is in flight while the pilot sum is formed.  The sum is taken in ascending pilot order by
// every lane of the group (cross-lane reads), so all lanes hold the same rotator and no LDS or barrier is involved.
// MOD: 0 = no bits, else bits per symbol of the hard decision.  SLOPE: OFDM_PILOT_CPE_SLOPE.
template <int MOD, bool SLOPE>
__global__ void __launch_bounds__(256) pilot_track_kernel(PilotArgs a) {
    constexpr int UNR = 2;                                            // output pairs a lane has in flight
    const int G = 1 << a.g_log2;
    const int lane = threadIdx.x & 63, l = lane & (G - 1), gbase = lane - l;
    const int64_t group = (int64_t(blockIdx.x) * 256 + threadIdx.x) >> a.g_log2;
    const int64_t total = a.n_seg * a.rows;
    const int npairs = (a.Kd + 1) >> 1;
    const int half = a.K >> 1;
    for (int it = 0; it < a.rows_per_group; ++it) {
        const int64_t R = group * a.rows_per_group + it;              // row of the whole call; ascending with the lane
        const bool rv = R < total;
        if (__ballot(rv) == 0) break;                                 // wave-uniform: nobody leaves a cross-lane read alone
        const int64_t seg = rv ? R / a.rows : 0;
        const cf* row = a.sym + seg * a.seg_stride + (R - seg * a.rows) * a.K;      // only dereferenced under rv
        cf zp = (rv && l < a.n_pilots) ? row[a.pidx[l]] : cf{0.f, 0.f};

        int si[UNR][2] = {};
        cf z[UNR][2] = {};
        auto load_batch = [&](int q0) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int q = q0 + u * G + l;
                const bool v0 = rv && 2 * q < a.Kd, v1 = rv && 2 * q + 1 < a.Kd;
                const unsigned s2 = v0 ? *reinterpret_cast<const unsigned*>(a.src + 2 * q) : 0u;     // table padded to even
                si[u][0] = int(s2 & 0xffffu);
                si[u][1] = int(s2 >> 16);
                z[u][0] = v0 ? row[si[u][0]] : cf{0.f, 0.f};
                z[u][1] = v1 ? row[si[u][1]] : cf{0.f, 0.f};
            }
        };
        if (a.data) load_batch(0);

        // U = sum_p z[p] conj(pilot), ascending p, fp32
        float ur = 0.f, ui = 0.f;
        for (int p0 = 0; p0 < a.n_pilots; p0 += G) {
            if (p0 > 0) zp = (rv && p0 + l < a.n_pilots) ? row[a.pidx[p0 + l]] : cf{0.f, 0.f};
            const cf w = cmul(zp, a.pilot_conj);
            const int cnt = min(G, a.n_pilots - p0);
            for (int i = 0; i < cnt; ++i) {
                ur += __shfl(w.x, gbase + i, 64);
                ui += __shfl(w.y, gbase + i, 64);
            }
        }
        const float n2 = ur * ur + ui * ui;
        const bool usable = n2 > 0.f && n2 < INFINITY;                // NaN fails both
        const float inv = usable ? 1.0f / sqrtf(n2) : 0.f;
        const cf c = usable ? cf{ur * inv, -ui * inv} : cf{1.f, 0.f};

        float tau = 0.f, delta = 0.f;
        if constexpr (SLOPE) {
            // theta_p = arg(z[p] conj(pilot) c); tau = sum (k_p - kbar) theta_p / sum (k_p - kbar)^2, delta = mean theta - tau kbar
            float st = 0.f, skt = 0.f;
            for (int p0 = 0; p0 < a.n_pilots; p0 += G) {
                const int p = p0 + l;
                const bool pv = rv && p < a.n_pilots;
                const cf zq = pv ? row[a.pidx[p]] : cf{0.f, 0.f};
                const cf w = cmul(cmul(zq, a.pilot_conj), c);
                const float th = pv ? atan2f(w.y, w.x) : 0.f;
                const float kt = pv ? (a.pk[p] - a.kbar) * th : 0.f;
                const int cnt = min(G, a.n_pilots - p0);
                for (int i = 0; i < cnt; ++i) {
                    st += __shfl(th, gbase + i, 64);
                    skt += __shfl(kt, gbase + i, 64);
                }
            }
            if (usable) {
                tau = skt * a.inv_skk;
                delta = st / float(a.n_pilots) - tau * a.kbar;
            }
        }
        if (rv && l == 0) {
            if (a.cpe) a.cpe[R] = usable ? cf{ur * inv, ui * inv} : cf{0.f, 0.f};
            if (a.usum) a.usum[R] = usable ? cf{ur, ui} : cf{0.f, 0.f};
            if (SLOPE && a.slope_out) a.slope_out[R] = tau;
        }
        if (!a.data) continue;                                        // uniform

        // c e^{-j(delta + tau k)} for list index i (k = signed bin offset): hardware sin / cos of the phase in revolutions,
        // reduced to [-1/2, 1/2]
        auto rotor = [&](int i) {
            const float k = float(i - half + (i >= half ? 1 : 0));
            float rev = (delta + tau * k) * 0.15915494309189535f;
            rev -= rintf(rev);
            return cmul(c, cf{__builtin_amdgcn_cosf(rev), -__builtin_amdgcn_sinf(rev)});
        };
        for (int q0 = 0; q0 < npairs; q0 += G * UNR) {
            if (q0 > 0) load_batch(q0);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int q = q0 + u * G + l, j0 = 2 * q;
                const bool v0 = rv && j0 < a.Kd, v1 = rv && j0 + 1 < a.Kd;
                cf o0, o1;
                if constexpr (SLOPE) {
                    o0 = cmul(rotor(si[u][0]), z[u][0]);
                    o1 = cmul(rotor(si[u][1]), z[u][1]);
                } else {
                    o0 = cmul(c, z[u][0]);
                    o1 = cmul(c, z[u][1]);
                }
                cf* dst = a.data + (R * a.Kd + j0);
                if (v1 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                    typedef float f4 __attribute__((ext_vector_type(4)));
                    __builtin_nontemporal_store(f4{o0.x, o0.y, o1.x, o1.y}, reinterpret_cast<f4*>(dst));
                } else {
                    if (v0) dst[0] = o0;
                    if (v1) dst[1] = o1;
                }
                if constexpr (MOD != 0) {
                    // bits of the STORED values, b0 first; pw = this lane's my_n * MOD bits, first symbol on top
                    const unsigned h0 = v0 ? hard_bits<MOD>(o0) : 0u, h1 = v1 ? hard_bits<MOD>(o1) : 0u;
                    const unsigned my_n = unsigned(v0) + unsigned(v1);
                    const unsigned pw = v1 ? ((h0 << MOD) | h1) : h0;
                    if (a.bits_mode == 1) {                           // OFDM_BITS_PACKED: the even lane stores the pair of pairs
                        const unsigned nw = lane_xor1(pw), nn = lane_xor1(my_n);
                        if ((l & 1) == 0 && my_n > 0) {
                            const unsigned word = (pw << (nn * MOD)) | nw;
                            const int nbits = int(my_n + nn) * MOD;   // a multiple of 8: the caller checked Kd * MOD % 8 == 0
                            uint8_t* bp = a.bits + (((R * a.Kd + j0) * MOD) >> 3);
#pragma unroll
                            for (int b = 0; b < MOD / 2; ++b)
                                if (8 * (b + 1) <= nbits) bp[b] = uint8_t(word >> (nbits - 8 * (b + 1)));
                        }
                    } else {                                          // one bit per byte
                        uint8_t* bp = a.bits + (R * a.Kd + j0) * MOD;
                        if (v1 && (reinterpret_cast<uintptr_t>(bp) & 3) == 0) {
#pragma unroll
                            for (int k = 0; k < MOD / 2; ++k) {
                                uint32_t w = 0u;
#pragma unroll
                                for (int e = 0; e < 4; ++e) w |= ((pw >> (2 * MOD - 1 - (4 * k + e))) & 1u) << (8 * e);
                                reinterpret_cast<uint32_t*>(bp)[k] = w;
                            }
                        } else {
                            const int nby = int(my_n) * MOD;
                            for (int i = 0; i < nby; ++i) bp[i] = uint8_t((pw >> (nby - 1 - i)) & 1u);
                        }
                    }
                }
            }
        }
    }
}

// One wave per segment.  Lane l adds the pairs (s, s+1), s = l, l + 64, ..., in ascending s in fp64 (the products of two floats
// are exact in double), then the 64 lane sums are added by a butterfly: the order depends on rows and rows_per_pattern only.
__global__ void __launch_bounds__(64) pilot_cfo_kernel(PilotArgs a) {
    const int64_t seg = blockIdx.x;
    const cf* u = a.usum + seg * a.rows;
    double ar = 0.0, ai = 0.0;
    int cnt = 0;
    for (int64_t s = threadIdx.x; s + 1 < a.rows; s += 64) {
        if (s % a.rows_per_pattern == a.rows_per_pattern - 1) continue;                 // s + 1 opens the next pattern
        const cf u0 = u[s], u1 = u[s + 1];
        if ((u0.x == 0.f && u0.y == 0.f) || (u1.x == 0.f && u1.y == 0.f)) continue;      // a row without a usable pilot sum
        ar += double(u1.x) * double(u0.x) + double(u1.y) * double(u0.y);                 // U[s+1] conj(U[s])
        ai += double(u1.y) * double(u0.x) - double(u1.x) * double(u0.y);
        ++cnt;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ar += __shfl_xor(ar, m, 64);
        ai += __shfl_xor(ai, m, 64);
        cnt += __shfl_xor(cnt, m, 64);
    }
    if (threadIdx.x == 0) a.cfo[seg] = cnt ? atan2(ai, ar) * a.cfo_scale : double(NAN);
}

template <int MOD>
void launch_pilot_mod(const PilotArgs& a, unsigned grid, hipStream_t s) {
    if (a.slope)
        hipLaunchKernelGGL((pilot_track_kernel<MOD, true>), dim3(grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((pilot_track_kernel<MOD, false>), dim3(grid), dim3(256), 0, s, a);
}

}  // namespace

// The caller has checked the arguments (index ranges included) and sized a.usum.
hipError_t launch_pilot_track(const PilotArgs& a, hipStream_t s) {
    const int64_t total = a.n_seg * a.rows;
    if (total > 0 && (a.data || a.cpe || a.slope_out || a.usum)) {
        const int64_t groups = (total + a.rows_per_group - 1) / a.rows_per_group;
        const int64_t per_wg = 256 >> a.g_log2;
        const unsigned grid = unsigned((groups + per_wg - 1) / per_wg);
        switch (a.bits ? a.mod : 0) {
            case 0: launch_pilot_mod<0>(a, grid, s); break;
            case 2: launch_pilot_mod<2>(a, grid, s); break;
            case 4: launch_pilot_mod<4>(a, grid, s); break;
            case 6: launch_pilot_mod<6>(a, grid, s); break;
            default: return hipErrorInvalidValue;
        }
    }
    if (a.cfo && a.n_seg > 0) hipLaunchKernelGGL(pilot_cfo_kernel, dim3(unsigned(a.n_seg)), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ofdm
