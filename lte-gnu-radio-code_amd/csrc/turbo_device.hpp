// turbo_device.hpp -- the device routines the turbo encoders share (turbo.hip, turbo_rm.hip): the QPP interleaver in 32-bit
// arithmetic and the constituent encoder's step, free response and termination (the information-bit fetch: codec_device.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "codec_device.hpp"
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

// pi(i) = (f1 i + f2 i^2) mod K in 32-bit arithmetic: every product stays below 2^26 for K <= 6144
__device__ __forceinline__ unsigned turbo_qpp_at(const TurboQpp& q, unsigned i) {
    const unsigned K = unsigned(q.K);
    return ((unsigned(q.f1) * i) % K + ((i * i) % K) * unsigned(q.f2) % K) % K;
}
__device__ __forceinline__ unsigned turbo_mod_add(unsigned a, unsigned b, unsigned K) {
    const unsigned s = a + b;                                // a, b < K
    return s >= K ? s - K : s;
}

// one step of a constituent encoder: state s = 4 r1 + 2 r2 + r3, input u -> parity z, next state
__device__ __forceinline__ unsigned turbo_rsc_step(unsigned s, unsigned u, unsigned& z) {
    const unsigned r1 = s >> 2, r2 = (s >> 1) & 1u, r3 = s & 1u;
    const unsigned a = u ^ r2 ^ r3;
    z = a ^ r1 ^ r3;
    return (a << 2) | (s >> 1);
}
// n steps with input 0 (the register's free response; its period is 7)
__device__ __forceinline__ unsigned turbo_rsc_free(unsigned s, int n) {
    for (; n > 0; --n) s = ((((s >> 1) ^ s) & 1u) << 2) | (s >> 1);
    return s;
}
// the three termination steps from state s: x_K z_K x_{K+1} z_{K+1} x_{K+2} z_{K+2}, the first on top (bit 5)
__device__ __forceinline__ unsigned turbo_rsc_tail(unsigned s) {
    unsigned bits = 0u;
    for (int j = 0; j < 3; ++j) {
        const unsigned r1 = s >> 2, r2 = (s >> 1) & 1u, r3 = s & 1u;
        bits = (bits << 2) | ((r2 ^ r3) << 1) | (r1 ^ r3);
        s >>= 1;
    }
    return bits;
}

}  // namespace

}  // namespace ofdm
