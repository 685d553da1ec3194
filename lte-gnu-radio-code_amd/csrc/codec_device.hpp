// codec_device.hpp -- device helpers the channel-coding kernels share (gfx950): tbcc.hip, turbo.hip, turbo_es.hip (through
// turbo_siso.hpp) and turbo_rm.hip.  Every helper is inlined into its caller.  There is NO file-scope fp-contract pragma here:
// tbcc.hip is compiled with contraction allowed and the turbo units with it off, so nothing in this file may contain a product
// followed by an add.
//
// What is NOT here although several kernels repeat it: the aligned-word-else-bytes store, the packed / unpacked coded-word loop,
// the de-matching decomposition and combine loop, and the turbo decoders' output pass.  As shared inline functions each of them
// changed the instructions of the kernels that used it (same descriptor, another order), and a codec kernel whose text changes
// has to be held byte-equal and timed against its parent first; those kernels carry the code written out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ofdm {

namespace {

// An input LLR that is not finite counts as 0 (the contract's non-finite rule), by the exponent mask.  NOT soft_finite of
// soft_device.hpp: that one is fabsf(x) < inf, another expression that compiles to other instructions, and the kernels of both
// sides are held to their instructions.
__device__ __forceinline__ float finite_or_zero(float v) {
    return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u ? 0.f : v;
}

// bit i of a block of information bits: one per byte, or packed MSB-first.  Index = int (TBCC) or unsigned (turbo).
template <class Index>
__device__ __forceinline__ unsigned info_bit(const uint8_t* blk, int packed, Index i) {
    return packed ? (unsigned(blk[i >> 3]) >> (7 - (i & 7))) & 1u : unsigned(blk[i]) & 1u;
}

__device__ __forceinline__ float readlane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float bperm(int byte_addr, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(v)));
}

}  // namespace

}  // namespace ofdm
