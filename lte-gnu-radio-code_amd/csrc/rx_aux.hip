// rx_aux.hip -- small stand-alone kernels of the receive path (gfx950): bit-error count, row renormalisation, output packing,
// DSSS despreading.
#include "ofdm_launch.hpp"

namespace ofdm {

// ------------------------------------------------------------------------------------------ bit-error count
// count += popcount(a ^ b) over n bytes: the BER numerator of two packed bit-streams without moving them anywhere (SURVEY 8e:
// "gather counts instead"; the reference's idiom is bitwise_xor(a, b).sum(), TEST/GNU_RADIO_OFFLINE/pls_aio.py:131).
__global__ void __launch_bounds__(256) bit_errors_kernel(const uint8_t* a, const uint8_t* b, int64_t n, unsigned long long* count) {
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = int64_t(gridDim.x) * blockDim.x;
    const bool wide = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    const int64_t n16 = wide ? n / 16 : 0;
    unsigned c = 0;                                                   // <= 128 per step: a lane would need 2^25 steps to overflow
    const uint4* a4 = reinterpret_cast<const uint4*>(a);
    const uint4* b4 = reinterpret_cast<const uint4*>(b);
    for (int64_t i = gid; i < n16; i += stride) {
        const uint4 x = a4[i], y = b4[i];
        c += __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
    }
    for (int64_t i = n16 * 16 + gid; i < n; i += stride) c += __popc(unsigned(a[i] ^ b[i]));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, static_cast<unsigned long long>(c));
}

hipError_t launch_bit_errors(const uint8_t* a, const uint8_t* b, int64_t n, unsigned long long* count, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n / 16 + 255) / 256 + 1, 65536);
    hipLaunchKernelGGL(bit_errors_kernel, dim3(unsigned(blocks)), dim3(256), 0, s, a, b, n, count);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ row renormalisation
// SynchronizeAndEstimate.py:431-434: after row r = f*D + n has been equalised it is divided by sqrt(mean |row f|^2) -- row f,
// not row r -- in loop order, so row f already carries its own final scaling (f <= r; f == r only for row 0).
__global__ void __launch_bounds__(256) row_renorm_kernel(cf* eq, int Kd, int D, int n_frames, const int* tsr) {
    __shared__ float sh[256];
    for (int f = 0; f < n_frames; ++f) {
        if (tsr[f * 4 + 3] == 0) continue;                       // guard failed: row untouched
        for (int n = 0; n < D; ++n) {
            const int r = f * D + n;
            float acc = 0.f;
            for (int i = threadIdx.x; i < Kd; i += blockDim.x) acc += cnorm2(eq[int64_t(f) * Kd + i]);
            sh[threadIdx.x] = acc;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
                __syncthreads();
            }
            const float inv = 1.f / sqrtf(sh[0] / float(Kd));
            __syncthreads();
            for (int i = threadIdx.x; i < Kd; i += blockDim.x) eq[int64_t(r) * Kd + i] = cscale(eq[int64_t(r) * Kd + i], inv);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------ output packing of the stream block
// SynchAndChanEst.py:249-255: rows 3, 3 + (S+D), ... of est_data_freq are deleted (literal 3), the rest flattened row-major.
// Done on the device so that the block's output leaves in ONE contiguous device-to-host copy straight into the caller's buffer.
__global__ void __launch_bounds__(256) pack_rows_kernel(const cf* edf, int rows, int Kd, int SD, cf* out) {
    const int r = blockIdx.y;
    if (r >= 3 && (r - 3) % SD == 0) return;                                            // a deleted row
    const int w = r - (r >= 3 ? (r - 3) / SD + 1 : 0);                                  // rows kept before it
    const float4* src = reinterpret_cast<const float4*>(edf + int64_t(r) * Kd);         // Kd is even: whole 16 B pairs
    float4* dst = reinterpret_cast<float4*>(out + int64_t(w) * Kd);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (Kd >> 1); i += gridDim.x * blockDim.x) dst[i] = src[i];
}
hipError_t launch_pack_rows(const cf* edf, int rows, int Kd, int SD, cf* out, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_rows_kernel, dim3(unsigned(((Kd >> 1) + 255) / 256), unsigned(rows)), dim3(256), 0, s, edf, rows, Kd, SD, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ DSSS despreading
__global__ void despread_kernel(const cf* in, int in_row_stride, const cf* code, int dsss, int n_spread, int rows, cf* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (i >= n_spread || row >= rows) return;
    const cf* x = in + int64_t(row) * in_row_stride + int64_t(i) * dsss;
    cf acc = cf{0.f, 0.f};
    for (int sf = 0; sf < dsss; ++sf) acc = acc + cmulc(x[sf], code[sf]);              // x * conj(SC[sf])  (:395)
    out[int64_t(row) * n_spread + i] = cscale(acc, 1.f / float(dsss));                  // np.average        (:396)
}

hipError_t launch_row_renorm(cf* eq, int Kd, int D, int n_frames, const int* tsr, hipStream_t s) {
    if (n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(row_renorm_kernel, dim3(1), dim3(256), 0, s, eq, Kd, D, n_frames, tsr);
    return hipGetLastError();
}

hipError_t launch_despread(const cf* in, int in_row_stride, const cf* code, int dsss, int n_spread, int rows, cf* out, hipStream_t s) {
    if (rows <= 0 || n_spread <= 0) return hipSuccess;
    hipLaunchKernelGGL(despread_kernel, dim3(unsigned((n_spread + 63) / 64), unsigned(rows)), dim3(64), 0, s, in, in_row_stride, code,
                       dsss, n_spread, rows, out);
    return hipGetLastError();
}

}  // namespace ofdm
