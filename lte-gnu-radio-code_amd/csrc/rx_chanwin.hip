// rx_chanwin.hip -- delay-window denoising of the LS channel estimate (gfx950): chan_window_kernel and its launch.
// Contract: include/ofdm_mi355x.h, "delay-window channel-estimate denoising"; tests/chanwin_ref.py restates it in fp64 NumPy.
//
// A unit of its own on purpose: the kernels of rx_sync.hip keep their module and with it their code (rx_sync_scan.hpp says why
// those live in one unit).
#include <type_traits>

#include "ofdm_launch.hpp"

namespace ofdm {

// One row (frame) per FFT slot, Plan<N>::SLOTS rows per workgroup, laid out as rx_chan_time_kernel:
//   H row -> conj / FFT / conj * 1/N = h (register slot order) -> LDS in natural tap order -> each lane takes back the taps
//   n = t + T*n0 it feeds the forward FFT with, zeroes the ones outside the window and adds their power -> FFT -> sync-bin mask
//   -> H', gains, tail.
// The tail sum has a fixed order: a lane's P taps in ascending n0, the T lanes through symbol_sum (lane shuffles, then one LDS
// partial per wave for T > 64, added in wave order): the same bits on every call, in any batch.
// A row without a sync (tsr[3] != 1) runs the arithmetic on zeros and stores nothing but tail = +0.
template <int N>
__global__ void __launch_bounds__(Plan<N>::WG) chan_window_kernel(RxDev rx, ChanWinArgs a) {
    using PL = Plan<N>;
    constexpr int T = PL::T, P = PL::P;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int slot = (T >= 64) ? __builtin_amdgcn_readfirstlane(tid / T) : tid / T;
    const int t = tid % T;
    cf* smem = reinterpret_cast<cf*>(smem_raw);
    cf* lds = smem + slot * WgLds<N>::STRIDE;
    float* red = reinterpret_cast<float*>(lds + WgLds<N>::ELEMS);
    const cf* w1tab = wg_init_w1<N>(smem, rx.tw, tid);
    std::conditional_t<PL::R0 == 16, CompactTwiddles<N>, LaneTwiddles<N>> tw;
    load_twiddles(tw, rx.tw, t);

    const int64_t row = int64_t(blockIdx.x) * PL::SLOTS + slot;
    const bool in_range = row < a.n_rows;
    const bool active = in_range && a.tsr[row * 4 + 3] == 1;
    const int lag = active ? a.tsr[row * 4 + 1] : 0;

    cf v[P];
#pragma unroll
    for (int n0 = 0; n0 < P; ++n0) v[n0] = active ? cconj(a.H_in[row * N + t + T * n0]) : cf{0.f, 0.f};
    wg_fft<N>(v, lds, tw, w1tab, t);                       // conj(ifft(H)) * N
    wg_barrier();                                          // the exchange region is read until every lane is through the last pass
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) lds[(t + T * j) + PL::NC * kl] = cscale(cconj(v[out_slot<N>(j, kl)]), 1.f / float(N));
    }
    wg_barrier();
    float acc = 0.f;
#pragma unroll
    for (int n0 = 0; n0 < P; ++n0) {
        const int n = t + T * n0;
        const cf h = lds[n];
        const bool keep = n < a.post || n >= N - a.pre;
        acc += keep ? 0.f : cnorm2(h);
        v[n0] = keep ? h : cf{0.f, 0.f};
    }
    wg_barrier();                                          // every tap is read before the FFT below overwrites the region
    const float sum = symbol_sum<T>(acc, red, t);
    const int M = N - a.pre - a.post;
    const float tail = M > 0 ? (float(N) / float(M)) * sum : 0.f;
    wg_fft<N>(v, lds, tw, w1tab, t);

    if (in_range && t == 0 && a.tail) a.tail[row] = active ? tail : 0.f;
    if (!active) return;
    // this lane's bins k = (t + T*j) + NC*kl: consecutive lanes hold consecutive bins.  The lag de-rotation e^{+j 2pi d k/N} and
    // the gain are the expressions of sync_finalize (rx_sync.hpp).
    const int Ks = rx.Ks, Kd = rx.Kd;
#pragma unroll
    for (int j = 0; j < PL::C; ++j) {
#pragma unroll
        for (int kl = 0; kl < PL::RL; ++kl) {
            const int k = (t + T * j) + PL::NC * kl;
            int in_, ip_;
            const bool neg = bin_neg(k, Ks, N, in_), pos = bin_pos(k, Ks, ip_);
            const cf Hk = (neg || pos) ? v[out_slot<N>(j, kl)] : cf{0.f, 0.f};
            a.H_out[row * N + k] = Hk;
            if (a.gain) {
                const cf rot = cconj(rx.tw[(unsigned(lag) * unsigned(k)) & unsigned(N - 1)]);   // any lag, also a negative one
                const cf gk = cmul(cscale(cconj(Hk), 1.f / (cnorm2(Hk) + rx.inv_snr_data)), rot);
                int id_;
                if (bin_neg(k, Kd, N, id_)) a.gain[row * Kd + id_] = gk;
                if (bin_pos(k, Kd, id_)) a.gain[row * Kd + id_] = gk;
            }
        }
    }
}

template <int N>
static hipError_t launch_chan_window_n(const RxDev& rx, const ChanWinArgs& a, hipStream_t s) {
    const unsigned grid = unsigned((a.n_rows + Plan<N>::SLOTS - 1) / Plan<N>::SLOTS);
    hipLaunchKernelGGL(chan_window_kernel<N>, dim3(grid), dim3(Plan<N>::WG), WgLds<N>::BYTES, s, rx, a);
    return hipGetLastError();
}

// the dispatch of rx_sync.hpp's OFDM_DISPATCH_N, written out: this unit does not include the sync kernels' header
hipError_t launch_chan_window(const RxDev& rx, const ChanWinArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    switch (rx.nfft) {
        case 64: return launch_chan_window_n<64>(rx, a, s);
        case 128: return launch_chan_window_n<128>(rx, a, s);
        case 256: return launch_chan_window_n<256>(rx, a, s);
        case 512: return launch_chan_window_n<512>(rx, a, s);
        case 1024: return launch_chan_window_n<1024>(rx, a, s);
        case 2048: return launch_chan_window_n<2048>(rx, a, s);
        case 4096: return launch_chan_window_n<4096>(rx, a, s);
        default: return hipErrorInvalidValue;
    }
}

// sigma2[f] = double(tail[f]): the layout OFDM_MRC_NOISE_SEG takes
__global__ void __launch_bounds__(256) chan_noise_kernel(const float* tail, int64_t n, double* sigma2) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) sigma2[i] = double(tail[i]);
}

hipError_t launch_chan_noise(const float* tail, int64_t n, double* sigma2, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(chan_noise_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, s, tail, n, sigma2);
    return hipGetLastError();
}

hipError_t chan_window_prepare() {
    return load_kernels(chan_noise_kernel,chan_window_kernel<64>, chan_window_kernel<128>, chan_window_kernel<256>, chan_window_kernel<512>,
                        chan_window_kernel<1024>, chan_window_kernel<2048>, chan_window_kernel<4096>);
}

}  // namespace ofdm
