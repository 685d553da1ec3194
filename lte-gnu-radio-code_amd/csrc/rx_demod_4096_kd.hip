// rx_demod_4096_kd.hip -- instantiates the batch launch of rx_demod_kernel<4096, ..., KD = 2400> (bin-list length compiled in)
#include "rx_demod.hpp"
namespace ofdm {
template hipError_t launch_rx_demod_batch<4096, DemodGeom<4096>::KD_LTE>(const RxDev&, DemodArgs, unsigned, size_t, int, hipStream_t);
}  // namespace ofdm
