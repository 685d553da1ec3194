// rx_demod_2048_kd.hip -- instantiates the batch launch of rx_demod_kernel<2048, ..., KD = 1200> (bin-list length compiled in)
#include "rx_demod.hpp"
namespace ofdm {
template hipError_t launch_rx_demod_batch<2048, DemodGeom<2048>::KD_LTE>(const RxDev&, DemodArgs, unsigned, size_t, int, hipStream_t);
}  // namespace ofdm
