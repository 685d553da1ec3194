// rx_demod_1024_kd.hip -- instantiates the batch launch of rx_demod_kernel<1024, ..., KD = 600> (bin-list length compiled in)
#include "rx_demod.hpp"
namespace ofdm {
template hipError_t launch_rx_demod_batch<1024, DemodGeom<1024>::KD_LTE>(const RxDev&, DemodArgs, unsigned, size_t, int, hipStream_t);
}  // namespace ofdm
