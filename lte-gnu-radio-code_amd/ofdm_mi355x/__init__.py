"""MI355X-native OFDM PHY hot path: Python host side of libofdm_mi355x.so."""
from ._lib import (BITS_NONE, BITS_PACKED, BITS_UNPACKED, COMPAT_RXOFDM, COMPAT_UTSA, CRC8, CRC16, CRC24A, CRC24B,  # noqa: F401
                   CSI_NOISE_EST, CSI_NOISE_GIVEN, CSI_ROWS_ALL, CSI_ROWS_DATA, DESPREAD_NOISE_GIVEN, DESPREAD_NOISE_RHO,
                   DESPREAD_NOISE_SEG, LIB_PATH, MRC_NOISE_EST, MRC_NOISE_GIVEN,
                   MRC_NOISE_SEG, OfdmError, OfdmLibraryError, PILOT_CPE,
                   PILOT_CPE_SLOPE, TRACK_HOLD, TRACK_LINEAR, load)
from .engine import (DeviceBuffer, FoEngine, RxEngine, TrkEngine, TxEngine, alloc_layout, bins_p, count_bit_errors, crc_bits,  # noqa: F401
                     crc_compute, crc_compute_long, dft_plan_info, dft_size_ok, gold_bits, tb_geometry, tbcc_blocks, tbcc_rm_blocks, turbo_blocks,
                     turbo_k_next, turbo_qpp_check, turbo_rm_blocks, turbo_rm_info, zadoff_chu)
from .safe_pickle import UnsafePickleError, load_ndarray  # noqa: F401
