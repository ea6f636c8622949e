// sk_u16_dense_dvb.hip — the search kernel family for uint16_t components with the LK_DENSE query lookup table,
// DotVByte forward index: fixed-u8 codes + eight 12-bit component gaps per slice (record.hpp: VT_DVB).
#include "search_kernel.inc"

namespace sgpu {
hipError_t run_u16_dense_dvb(const LaunchArgs& a, int* occupancy) { return run_family<uint16_t, LK_DENSE, VT_DVB>(a, occupancy); }
}  // namespace sgpu
