// yawhip_kernel_band32.hip -- k_count_band32: the float32 band kernel (BAND on strip layouts of unit vectors, the headline) with
// up to three windows (or pieces of one) staged in a round, and launch_band32. Kernel and launcher are csrc/yawhip_band32.inc; yawhip.hip has the map of the units.
#include "yawhip_count_device.h"

#define YAW_B32_NAME k_count_band32
#define YAW_B32_LAUNCH launch_band32
#define YAW_B32_CH 3
#include "yawhip_band32.inc"
