// yawhip_kernel_band32_one.hip -- k_count_band32_one: the float32 band kernel (BAND on strip layouts of unit vectors, the headline) with
// one window staged in a round, and launch_band32_one. Kernel and launcher are csrc/yawhip_band32.inc; yawhip.hip has the map of the units.
#include "yawhip_count_device.h"

#define YAW_B32_NAME k_count_band32_one
#define YAW_B32_LAUNCH launch_band32_one
#define YAW_B32_CH 1
#include "yawhip_band32.inc"
