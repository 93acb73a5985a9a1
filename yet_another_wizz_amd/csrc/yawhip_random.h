// Internal interface between yawhip_api.hip and yawhip_random.hip (random catalogues drawn from numpy's PCG64 stream,
// yawhip_random_box and yawhip_random_healpix). Not part of the C ABI: yawhip_api.hip checks the arguments and owns the
// error reporting.
#ifndef YAWHIP_RANDOM_H
#define YAWHIP_RANDOM_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace yawrand {

// What every generator's draw of n values in chunks of `chunksize` has: numpy's PCG64 state before the first chunk, the
// attached data and the host outputs (see yawhip_random_box in include/yawhip.h for the meaning of every field).
struct Draw {
    int64_t n = 0, chunksize = 0;
    uint64_t state_hi = 0, state_lo = 0, inc_hi = 0, inc_lo = 0;
    int32_t has_uint32 = 0;
    uint32_t uinteger = 0;
    int64_t n_data = -1;  // -1: nothing attached, else 1 .. 2^32
    const double *data_w = nullptr, *data_z = nullptr;  // host, n_data values each, may be null
    double *x_out = nullptr, *y_out = nullptr, *w_out = nullptr, *z_out = nullptr;  // host, n values each
    int64_t *idx_out = nullptr;  // host, n values, may be null
};

// One BoxRandoms draw: the box.
struct BoxDraw : Draw {
    double x_min = 0.0, x_range = 0.0, y_min = 0.0, y_range = 0.0;
};

// One HealPixRandoms draw: the unmasked pixels of a nested map of `order` and their cumulative probabilities (see
// yawhip_random_healpix in include/yawhip.h).
struct HealpixDraw : Draw {
    int32_t order = 0;
    int64_t n_unmasked = 0;
    const int64_t *ipix_unmasked = nullptr;  // host, n_unmasked values
    const double *cdf = nullptr;             // host, n_unmasked values
    int64_t *pix_out = nullptr;              // host, n values, may be null
};

// numpy's PCG64 state after the last chunk.
struct DrawEnd {
    uint64_t state_hi = 0, state_lo = 0;
    int32_t has_uint32 = 0;
    uint32_t uinteger = 0;
};

// Run the draw on the current device's `stream` and wait for it. Arguments are already checked.
hipError_t draw_box(hipStream_t stream, const BoxDraw &d, DrawEnd &end);
hipError_t draw_healpix(hipStream_t stream, const HealpixDraw &d, DrawEnd &end);

}  // namespace yawrand
#endif
