// Internal interface between yawhip_api.hip and yawhip_hist.hip (per-patch redshift histograms, yawhip_redshift_histogram).
// Not part of the C ABI: yawhip_api.hip checks the arguments and owns the error reporting.
#ifndef YAWHIP_HIST_H
#define YAWHIP_HIST_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace yawhist {

// One histogram call (see yawhip_redshift_histogram in include/yawhip.h for the meaning of every field).
struct HistCall {
    int64_t n = 0;
    const double *z = nullptr, *w = nullptr;  // host, n values each, w may be null
    int32_t n_patches = 0;
    const int64_t *offsets = nullptr;  // host, n_patches + 1
    int32_t n_edges = 0;
    const double *edges = nullptr;  // host, n_edges
    int32_t closed_right = 1;
    int chunk_log2 = 23;  // objects per upload = 2^chunk_log2
    double *out = nullptr;  // host, n_patches x (n_edges - 1)
};

// Runs the histogram on the current device's `stream` and waits for it. Arguments are already checked.
hipError_t redshift_histogram(hipStream_t stream, const HistCall &c);

}  // namespace yawhist
#endif
