// Internal interface between yawhip_api.hip and yawhip_healpix.hip (HEALPix pixels and maps of a catalogue,
// yawhip_healpix_map; the unmasked pixels of a scalar map as a catalogue's columns, yawhip_healpix_pixels). Not part of
// the C ABI: yawhip_api.hip checks the arguments and owns the error reporting. The Workspace is a member of every context
// (yawhip_internal.h).
#ifndef YAWHIP_HEALPIX_H
#define YAWHIP_HEALPIX_H
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "yawhip_devmem.h"

namespace yawpix {

using yawhip_detail::DevBuf;
using yawhip_detail::DevPtr;

constexpr int MAX_ORDER = 13;                         // a float64 map of order 14 is 25 GB
constexpr int64_t DEFAULT_CHUNK = (int64_t)1 << 24;   // objects per pass when the caller gives 0
constexpr int64_t MAX_CHUNK = (int64_t)1 << 28;       // larger chunk sizes are cut to this

// Device buffers of the call (grow-only, owned by the caller's context).
struct Workspace {
    DevPtr<double> cols;         // [3][chunk_cap]: phi, z, w of one pass
    DevPtr<int64_t> pix;         // [chunk_cap] pixels of one pass
    DevPtr<uint32_t> keys;       // [2][chunk_cap] sort keys, in and out (weighted maps)
    DevPtr<double> w_sorted;     // [chunk_cap]
    size_t chunk_cap = 0;
    bool sort_bufs = false;      // keys and w_sorted are allocated for chunk_cap
    DevBuf<unsigned char> tmp;   // rocPRIM's temporary storage
    DevBuf<double> map;          // the map: uint64 counters while objects are counted, float64 at the end
    // yawhip_healpix_pixels
    DevBuf<double> src;          // the uploaded scalar map, then (with a weight map) the weight map behind it
    DevPtr<double> sel;          // [4][sel_cap]: phi, z, kappa, w of the selected pixels of one pass
    DevPtr<int64_t> sel_pix;     // [sel_cap] their pixel numbers
    DevPtr<int64_t> wg_counts;   // [2][sel_cap / 256 + 2]: selected pixels per workgroup of a pass, and their exclusive scan
    size_t sel_cap = 0;
    size_t bytes() const;
    void release() { *this = Workspace{}; }
};

// One call (see yawhip_healpix_map in include/yawhip.h for the meaning of every field).
struct MapCall {
    int64_t n = 0, chunksize = 0;                           // chunksize in 1 .. MAX_CHUNK
    const double *phi = nullptr, *z = nullptr, *w = nullptr;  // host, n values each, w may be null
    int32_t order = 0, nested = 1;
    int64_t *pix_out = nullptr;  // host, n values, may be null
    double *map_out = nullptr;   // host, 12 * 4^order values, may be null
};

// Runs the call on the current device's `stream` and waits for it. Arguments are already checked.
hipError_t healpix_map(Workspace &ws, hipStream_t stream, const MapCall &c);

// One call of yawhip_healpix_pixels (see include/yawhip.h for the meaning of every field).
struct PixelsCall {
    int64_t chunksize = 0;                                  // nested pixels per pass, 1 .. MAX_CHUNK
    const double *values = nullptr, *weights = nullptr;     // host, 12 * 4^order values each, weights may be null
    int32_t order = 0, nested = 0;
    int64_t capacity = 0;                                   // entries of every host output
    int64_t *ipix_out = nullptr;                            // host outputs; w_out is null without weights
    double *phi_out = nullptr, *z_out = nullptr, *kappa_out = nullptr, *w_out = nullptr;
};

// Runs the call on the current device's `stream` and waits for it. Arguments are already checked. `selected` is the
// number of pixels copied to the outputs; `overflow` is set, and the call stops before it copies, when a pass would go
// beyond `capacity`.
hipError_t healpix_pixels(Workspace &ws, hipStream_t stream, const PixelsCall &c, int64_t &selected, bool &overflow);

}  // namespace yawpix
#endif
