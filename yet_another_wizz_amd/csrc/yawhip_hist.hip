// yawhip_hist.hip -- per-patch redshift histograms (HistData.from_catalog, reference src/yaw/redshifts.py:44-57, 101-151).
//
// The reference calls np.histogram(z[mask], edges, weights=w[mask]) once per patch, mask = z > e[0] (closed "right") or
// z < e[B] (closed "left"). numpy's rule on the kept values: bin i if e[i] <= z < e[i+1], the last bin also takes
// z == e[B]; values outside [e[0], e[B]] and NaN are dropped. Every bin is decided here by float64 comparisons against
// the given edges (a binary search), never by an index computed from a bin width.
//
// The columns are uploaded in chunks of 2^chunk_log2 objects (peak device memory does not grow with n). The host cuts
// every chunk into tiles of at most TILE objects that never cross a patch boundary, and the tiles into batches whose
// partial histograms fit PARTIAL_BUDGET. Per batch:
//   * k_hist_tiles: one workgroup per tile. With at most HIST_LDS_BINS bins the tile's histogram lives in LDS (uint32
//     counters without weights, so counts are exact; float64 sums with weights) and is written to the tile's row of the
//     partial buffer; with more bins the workgroup adds straight into its own row (zeroed before: uint64 counters
//     without weights, float64 sums with them), so no row is ever shared between workgroups. Edges are read from LDS
//     when they fit EDGES_LDS_MAX, else from global memory.
//   * k_hist_combine: sums the rows of each run of consecutive tiles of one patch, in tile order.
// The host adds the runs into out[patch] in chunk order. Without weights every partial is an integer count (exact as a
// float64 below 2^53), so the counts are exact whatever the order; with weights the only order that varies is that of
// the float64 LDS / in-row atomic adds inside one tile (at most TILE terms).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "yawhip_devmem.h"
#include "yawhip_hist.h"

namespace yawhist {

namespace {

constexpr int WG = 256;
constexpr int ROUNDS = 16;                       // objects per thread and tile
constexpr int64_t TILE = (int64_t)WG * ROUNDS;   // objects per tile (workgroup)
constexpr int HIST_LDS_BINS = 2048;              // most bins of the LDS histogram (16 KiB of float64 + 16 KiB of edges)
constexpr int EDGES_LDS_MAX = 8192;              // most edges copied to LDS (64 KiB)
constexpr int64_t PARTIAL_BUDGET = (int64_t)64 << 20;  // bytes of per-tile partial histograms per batch
constexpr int64_t BATCH_TILES_MAX = 32768;       // tiles per batch (k_hist_combine takes one grid row per run)

__device__ __forceinline__ int find_bin(const double *e, int n_bins, double z) {  // e[lo] <= z, lo in [0, n_bins - 1]
    int lo = 0, hi = n_bins;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= z) lo = mid;
        else hi = mid;
    }
    return lo;
}

// tiles[t] = {first object (chunk-relative), object count}; partial[t][n_edges - 1]
template <bool WEIGHTED, bool LDS_HIST, bool LDS_EDGES>
__global__ __launch_bounds__(WG) void k_hist_tiles(const double *__restrict__ z, const double *__restrict__ w,
                                                   const int2 *__restrict__ tiles, const double *__restrict__ edges_g,
                                                   int n_edges, int closed_right, double *__restrict__ partial) {
    extern __shared__ double lds[];
    const int n_bins = n_edges - 1;
    const int2 tile = tiles[blockIdx.x];
    double *row = partial + (size_t)blockIdx.x * (size_t)n_bins;
    const double *e = edges_g;
    if constexpr (LDS_EDGES) {
        for (int i = threadIdx.x; i < n_edges; i += WG) lds[i] = edges_g[i];
        e = lds;
    }
    double *hist_w = lds + n_edges;                              // LDS_HIST && WEIGHTED
    unsigned *hist_n = reinterpret_cast<unsigned *>(lds + n_edges);  // LDS_HIST && !WEIGHTED
    if constexpr (LDS_HIST) {
        for (int b = threadIdx.x; b < n_bins; b += WG) {
            if constexpr (WEIGHTED) hist_w[b] = 0.0;
            else hist_n[b] = 0u;
        }
    }
    if constexpr (LDS_EDGES || LDS_HIST) __syncthreads();
    const double e_lo = e[0], e_hi = e[n_bins];
    const double excluded = closed_right ? e_lo : e_hi;  // the reference's mask: z > e[0] or z < e[B]
    const double *zt = z + tile.x;
    const double *wt = WEIGHTED ? w + tile.x : nullptr;
    for (int i = threadIdx.x; i < tile.y; i += WG) {
        const double v = zt[i];
        if (!(v >= e_lo && v <= e_hi) || v == excluded) continue;  // outside the edges, NaN, or masked
        const int b = find_bin(e, n_bins, v);
        if constexpr (LDS_HIST) {
            if constexpr (WEIGHTED) atomicAdd(&hist_w[b], wt[i]);
            else atomicAdd(&hist_n[b], 1u);
        } else {
            // the workgroup's own row: no other workgroup writes it
            if constexpr (WEIGHTED) atomicAdd(&row[b], wt[i]);
            else atomicAdd(reinterpret_cast<unsigned long long *>(row) + b, 1ull);
        }
    }
    if constexpr (LDS_HIST) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += WG) row[b] = WEIGHTED ? hist_w[b] : (double)hist_n[b];
    }
}

// runs[r] = {first tile, end tile} of one patch inside the batch; run_out[r][n_bins] = the rows summed in tile order.
// count_rows: the rows hold uint64 counters (unweighted calls above HIST_LDS_BINS), else float64 values.
__global__ __launch_bounds__(WG) void k_hist_combine(const double *__restrict__ partial, const int2 *__restrict__ runs, int n_bins,
                                                     int count_rows, double *__restrict__ run_out) {
    const int b = blockIdx.x * WG + threadIdx.x;
    if (b >= n_bins) return;
    const int2 run = runs[blockIdx.y];
    double s = 0.0;
    const unsigned long long *counts = reinterpret_cast<const unsigned long long *>(partial);
    for (int t = run.x; t < run.y; ++t) {
        const size_t i = (size_t)t * n_bins + b;
        s += count_rows ? (double)counts[i] : partial[i];
    }
    run_out[(size_t)blockIdx.y * n_bins + b] = s;
}

template <bool WEIGHTED, bool LDS_HIST, bool LDS_EDGES>
hipError_t launch_tiles(hipStream_t stream, unsigned n_tiles, const double *z, const double *w, const int2 *tiles, const double *edges,
                        int n_edges, int closed_right, double *partial) {
    const size_t lds = (LDS_EDGES ? (size_t)n_edges * sizeof(double) : 0) +
                       (LDS_HIST ? (size_t)(n_edges - 1) * (WEIGHTED ? sizeof(double) : sizeof(unsigned)) : 0);
    hipLaunchKernelGGL((k_hist_tiles<WEIGHTED, LDS_HIST, LDS_EDGES>), dim3(n_tiles), dim3(WG), lds, stream, z, w, tiles, edges, n_edges,
                       closed_right, partial);
    return hipGetLastError();
}

template <bool WEIGHTED>
hipError_t launch_tiles(hipStream_t stream, unsigned n_tiles, const double *z, const double *w, const int2 *tiles, const double *edges,
                        int n_edges, int closed_right, double *partial) {
    if (n_edges - 1 <= HIST_LDS_BINS)
        return launch_tiles<WEIGHTED, true, true>(stream, n_tiles, z, w, tiles, edges, n_edges, closed_right, partial);
    if (n_edges <= EDGES_LDS_MAX)
        return launch_tiles<WEIGHTED, false, true>(stream, n_tiles, z, w, tiles, edges, n_edges, closed_right, partial);
    return launch_tiles<WEIGHTED, false, false>(stream, n_tiles, z, w, tiles, edges, n_edges, closed_right, partial);
}

}  // namespace

hipError_t redshift_histogram(hipStream_t stream, const HistCall &c) {
    const int n_bins = c.n_edges - 1;
    const int P = c.n_patches;
    std::fill(c.out, c.out + (size_t)P * (size_t)n_bins, 0.0);
    if (c.n == 0) return hipSuccess;
    const bool weighted = c.w != nullptr;
    const int64_t chunk = std::min<int64_t>((int64_t)1 << c.chunk_log2, c.n);
    const int64_t batch_max = std::max<int64_t>(1, std::min<int64_t>(BATCH_TILES_MAX, PARTIAL_BUDGET / ((int64_t)n_bins * 8)));

    using yawhip_detail::DevPtr;  // (no count below is zero: n, n_edges, n_bins and batch_max are all >= 1 here)
    DevPtr<double> d_z, d_w, d_edges, d_partial, d_run_out;
    DevPtr<int2> d_tiles, d_runs;
    hipError_t e = d_z.alloc((size_t)chunk);
    if (e == hipSuccess && weighted) e = d_w.alloc((size_t)chunk);
    if (e == hipSuccess) e = d_edges.alloc((size_t)c.n_edges);
    if (e == hipSuccess) e = d_partial.alloc((size_t)batch_max * n_bins);
    if (e == hipSuccess) e = d_run_out.alloc((size_t)batch_max * n_bins);
    if (e == hipSuccess) e = d_tiles.alloc((size_t)batch_max);
    if (e == hipSuccess) e = d_runs.alloc((size_t)batch_max);
    if (e == hipSuccess) e = hipMemcpyAsync(d_edges, c.edges, (size_t)c.n_edges * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;

    std::vector<int2> tiles, runs;
    std::vector<int32_t> tile_patch, run_patch;
    std::vector<double> run_out;
    int32_t p_first = 0;  // first patch that ends after the current chunk's start
    for (int64_t c0 = 0; c0 < c.n && e == hipSuccess; c0 += chunk) {
        const int64_t c1 = std::min(c.n, c0 + chunk);
        e = hipMemcpyAsync(d_z, c.z + c0, (size_t)(c1 - c0) * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && weighted)
            e = hipMemcpyAsync(d_w, c.w + c0, (size_t)(c1 - c0) * sizeof(double), hipMemcpyHostToDevice, stream);
        // tiles of this chunk: the pieces of every patch it overlaps, cut into TILE objects
        tiles.clear();
        tile_patch.clear();
        while (p_first < P && c.offsets[p_first + 1] <= c0) ++p_first;
        for (int32_t p = p_first; p < P && c.offsets[p] < c1; ++p) {
            const int64_t lo = std::max(c.offsets[p], c0), hi = std::min(c.offsets[p + 1], c1);
            for (int64_t s = lo; s < hi; s += TILE) {
                tiles.push_back(make_int2((int)(s - c0), (int)std::min(TILE, hi - s)));
                tile_patch.push_back(p);
            }
        }
        for (size_t t0 = 0; t0 < tiles.size() && e == hipSuccess; t0 += (size_t)batch_max) {
            const size_t t1 = std::min(tiles.size(), t0 + (size_t)batch_max);
            runs.clear();
            run_patch.clear();
            for (size_t t = t0; t < t1; ++t) {
                if (t == t0 || tile_patch[t] != tile_patch[t - 1]) {
                    runs.push_back(make_int2((int)(t - t0), (int)(t - t0)));
                    run_patch.push_back(tile_patch[t]);
                }
                runs.back().y = (int)(t - t0 + 1);
            }
            const unsigned n_tiles = (unsigned)(t1 - t0), n_runs = (unsigned)runs.size();
            e = hipMemcpyAsync(d_tiles, tiles.data() + t0, n_tiles * sizeof(int2), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(d_runs, runs.data(), n_runs * sizeof(int2), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess && n_bins > HIST_LDS_BINS)  // rows the workgroups add into
                e = hipMemsetAsync(d_partial, 0, (size_t)n_tiles * n_bins * sizeof(double), stream);
            if (e == hipSuccess)
                e = weighted ? launch_tiles<true>(stream, n_tiles, d_z, d_w, d_tiles, d_edges, c.n_edges, c.closed_right, d_partial)
                             : launch_tiles<false>(stream, n_tiles, d_z, nullptr, d_tiles, d_edges, c.n_edges, c.closed_right, d_partial);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_hist_combine, dim3((unsigned)((n_bins + WG - 1) / WG), n_runs), dim3(WG), 0, stream, d_partial, d_runs,
                                   n_bins, (int)(!weighted && n_bins > HIST_LDS_BINS), d_run_out);
                e = hipGetLastError();
            }
            run_out.resize((size_t)n_runs * n_bins);
            if (e == hipSuccess)
                e = hipMemcpyAsync(run_out.data(), d_run_out, run_out.size() * sizeof(double), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) break;
            for (unsigned r = 0; r < n_runs; ++r) {  // runs in order: a patch's pieces are added in object order
                double *dst = c.out + (size_t)run_patch[r] * n_bins;
                const double *src = run_out.data() + (size_t)r * n_bins;
                for (int b = 0; b < n_bins; ++b) dst[b] += src[b];
            }
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // nothing of this call is left in flight before the buffers go
    else (void)hipStreamSynchronize(stream);
    return e;
}

}  // namespace yawhist
