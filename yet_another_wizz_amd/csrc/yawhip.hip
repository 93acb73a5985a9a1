// yawhip.hip -- MI355X (gfx950 / CDNA4) angular pair counting: the count kernels, the item builders and the count call
// that plans and launches them (count_enqueue / count_finish / run_single, yawhip_count_pairs, yawhip_job_work), behind the C
// ABI of include/yawhip.h. The rest of the library lives in units of its own, joined by csrc/yawhip_internal.h:
//   yawhip_ingest.hip   catalogue upload, strip layouts and merged triple runs, yawhip_assign_patches (with their kernels);
//   yawhip_dense.hip    the dense epilogue on top of the count call: yawhip_count_pairs_dense(_batch), ..._rows_device;
//   yawhip_api.hip      contexts and options, error reporting, host-side grouping, and the wrappers of yawhip_hist.hip,
//                       yawhip_healpix.hip and yawhip_random.hip.
//
// Replaces the per-job loop of PatchLinkage.count_pairs (reference src/yaw/correlation/measurements.py:344-364):
// for each linked patch pair (p,q) and redshift bin k it counts, per fine angular bin e, the object
// pairs with  t[k][e] < s <= t[k][e+1],  s = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2  in float64 without
// FMA -- the predicate scipy's KDTree.count_neighbors applies behind AngularTree.count
// (src/yaw/catalog/trees.py:303-362).
//
// Design (wave64, no MFMA -- K=3 distances are not a contraction and bit parity forbids replacing the
// predicate by a dot-product form; DESIGN.md section 4 has the details and the measurements):
//   * catalogues live in HBM as SoA float64 columns x,y,z,(w) in two library-private orders, both made on the
//     device at upload (yawhip_ingest.hip, yawhip_sort.hip): (patch, z-bin, u) with a CSR offset table, u = the sort axis; and the
//     strip layout (patch, strip, u) -- strips of a global grid along a second axis, all bins together, bin id
//     per object -- whose runs can be paired across catalogues by grid index alone;
//   * k_build_items / k_build_items_strips turn the job table into work items (lane tile of c2) x (window of a
//     c1 segment or run): one thread per potential item decodes it arithmetically, binary-searches the window
//     |du| <= sqrt(t_max) and drops empty ones; one atomic per workgroup appends the rest -- for the float32 band
//     kernels into one of eight segments of the list, one per XCD (append_items);
//   * k_count (EXACT / FILTER, non-unit input): 256-thread workgroups, 256*R lane objects in registers, the
//     c1 segment streamed through LDS; 8 FP64 ops + compare per pair, or a conservative FP32 dot-product test
//     first and exact FP64 for its survivors. Per-lane private LDS histograms, fixed-order reduction;
//   * k_count_merged (SWEEP): single-wave workgroups, float32 only on chip (packed v_pk_fma_f32),
//     survivors queued per wave and evaluated 64 at a time in exact FP64; one item of the cross-correlation
//     path covers all redshift bins. AUTO uses it on layouts without strips;
//   * k_count_band32 / k_count_band32_one (BAND, what AUTO runs on strip layouts of unit vectors -- the headline;
//     csrc/yawhip_band32.inc): single-wave workgroups, the window of a lane tile staged in LDS by LDS-DMA from float32
//     images of the columns, every lane walks only the band |du| <= r of its objects, classifies every entry in
//     float32 against guard bands around the edges and decides the few inside a guard band with the exact FP64
//     predicate on the float64 columns (results identical to an all-float64 evaluation). The streamed side is read
//     from merged runs of three neighbouring strips (k_merge_triples, yawhip_ingest.hip) where such a window fits the stage;
//     k_count_band32_fine: the same for fine radial grids (separation weights); k_count_band: every entry in FP64.
// Unweighted counts: uint32 LDS histograms -> 64-bit integer atomics. Weighted sums: per-item slabs (LDS float64
// atomics private to one wave) reduced in a fixed two-level order -> bit-reproducible run to run. No floating
// point atomics in global memory.
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off (see yet_another_wizz_amd/build.py).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <functional>
#include <vector>

#include "yawhip_internal.h"

using namespace yawhip_detail;

namespace {
constexpr int WG = 256;      // threads per workgroup = 4 waves of 64
constexpr int STAGE = 256;   // streamed objects per LDS stage (one per thread)
constexpr int MSTAGE = 64;   // stage of the merged path: smaller -> less LDS -> more workgroups per CU
constexpr int MAX_EDGES = 512;
constexpr int BAND_MIN_STREAM_RUN = 64;  // AUTO: objects per run of the streamed side (as the typical object sees it) from which the band kernel is used
constexpr int64_t SYNC_GRID_MIN_ITEMS = 400000;  // potential items from which the count grid is sized exactly (one host sync)
constexpr int MAX_STRIP_REACH = 12;  // strip pairing is used while sqrt(t_max) <= 12 grid spacings
constexpr int COUNT_FLUSH_MASK = (1 << 13) - 1;  // k_count: stages between flushes of the 32-bit LDS counters (see there)
constexpr int MERGED_FLUSH_MASK = (1 << 16) - 1; // k_count_merged: 256 lane objects x 64 streamed objects per stage
constexpr double PAD_COORD = 4.0;  // padded lanes sit >= 3 away from any unit vector: s >= 9 > max t = 4

struct alignas(16) Obj {  // one streamed object in LDS: two 16-byte broadcast reads
    double x, y, z, w;
};

struct alignas(16) ObjF {  // its float32 image for the pre-filter: one 16-byte broadcast read
    float x, y, z, pad;
};

// Pre-filter guard (see k_count): |dot32 - a.b| <= 5.000001 u for unit vectors rounded to float32 and
// a mul + 2 fma evaluation (u = 2^-24); 8 u leaves room for |a|^2 deviating from 1 by < 1e-9 and for
// the rounding of the threshold itself.
constexpr double FILTER_GUARD = 8.0 * 5.9604644775390625e-8;

// ------------------------------------------------------------------------------------------------
// Spherical caps (strip grid in latitude, trimmed u-bands; DESIGN.md sections 3 and 4).
// A pair passes s <= t_max only if its chord |a - b| <= rwin = sqrt(t_max) (1 + 1e-12) + 1e-15 (the float64 rounding of s,
// see k_build_items). The DIRECTIONS of a and b are then at most the angle sep_angle(rwin) apart: |a|^2 is within
// UNIT_NORM_TOL of 1, so ||a| - 1| <= 5e-10 and |a^ - b^| <= |a - b| + 1e-9 (2e-9 is added). Two consequences:
//   * latitudes about any axis (atan2(v, hypot(u, w)), the direction's own) differ by at most that angle: the strip grid of
//     k_strip_index in latitude pairs runs whose grid indices differ by at most floor(theta / width) + 1;
//   * with alpha = acos(u^) the polar angle of a about the sort axis, every partner has polar angle alpha -/+ theta, i.e.
//     u^_b in [cos(min(pi, alpha + theta)), cos(max(0, alpha - theta))] = [u c - sqrt(1 - u^2) s, u c + sqrt(1 - u^2) s]
//     (c = cos theta, s = sin theta), -1 below where alpha + theta > pi (u < -c), +1 above where alpha < theta (u > c).
//     Both bounds are monotone in u, so the band of objects with keys in [u0, u1] runs from lo(u0) to hi(u1).
// The bounds are culling bounds only: classification and the exact float64 path do not see them.
inline double sep_angle(double rwin) { return 2.0 * std::asin(std::min(1.0, 0.5 * (rwin + 2e-9))); }

// float64 (item builder): the key u is a float64 coordinate, |u - u^| <= 5e-10 (unit norm); shifting u by 1e-9 outward keeps
// the exact bound below / above the one of u^, the clip decisions are widened by 1e-12 (rounding of cos theta), and the
// result by 2e-9 (|u_b - u^_b| <= 5e-10 for the partner's key, plus the double-rounding of the formula, ~1e-15).
__device__ __forceinline__ double cap_lo64(double u, double c, double s) {
    const double ul = fmax(u - 1e-9, -1.0);
    return ul <= -c + 1e-12 ? -1.0 - 2e-9 : fma(ul, c, -sqrt(fmax(fma(-ul, ul, 1.0), 0.0)) * s) - 2e-9;
}
__device__ __forceinline__ double cap_hi64(double u, double c, double s) {
    const double uh = fmin(u + 1e-9, 1.0);
    return uh >= c - 1e-12 ? 1.0 + 2e-9 : fma(uh, c, sqrt(fmax(fma(-uh, uh, 1.0), 0.0)) * s) + 2e-9;
}
// float32 (band kernels): the lane key u is the float32 image, |u - u^| <= 2^-25 + 5e-10 < 3.1e-8. Input shift 1e-7: the
// rounding of u - 1e-7 (<= 6e-8) still leaves ul <= u^. Clip decisions widened by 1.2e-7 (c rounded to float32: 3e-8, and
// the rounding of -c + 1.2e-7: 6e-8). The formula in float32: c and s rounded (6e-8 u, 6e-8 s), fma(-u, u, 1) one rounding
// relative to 1 - u^2 and sqrtf within 2 ulp (together 2e-7 relative, times s), the product and the final fma (6e-8 each),
// the margin's own subtraction (6e-8): at most 1.8e-7 + 3.2e-7 s; the partner's float32 image adds 3.1e-8. The margin
// CAP32_MARGIN = 8e-7 covers s <= 1 (3e-4 of the band half width r at the headline's r = 2.9e-3).
constexpr float CAP32_SHIFT = 1e-7f, CAP32_CLIP = 1.2e-7f, CAP32_MARGIN = 8e-7f;
__device__ __forceinline__ float cap_lo32(float u, float c, float s) {
    const float ul = fmaxf(u - CAP32_SHIFT, -1.0f);
    return ul <= -c + CAP32_CLIP ? -1.0f - CAP32_MARGIN : fmaf(ul, c, -sqrtf(fmaxf(fmaf(-ul, ul, 1.0f), 0.0f)) * s) - CAP32_MARGIN;
}
__device__ __forceinline__ float cap_hi32(float u, float c, float s) {
    const float uh = fminf(u + CAP32_SHIFT, 1.0f);
    return uh >= c - CAP32_CLIP ? 1.0f + CAP32_MARGIN : fmaf(uh, c, sqrtf(fmaxf(fmaf(-uh, uh, 1.0f), 0.0f)) * s) + CAP32_MARGIN;
}

constexpr int SLOT_MASK = 0x3fffffff;
__host__ __device__ inline int item_slot(const Item &it) { return it.slot & SLOT_MASK; }
__host__ __device__ inline int item_orient(const Item &it) { return (int)((unsigned)it.slot >> 30); }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int BUILD_BISECT = 32;  // most bisection steps of the strip builder inside a grid cell: as many as a 32-bit range can take

// ------------------------------------------------------------------------------------------------
// Item builder: one thread per potential item (slot, lane tile).
//   SWEEP = false: the item streams the whole c1 segment; record written at its own index.
//   SWEEP = true : segments are sorted by one coordinate u (the catalogue's sort axis, z by default),
//                  so the tile spans [u(a0), u(a_last)] and only c1 objects with u in
//                  [umin - rwin, umax + rwin] can satisfy s <= t_max (s >= du^2);
//                  rwin[k] = sqrt(t_max[k]) * (1 + 1e-12) + 1e-15 absorbs every rounding in
//                  s = fl(fl(dx^2 + dy^2) + dz^2) >= dz^2 (1 - 3 eps). Items with an empty window are
//                  dropped; survivors are appended with one atomic per workgroup (order is irrelevant).
// ------------------------------------------------------------------------------------------------
constexpr int EVAL_SLOTS = 256;  // statistics counters, one 64-byte line each (a single hot address would serialise)
constexpr int BUILD_WG = 1024;       // most threads per workgroup of the item builders
// Builder workgroups: one atomic per workgroup appends its items, so few large workgroups suit long lists (16 k atomics on
// the one counter cost 0.15 ms at 4 M potential items), but 1024 threads make 300 workgroups for 256 CUs at the headline
// and half the chip waits for the CUs that got two (+0.07 ms): 256 threads while that keeps the atomics below 4096.
constexpr int BUILD_WG_SMALL = 256;
inline int build_wg_for(int64_t n_pot) { return n_pot / 256 <= 4096 ? BUILD_WG_SMALL : BUILD_WG; }
constexpr int BUILD_PREFIX_LDS = 1024;  // job tables up to this many entries are searched in LDS by the strip builder (8 KB: no occupancy cost)

// Append the kept items of a builder workgroup to the item list and add its evaluated-pair total: ONE atomic
// per workgroup on each of the two counters. (They are single hot addresses -- with an atomic per wave the
// builders spent three quarters of their time queueing on them.) Order of the list is irrelevant.
// seg_cap > 0: the list is kept in ITEM_SEGS segments of seg_cap records, workgroup b appends to segment b % ITEM_SEGS and
// counts in that segment's own counter (ITEM_SEG_CTR): eight addresses take the atomics of a launch side by side (on one
// address the 1200 appends of the headline queue for 10 of the builder's 43 us), and a segment -- every eighth builder
// workgroup's tiles -- is the same mix of dense and sparse items as the whole list: the float32 band kernels give XCD x
// segment x.
constexpr int ITEM_SEGS = 8;
__host__ __device__ constexpr int ITEM_SEG_CTR(int seg) { return 12 + 8 * seg; }  // counters[]: one 64-byte line each
// Clock stamps of a call (wall_clock64: the constant 100 MHz counter) and the words of its tail, in free words of the counter
// block; they travel to the host with the counters (k_call_tail) and give yawhip_stats.kernel_ms / count_ms without an
// event between the kernels.
//   CTR_T_BUILD     the builder's first workgroup starts
//   SEG_EXIT_CTR(s) latest exit of a builder workgroup, one word per item segment: spread like the append counters (one
//                   shared word would take every workgroup's atomic in turn)
//   CTR_T_COUNTED   the first kernel behind the count kernel(s) starts (reductions, k_counts_to_double); the tail writes its
//                   own start here when there is none
//   CTR_T_TAIL      the tail's first workgroup starts
//   CTR_TICKET      the tail's workgroups draw tickets here (the last one to finish signs the call off); wraps to 0
//   CTR_DONE        host image only: the sequence number of the call whose results the pinned block holds
constexpr int CTR_T_BUILD = 1, CTR_T_COUNTED = 2, CTR_T_TAIL = 3, CTR_TICKET = 4, CTR_DONE = 6;
__host__ __device__ constexpr int SEG_EXIT_CTR(int seg) { return ITEM_SEG_CTR(seg) + 1; }
constexpr double CLOCK_MS = 1.0e-5;  // milliseconds per tick of wall_clock64
__device__ __forceinline__ void stamp_start(unsigned long long *__restrict__ counters, int word) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[word] = wall_clock64();
}
__device__ __forceinline__ void append_items(bool keep, const Item &it, unsigned long long work, Item *__restrict__ items,
                                             unsigned long long *__restrict__ counters, unsigned char *__restrict__ kept,
                                             unsigned long long seg_cap = 0) {
    if (keep && kept) kept[it.pot] = 1;  // weighted runs: this potential item will write its slab
    __shared__ unsigned int s_cnt[BUILD_WG / 64];
    __shared__ unsigned long long s_work[BUILD_WG / 64], s_base;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) work += __shfl_down(work, off, 64);
    if (lane == 0) {
        s_cnt[wave] = (unsigned int)__popcll(mask);
        s_work[wave] = work;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int total = 0;
        unsigned long long wsum = 0;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) {
            const unsigned int c = s_cnt[wv];
            s_cnt[wv] = total;  // exclusive prefix
            total += c;
            wsum += s_work[wv];
        }
        if (seg_cap) {
            const int seg = (int)(blockIdx.x % ITEM_SEGS);
            s_base = (unsigned long long)seg * seg_cap + (total ? atomicAdd(&counters[ITEM_SEG_CTR(seg)], (unsigned long long)total) : 0ull);
        } else {
            s_base = total ? atomicAdd(&counters[0], (unsigned long long)total) : 0ull;
        }
        if (wsum) atomicAdd(&counters[10 + 8 * (blockIdx.x & (EVAL_SLOTS - 1))], wsum);  // statistics, spread like the other totals
    }
    __syncthreads();
    if (keep) items[s_base + s_cnt[wave] + __popcll(mask & ((1ull << lane) - 1ull))] = it;
    if (threadIdx.x == 0) atomicMax(&counters[SEG_EXIT_CTR((int)(blockIdx.x % ITEM_SEGS))], (unsigned long long)wall_clock64());
}

template <bool SWEEP>
__global__ __launch_bounds__(BUILD_WG) void k_build_items(CatView c1, CatView c2, const int32_t *__restrict__ jobs,
                                                     const int64_t *__restrict__ prefix, int n_slots, int n_bins,
                                                     int tile, const double *__restrict__ rwin, int64_t n_pot,
                                                     Item *__restrict__ items, unsigned long long *__restrict__ counters,
                                                     unsigned char *__restrict__ kept) {
    stamp_start(counters, CTR_T_BUILD);
    const int64_t pot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    Item it{};
    unsigned long long work = 0;
    if (pot < n_pot) {
        int lo = 0, hi = n_slots;  // slot = largest s with prefix[s] <= pot
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= pot) lo = mid; else hi = mid;
        }
        const int slot = lo, job = slot / n_bins, k = slot - job * n_bins;
        const int p = jobs[2 * job], q = jobs[2 * job + 1];
        const int k1 = c1.nb == 1 ? 0 : k, k2 = c2.nb == 1 ? 0 : k;
        int64_t b0 = c1.off[(int64_t)p * c1.nb + k1], b1 = c1.off[(int64_t)p * c1.nb + k1 + 1];
        const int64_t a_seg1 = c2.off[(int64_t)q * c2.nb + k2 + 1];
        const int64_t a0 = c2.off[(int64_t)q * c2.nb + k2] + (pot - prefix[slot]) * (int64_t)tile;
        const int64_t a1 = a0 + tile < a_seg1 ? a0 + tile : a_seg1;
        if (SWEEP) {
            const double wlo = c2.key[a0] - rwin[k], whi = c2.key[a1 - 1] + rwin[k];
            int64_t l = b0, h = b1;  // first index with z >= wlo
            while (l < h) {
                const int64_t m = (l + h) >> 1;
                if (c1.key[m] < wlo) l = m + 1; else h = m;
            }
            const int64_t first = l;
            h = b1;  // first index with z > whi
            while (l < h) {
                const int64_t m = (l + h) >> 1;
                if (c1.key[m] <= whi) l = m + 1; else h = m;
            }
            b0 = first;
            b1 = l;
        }
        keep = b1 > b0;
        it.a0 = a0; it.b0[0] = b0; it.na = (int32_t)(a1 - a0); it.nb[0] = (int32_t)(b1 - b0); it.nwin = 1; it.slot = slot; it.pot = (int32_t)pot;
        work = keep ? (unsigned long long)it.na * (unsigned long long)it.nb[0] : 0ull;
    }
    if (SWEEP) {
        append_items(keep, it, work, items, counters, kept);
    } else {
        if (pot < n_pot) items[pot] = it;  // every potential item is kept
        append_items(false, it, work, items, counters, nullptr);
        if (pot == 0) counters[0] = (unsigned long long)n_pot;
    }
}

// ------------------------------------------------------------------------------------------------
// Item builder of the strip path. A job (p, q) is cut into potential items
//   (lane tile of a (patch q, strip) run of c2)  x  (one of the 2*reach+1 neighbouring strips of patch p in c1),
// enumerated arithmetically: no per-job tables travel from the host. One thread per potential item finds its
// job (prefix over jobs), its tile (prefix of tiles over the runs of c2) and the strip of c1 on the common
// grid; window search and compaction as in k_build_items<true>.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BUILD_WG) void k_build_items_strips(const DevTab *__restrict__ tabs, const JobRec *__restrict__ jobs,
                                                            const int64_t *__restrict__ prefix, int n_jobs, int reach,
                                                            int tile, double rwin, double cap_c, double cap_s, int swap,
                                                            int triple, int64_t n_pot,
                                                            Item *__restrict__ items, unsigned long long *__restrict__ counters,
                                                            unsigned char *__restrict__ kept, unsigned long long seg_cap) {
    // triple: the streamed side consists of merged triple runs (k_merge_triples) -- the host passes reach = 0 (one partner
    // run per lane tile: the triple centred on its strip) and the triples' offsets and grid index in the streamed table; their
    // sort key exists as float32 image only, so the window is widened by the rounding of a key (the count kernel searches
    // its bands in float32 with a margin of its own).
    stamp_start(counters, CTR_T_BUILD);
    const int64_t pot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool keep = false;
    Item it{};
    unsigned long long work = 0;
    // Every thread walks a chain of dependent loads (job -> tile -> runs -> windows); its length is the kernel's run time.
    // The job table is small: searched in LDS (one coalesced load instead of log2(jobs) round trips to L2).
    __shared__ int64_t s_prefix[BUILD_PREFIX_LDS];
    // ... and so are the six layout records: which one a thread needs depends on its job's orientation, so every pointer in
    // them would be a vector load of its own in front of the load it points to (five round trips of the chain)
    __shared__ DevTab s_tabs[6];
    static_assert(sizeof(DevTab) % 8 == 0, "DevTab is copied in 8-byte words");
    for (int e = threadIdx.x; e < (int)(6 * sizeof(DevTab) / 8); e += blockDim.x)
        reinterpret_cast<uint64_t *>(s_tabs)[e] = reinterpret_cast<const uint64_t *>(tabs)[e];
    const bool prefix_in_lds = n_jobs + 1 <= BUILD_PREFIX_LDS;
    if (prefix_in_lds)
        for (int e = threadIdx.x; e <= n_jobs; e += blockDim.x) s_prefix[e] = prefix[e];
    __syncthreads();
    if (pot < n_pot) {
        int lo = 0, hi = n_jobs;  // job = largest j with prefix[j] <= pot
        if (prefix_in_lds) {
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_prefix[mid] <= pot) lo = mid; else hi = mid;
            }
        } else {
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (prefix[mid] <= pot) lo = mid; else hi = mid;
            }
        }
        const int job = lo;
        const JobRec jr = jobs[job];
        const int o = jr.o & 3;  // orientation of the job: which pair of layouts it runs on
        it.pad_ = (jr.o >> 2) & 1;  // 1: diagonal job of a self count: lanes walk only the entries behind their own place (see k_merge_triples)
        // swap: the lane tiles come from the first catalogue of the job (the binned one), the windows from the second
        const DevTab &c1 = s_tabs[swap ? 3 + o : o], &c2 = s_tabs[swap ? o : 3 + o];
        const gf64p key1d = tab_key(c1), key2 = tab_key(c2);
        const gf32p key1f = c1.axis == 0 ? c1.qx : (c1.axis == 1 ? c1.qy : c1.qz);
        auto key1 = [&](int64_t i) { return triple ? (double)key1f[i] : key1d[i]; };
        // potential items of a job in the order (lane tile, group of neighbour offsets). One item carries up to MAX_WIN
        // neighbouring strips of the streamed group (all 2 * reach + 1 = 3 of them when the grid is as wide as the
        // largest separation): the lane tile is loaded once and its histogram flushed once for all of them.
        const int nd = 2 * reach + 1, ng = (nd + MAX_WIN - 1) / MAX_WIN;
        const int64_t local = pot - (prefix_in_lds ? s_prefix[job] : prefix[job]);
        // (a call has fewer than 2^31 potential items: 32-bit division, and none in the usual case of one group)
        const uint32_t local32 = (uint32_t)local, tl = ng == 1 ? local32 : local32 / (uint32_t)ng;
        const int g = (int)(local32 - tl * (uint32_t)ng);
        const TileRec tr = c2.tile_rec[jr.t_lo + tl];
        const int64_t r2 = tr.run, a0 = tr.a0, a1 = a0 + tr.na;
        const double kpad = triple ? 1.2e-7 : 0.0;  // float32 rounding of a streamed key (|u| <= 1: 2^-24)
        // (half bands: no lane of the tile looks at an entry in front of the tile's first object -- the window starts there)
        // cap_s > 0 (band_trim): the window is trimmed to the caps the tile's first and last objects can reach (sep_angle)
        double wlo = key2[a0] - (it.pad_ ? 0.0 : rwin) - kpad, whi = key2[a1 - 1] + rwin + kpad;
        if (cap_s > 0.0) {
            if (!it.pad_) wlo = cap_lo64(key2[a0], cap_c, cap_s) - kpad;
            whi = cap_hi64(key2[a1 - 1], cap_c, cap_s) + kpad;
        }
        it.a0 = a0; it.na = tr.na; it.nwin = 0;
        it.slot = (int32_t)((unsigned)job | ((unsigned)o << 30)); it.pot = (int32_t)pot;
        // The windows of the (up to) three partner runs are searched in lockstep: three independent chains of loads per
        // thread instead of one after the other (static indices throughout: everything stays in registers).
        // (bounds relative to the run's first entry, 32 bits: half the integer work of the search)
        int64_t wb[MAX_WIN];
        uint32_t sl[MAX_WIN], sh[MAX_WIN], ul[MAX_WIN], uh[MAX_WIN];
        int32_t wn[MAX_WIN];
#pragma unroll
        for (int j = 0; j < MAX_WIN; ++j) {
            const int dd = g * MAX_WIN + j;
            const int64_t s1 = r2 + jr.k_off + (dd - reach);
            const bool valid = dd < nd && s1 >= 0 && s1 < jr.n_strips1;
            const int64_t r1 = jr.vbase1 + (valid ? s1 : 0);
            int64_t b0 = 0, b1 = 0;
            if (valid) { b0 = c1.off[r1]; b1 = c1.off[r1 + 1]; }
            // four partner runs in five lie entirely before or behind the tile's window (neighbouring patches share a
            // boundary only): two loads settle those
            const bool some = b1 > b0;
            // (loads under their condition: the texture path is what this kernel is bound by, and it charges the lanes of a
            // load that are switched on; a wave whose tiles face no live run skips them altogether)
            double kfirst = 0.0, klast = 0.0;
            if (some) { kfirst = key1(b0); klast = key1(b1 - 1); }
            const bool live = some && !(klast < wlo || kfirst > whi);
            // the run's index along the sort axis narrows both searches to one cell (RunGrid)
            uint32_t l0 = 0, l1 = 0, u0 = 0, u1 = 0;
            if (live) {
                const double inv = c1.grid[r1].inv;
                const int cl = run_cell(wlo, kfirst, inv), cu = run_cell(whi, kfirst, inv);
                const uint32_t *gr = c1.grid[r1].g;
                l0 = gr[cl]; l1 = gr[cl + 1]; u0 = gr[cu]; u1 = gr[cu + 1];
            }
            wb[j] = b0;
            sl[j] = l0; sh[j] = l1; ul[j] = u0; uh[j] = u1;  // all 0 for a dead window
        }
        // lower bounds (first index with key >= wlo) and upper bounds (first index with key > whi), all at once
        for (int step = 0; step < BUILD_BISECT &&
                           ((sl[0] < sh[0]) | (sl[1] < sh[1]) | (sl[2] < sh[2]) | (ul[0] < uh[0]) | (ul[1] < uh[1]) | (ul[2] < uh[2])); ++step) {
            double kl[MAX_WIN], ku[MAX_WIN];
            uint32_t ml[MAX_WIN], mu[MAX_WIN];
#pragma unroll
            for (int j = 0; j < MAX_WIN; ++j) {  // the six probes of a step are issued together ...
                ml[j] = sl[j] + ((sh[j] - sl[j]) >> 1);
                mu[j] = ul[j] + ((uh[j] - ul[j]) >> 1);
                kl[j] = ku[j] = 0.0;
                if (sl[j] < sh[j]) kl[j] = key1(wb[j] + ml[j]);
                if (ul[j] < uh[j]) ku[j] = key1(wb[j] + mu[j]);
            }
#pragma unroll
            for (int j = 0; j < MAX_WIN; ++j) {  // ... and consumed after one wait
                if (sl[j] < sh[j]) { if (kl[j] < wlo) sl[j] = ml[j] + 1; else sh[j] = ml[j]; }
                if (ul[j] < uh[j]) { if (ku[j] <= whi) ul[j] = mu[j] + 1; else uh[j] = mu[j]; }
            }
        }
#pragma unroll
        for (int j = 0; j < MAX_WIN; ++j) {
            wb[j] += sl[j];
            wn[j] = (int32_t)(ul[j] - sl[j]);  // 0 for a dead window
        }
#pragma unroll
        for (int j = 0; j < MAX_WIN; ++j) {  // non-empty windows to the front
            if (wn[j] <= 0) continue;
            if (it.nwin == 0) { it.b0[0] = wb[j]; it.nb[0] = wn[j]; }
            else if (it.nwin == 1) { it.b0[1] = wb[j]; it.nb[1] = wn[j]; }
            else { it.b0[2] = wb[j]; it.nb[2] = wn[j]; }
            ++it.nwin;
            work += (unsigned long long)it.na * (unsigned long long)wn[j];
        }
        keep = it.nwin > 0;
    }
    append_items(keep, it, work, items, counters, kept, seg_cap);
}

// ------------------------------------------------------------------------------------------------
// Pair count kernel.
//   R         objects per lane (lane tile = 256*R objects of the c2 segment)
//   WEIGHTED  accumulate w_a*w_b in float64 (else count in uint32)
//   PRIVATE   per-lane private LDS histogram (deterministic); else one shared LDS histogram per
//             workgroup updated with LDS atomics (only used when E is too large for private ones)
//   FILTER    false: every pair is evaluated in FP64 (8 flop + 1 compare);
//             true:  every pair is first tested in FP32 as  a.b >= 1 - t_max/2 - guard  (mul + 2 fma
//                    + compare on the float32 images of the unit vectors); only survivors (a few
//                    1e-5 of the pairs) are evaluated with the exact FP64 predicate. The test is
//                    conservative: s = |a|^2 + |b|^2 - 2 a.b, so s <= t_max implies
//                    a.b >= 1 - t_max/2 - eps_norm, and the float32 dot product is within 5.000001 u
//                    of a.b; dthr[k] is that bound rounded down. A pair the filter drops therefore has
//                    s > t_max and belongs to no bin: results are bit-identical to FILTER=false.
// ------------------------------------------------------------------------------------------------
template <int R, bool WEIGHTED, bool PRIVATE, bool FILTER>
__global__ __launch_bounds__(WG) void k_count(CatView c1, CatView c2, const Item *__restrict__ items, int n_bins,
                                              int n_edges, const double *__restrict__ t,
                                              const float *__restrict__ dthr, int64_t item_base,
                                              unsigned long long *__restrict__ out_counts,
                                              double *__restrict__ partials,
                                              const unsigned long long *__restrict__ n_kept) {
    using HistT = typename std::conditional<WEIGHTED, double, unsigned int>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Obj *stage = reinterpret_cast<Obj *>(lds_raw);                                  // [2][STAGE]
    ObjF *stagef = reinterpret_cast<ObjF *>(lds_raw + 2 * STAGE * sizeof(Obj));     // [2][STAGE]
    double *thr = reinterpret_cast<double *>(lds_raw + 2 * STAGE * (sizeof(Obj) + sizeof(ObjF)));  // [n_edges]
    HistT *hist = reinterpret_cast<HistT *>(thr + ((n_edges + 1) & ~1));            // [nf][WG] or [nf]

    const int tid = threadIdx.x;
    const int nf = n_edges - 1;
    if ((unsigned long long)(item_base + blockIdx.x) >= *n_kept) return;  // grid = potential items; the builder kept fewer
    const Item it = items[item_base + blockIdx.x];
    const int slot = it.slot;
    const int k = slot % n_bins;
    const int64_t b0 = it.b0[0], b1 = it.b0[0] + it.nb[0];  // items of k_build_items carry one window
    const int64_t a0 = it.a0, a_seg1 = it.a0 + it.na;
    const int64_t item = it.pot;

    // lane objects (c2 side) -> registers; padded lanes are parked far away
    double ax[R], ay[R], az[R], aw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = a0 + (int64_t)r * WG + tid;
        const bool ok = i < a_seg1;
        ax[r] = ok ? c2.x[i] : PAD_COORD;
        ay[r] = ok ? c2.y[i] : PAD_COORD;
        az[r] = ok ? c2.z[i] : PAD_COORD;
        aw[r] = (WEIGHTED && ok && c2.w) ? c2.w[i] : (ok ? 1.0 : 0.0);
    }
    float fx[R], fy[R], fz[R];  // float32 images; a padded lane gets NaN -> its dot product fails every comparison
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool ok = a0 + (int64_t)r * WG + tid < a_seg1;
        fx[r] = ok ? (float)ax[r] : __builtin_nanf("");
        fy[r] = ok ? (float)ay[r] : 0.f;
        fz[r] = ok ? (float)az[r] : 0.f;
    }
    const float dmin = FILTER ? dthr[3 * k] : 0.f;

    for (int e = tid; e < n_edges; e += WG) thr[e] = t[(int64_t)k * n_edges + e];
    if (PRIVATE) {
        for (int j = 0; j < nf; ++j) hist[j * WG + tid] = HistT(0);
    } else {
        for (int j = tid; j < nf; j += WG) hist[j] = HistT(0);
    }
    const double tmax = t[(int64_t)k * n_edges + n_edges - 1];

    const int64_t nb_total = b1 - b0;
    const int nstages = (int)((nb_total + STAGE - 1) / STAGE);
    // LDS histogram(s) -> result: fixed-order tree reduction of the private histograms, then 64-bit integer atomics
    // (unweighted; the histogram is cleared and counting goes on) or the item's slab (weighted, once at the end)
    auto flush_counts = [&]() {
        if (PRIVATE) {
            for (int stride = WG / 2; stride > 0; stride >>= 1) {
                if (tid < stride)
                    for (int j = 0; j < nf; ++j) hist[j * WG + tid] += hist[j * WG + tid + stride];
                __syncthreads();
            }
        }
        for (int j = tid; j < nf; j += WG) {
            const HistT v = PRIVATE ? hist[j * WG] : hist[j];
            if (WEIGHTED) partials[item * nf + j] = (double)v;
            else if (v != HistT(0)) atomicAdd(&out_counts[(int64_t)slot * nf + j], (unsigned long long)v);
        }
        __syncthreads();
        if (PRIVATE) {
            for (int j = 0; j < nf; ++j) hist[j * WG + tid] = HistT(0);
        } else {
            for (int j = tid; j < nf; j += WG) hist[j] = HistT(0);
        }
        __syncthreads();
    };

    // stage 0
    {
        const int64_t i = b0 + tid;
        Obj o;
        const bool ok = i < b1;
        o.x = ok ? c1.x[i] : 0.0; o.y = ok ? c1.y[i] : 0.0; o.z = ok ? c1.z[i] : 0.0;
        o.w = (WEIGHTED && ok && c1.w) ? c1.w[i] : 1.0;
        stage[tid] = o;
        if (FILTER) stagef[tid] = ObjF{(float)o.x, (float)o.y, (float)o.z, 0.f};
    }
    __syncthreads();

    for (int st = 0; st < nstages; ++st) {
        const Obj *cur = stage + (st & 1) * STAGE;
        // issue the next stage's global loads early; they land in registers while we compute
        Obj nxt;
        const bool have_next = st + 1 < nstages;
        if (have_next) {
            const int64_t i = b0 + (int64_t)(st + 1) * STAGE + tid;
            const bool ok = i < b1;
            nxt.x = ok ? c1.x[i] : 0.0; nxt.y = ok ? c1.y[i] : 0.0; nxt.z = ok ? c1.z[i] : 0.0;
            nxt.w = (WEIGHTED && ok && c1.w) ? c1.w[i] : 1.0;
        }
        const int64_t left = nb_total - (int64_t)st * STAGE;
        const int n = left < STAGE ? (int)left : STAGE;

        const ObjF *curf = stagef + (st & 1) * STAGE;
        // exact evaluation + histogram update of lane object r against streamed object b
        auto settle = [&](int r, const Obj &b) {
            const double dx = ax[r] - b.x;
            const double dy = ay[r] - b.y;
            const double dz = az[r] - b.z;
            const double xx = dx * dx;
            const double yy = dy * dy;
            const double zz = dz * dz;
            const double sxy = xx + yy;
            const double s = sxy + zz;
            if (s <= tmax) {
                int cnt = 0;
                for (int e = 0; e < n_edges; ++e) cnt += (s > thr[e]) ? 1 : 0;
                if (cnt > 0) {  // t[cnt-1] < s <= t[cnt]
                    const HistT v = WEIGHTED ? HistT(aw[r] * b.w) : HistT(1);
                    if (PRIVATE) hist[(cnt - 1) * WG + tid] += v;
                    else atomicAdd(&hist[cnt - 1], v);
                }
            }
        };
        if (FILTER) {
            for (int i = 0; i < n; ++i) {
                const ObjF bf = curf[i];  // wave-wide broadcast read, 16 B
                float d[R];
                float best = -2.f;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    d[r] = __builtin_fmaf(fz[r], bf.z, __builtin_fmaf(fy[r], bf.y, fx[r] * bf.x));
                    best = fmaxf(best, d[r]);
                }
                if (__builtin_amdgcn_ballot_w64(best >= dmin) != 0ull) {  // rare: a pair may be inside the outer edge
                    const Obj b = cur[i];
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (d[r] >= dmin) settle(r, b);
                }
            }
        } else {
            for (int i = 0; i < n; ++i) {
                const Obj b = cur[i];  // wave-wide broadcast read
                double s[R];
                bool any = false;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double dx = ax[r] - b.x;
                    const double dy = ay[r] - b.y;
                    const double dz = az[r] - b.z;
                    const double xx = dx * dx;
                    const double yy = dy * dy;
                    const double zz = dz * dz;
                    const double sxy = xx + yy;
                    s[r] = sxy + zz;
                    any |= (s[r] <= tmax);
                }
                if (__builtin_amdgcn_ballot_w64(any) != 0ull) {  // rare: some lane has a pair inside the outer edge
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (s[r] <= tmax) settle(r, b);
                }
            }
        }

        if (have_next) {
            stage[((st + 1) & 1) * STAGE + tid] = nxt;
            if (FILTER) stagef[((st + 1) & 1) * STAGE + tid] = ObjF{(float)nxt.x, (float)nxt.y, (float)nxt.z, 0.f};
        }
        __syncthreads();
        // 32-bit counters: 256 * R lane objects (R <= 4) x 256 streamed objects per stage reach 2^32 after 2^14 stages
        // (a c1 segment of 4.2 M objects inside one wide bin): move them to the 64-bit result before that
        if (!WEIGHTED && (st & COUNT_FLUSH_MASK) == COUNT_FLUSH_MASK && st + 1 < nstages) flush_counts();
    }
    flush_counts();
}

// ------------------------------------------------------------------------------------------------
// Culling kernel (SWEEP). Cross-correlation form: c1 binned in redshift, c2 unbinned, unit vectors, both in
// their strip layouts (runs of (patch, strip), all bins together, bin id per object on the c1 side).
// A work item = (lane tile: 64*R consecutive objects of one run of c2) x (the window of one partner run of c1
// that can hold partners of the tile, whatever their bin). One wave = one workgroup = one item.
//
// Fast path (all pairs of the window): only float32 lives on chip. Lanes keep the float32 image of
// their R objects packed in pairs; the stream is staged in LDS 64 objects at a time as 16-byte records
// (xf, yf, zf, pre-filter threshold of the object's own bin), so per-bin scales cost nothing in the loop:
// per trip (two streamed objects, R = 2: 256 pairs) 6 v_pk_mul/fma_f32 + 2 v_max + 2 v_cmp, next trip
// prefetched from LDS. Stage entries outside the wave's own window are skipped (ballot + popcount).
//
// Survivors (the real pairs and a 1e-6 fringe): the owner lane pushes a 4-byte code (r, lane, stage
// slot) on its wave's queue; when 64 are waiting (or the stage ends) every lane takes one, gathers
// the two float64 positions from global memory (L2-hot: both were just read by this workgroup) and
// evaluates the exact predicate -- full lanes, one memory latency per 64 survivors. Hits go to a
// [B][E-1] histogram in LDS:
//   unweighted: uint32 LDS atomics (exact, order independent);
//   weighted:   one float64 histogram per wave, updated with wave-private LDS float64 atomics
//               (no other wave writes it => bit-reproducible sums, see the drain).
// One item covers all B bins, so the c2 tile is read once per job instead of once per (job, bin).
// ------------------------------------------------------------------------------------------------
typedef float v2f __attribute__((ext_vector_type(2)));
struct MergedView {
    const double *x, *y, *z, *w;  // w may be null
    const int32_t *k;             // bin id per object
};

// MERGED = true:  the cross-correlation form described above (c1 binned, c2 unbinned, strip layouts, one item for
//                 all bins).
// MERGED = false: per-bin items (job, bin, tile): every streamed object belongs to the item's bin. Serves the
//                 binned x binned counts of an autocorrelation -- on the per-(patch, bin) strip layouts when the lane
//                 side is dense enough, else on the plain (patch, bin, u) layout -- and everything without a common
//                 strip grid.
template <int R, bool WEIGHTED, bool NF1, bool MERGED>
__device__ __forceinline__ void count_merged_body(const DevTab *__restrict__ tabs, const Item *__restrict__ items,
                                                     int n_bins, int n_edges, const double *__restrict__ t,
                                                     const float *__restrict__ dthr, const double *__restrict__ rwin_k,
                                                     int64_t item_base, unsigned long long *__restrict__ out_counts,
                                                     double *__restrict__ partials,
                                                     const unsigned long long *__restrict__ counters) {
    using HistT = typename std::conditional<WEIGHTED, double, unsigned int>::type;
    constexpr int NHIST = WEIGHTED ? MWG / 64 : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    ObjF *stagef = reinterpret_cast<ObjF *>(lds_raw);                                // [2][MSTAGE]
    double *thr = reinterpret_cast<double *>(stagef + 2 * MSTAGE);                   // [nkb][n_edges]
    const int nkb_l = MERGED ? n_bins : 1;
    HistT *hist = reinterpret_cast<HistT *>(thr + (size_t)nkb_l * n_edges);          // [NHIST][nkb*nf]
    float *dth = reinterpret_cast<float *>(hist + (size_t)NHIST * nkb_l * (n_edges - 1));  // [nkb]
    unsigned int *candq = reinterpret_cast<unsigned int *>(dth + nkb_l);             // [MWG/64][64] survivor codes

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = n_edges - 1;
    const unsigned long long ticket = item_base + blockIdx.x;
    if (ticket >= counters[0]) return;  // never taken when the host sized the grid from the builder's count
    const Item it = items[ticket];
    const int o = item_orient(it), islot = item_slot(it);
    const DevTab T1 = tabs[o], T2 = tabs[3 + o];
    const MergedView c1{(const double *)T1.x, (const double *)T1.y, (const double *)T1.z, (const double *)T1.w, (const int32_t *)T1.k};
    const CatView c2{(const double *)T2.x, (const double *)T2.y, (const double *)T2.z, (const double *)T2.w, (const int64_t *)T2.off, 1,
                     (const double *)tab_key(T2), T2.axis};
    const int kfix = MERGED ? 0 : islot % n_bins;  // the item's bin (ordinary items)
    const int nkb = MERGED ? n_bins : 1;             // bins this item can add to
    const int nslots = nkb * nf;
    const double rwin = rwin_k[kfix];
    int64_t b0 = it.b0[0], b1 = it.b0[0] + it.nb[0];  // the current window (an item of the strip builder carries up to three)
    const int64_t a0 = it.a0, a_end = it.a0 + it.na;
    // wave-contiguous assignment: wave w owns objects [w*64R, (w+1)*64R) of the z-sorted tile, so its
    // own z-window is narrower than the workgroup's
    const int64_t wa0 = a0 + (int64_t)wave * (64 * R);

    // Everything the item needs from global memory is requested here, back to back, before the first use:
    // lane objects, the key range of the wave, the first stage of the stream, thresholds (one memory latency).
    int64_t nb_total = b1 - b0;
    int nstages = (int)((nb_total + MSTAGE - 1) / MSTAGE);
    constexpr int NPF = (MSTAGE + MWG - 1) / MWG;  // stage slots a thread fills
    struct Raw { double x, y, z; int k; bool in; };
    auto fetch_raw = [&](int64_t i) {  // streamed object i (clamped into the window: unconditional loads)
        Raw o;
        o.in = i < b1;
        const int64_t ic = o.in ? i : b0;
        o.x = c1.x[ic]; o.y = c1.y[ic]; o.z = c1.z[ic];
        o.k = MERGED ? c1.k[ic] : 0;
        return o;
    };
    auto finish = [&](const Raw &o) {  // float32 record; slots past the window get a threshold nothing passes
        return ObjF{(float)o.x, (float)o.y, (float)o.z, o.in ? dth[o.k] : 2.0f};
    };
    double lx[R], ly[R], lz[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = wa0 + (int64_t)r * 64 + lane;
        const int64_t ic = i < a_end ? i : a0;  // padded lanes read a valid object
        lx[r] = c2.x[ic]; ly[r] = c2.y[ic]; lz[r] = c2.z[ic];
    }
    int64_t wa1 = wa0 + 64 * R;
    if (wa1 > a_end) wa1 = a_end;
    const bool wave_has = wa0 < wa1;
    const double key_lo = c2.key[wave_has ? wa0 : a0], key_hi = c2.key[wave_has ? wa1 - 1 : a0];
    Raw first[NPF];
#pragma unroll
    for (int f = 0; f < NPF; ++f) first[f] = fetch_raw(b0 + f * MWG + tid);
    // threshold tables: the first MWG entries travel with the batch above (all of them in the standard
    // 30 bins x 2 edges case), the rest in ordinary loops
    const bool has_t0 = tid < nkb * n_edges, has_d0 = tid < nkb;
    const double t0 = t[(int64_t)kfix * n_edges + (has_t0 ? tid : 0)];
    const float d0 = dthr[3 * (kfix + (has_d0 ? tid : 0))];
    __builtin_amdgcn_sched_barrier(0);
    if (has_t0) thr[tid] = t0;
    if (has_d0) dth[tid] = d0;
    for (int e = tid + MWG; e < nkb * n_edges; e += MWG) thr[e] = t[(int64_t)kfix * n_edges + e];
    for (int e = tid + MWG; e < nkb; e += MWG) dth[e] = dthr[3 * (kfix + e)];
    for (int e = tid; e < NHIST * nslots; e += MWG) hist[e] = HistT(0);
    __syncthreads();

    float fx[R], fy[R], fz[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool ok = wa0 + (int64_t)r * 64 + lane < a_end;
        fx[r] = ok ? (float)lx[r] : __builtin_nanf("");  // padded lane: dot = NaN fails every comparison (thresholds
                                                          // are <= 0 for separations >= 90 degrees, so 0 would pass)
        fy[r] = ok ? (float)ly[r] : 0.f;
        fz[r] = ok ? (float)lz[r] : 0.f;
    }
    constexpr int RP = (R + 1) / 2;
    v2f px[RP], py[RP], pz[RP];  // the same, packed in pairs for v_pk_*_f32 (R = 1: the upper half idles on NaN)
#pragma unroll
    for (int q = 0; q < RP; ++q) {
        const int r1 = 2 * q + 1 < R ? 2 * q + 1 : 2 * q;
        px[q] = v2f{fx[2 * q], 2 * q + 1 < R ? fx[r1] : __builtin_nanf("")};
        py[q] = v2f{fy[2 * q], fy[r1]};
        pz[q] = v2f{fz[2 * q], fz[r1]};
    }
    // z-range of this wave's lane objects (+/- the window half width), as conservative float32 bounds
    // for comparison with the float32 z of the staged objects (monotone rounding keeps them conservative)
    float wz_lo = 4.0f, wz_hi = -4.0f;  // wave without objects: empty range
    if (wave_has) {
        const double lo = key_lo - rwin, hi = key_hi + rwin;
        wz_lo = (float)lo;
        if ((double)wz_lo > lo) wz_lo = nextafterf(wz_lo, -4.0f);
        wz_hi = (float)hi;
        if ((double)wz_hi < hi) wz_hi = nextafterf(wz_hi, 4.0f);
    }
#pragma unroll
    for (int f = 0; f < NPF; ++f)
        if (f * MWG + tid < MSTAGE) stagef[f * MWG + tid] = finish(first[f]);
    __syncthreads();

    auto flush_hist = [&]() {  // LDS histogram -> 64-bit result (unweighted: cleared, counting goes on) / the item's slab
        for (int idx = tid; idx < nslots; idx += MWG) {
            if (WEIGHTED) {
                double v = 0.0;
                for (int wv = 0; wv < NHIST; ++wv) v += reinterpret_cast<double *>(hist)[wv * nslots + idx];
                partials[(int64_t)it.pot * nslots + idx] = v;
            } else {
                const unsigned int v = reinterpret_cast<unsigned int *>(hist)[idx];
                if (v) atomicAdd(&out_counts[(int64_t)islot * nslots + idx], (unsigned long long)v);
                reinterpret_cast<unsigned int *>(hist)[idx] = 0u;
            }
        }
    };
    int qn = 0;  // entries in this wave's survivor queue (wave-uniform)
    for (int win = 0; win < it.nwin; ++win) {
    if (win > 0) {  // next window of the item: its first stage goes through the same double buffer
        b0 = win == 1 ? it.b0[1] : it.b0[2];
        b1 = b0 + (win == 1 ? it.nb[1] : it.nb[2]);
        nb_total = b1 - b0;
        nstages = (int)((nb_total + MSTAGE - 1) / MSTAGE);
#pragma unroll
        for (int f = 0; f < NPF; ++f) first[f] = fetch_raw(b0 + f * MWG + tid);
        __syncthreads();  // every lane is done with the previous window's last stage
#pragma unroll
        for (int f = 0; f < NPF; ++f)
            if (f * MWG + tid < MSTAGE) stagef[f * MWG + tid] = finish(first[f]);
        __syncthreads();
    }
    for (int st = 0; st < nstages; ++st) {
        const int cb = st & 1;
        const int64_t sb0 = b0 + (int64_t)st * MSTAGE;  // global index of stage slot 0
        Raw nxt[NPF];
        const bool have_next = st + 1 < nstages;
#pragma unroll
        for (int f = 0; f < NPF; ++f)
            if (have_next) nxt[f] = fetch_raw(sb0 + MSTAGE + f * MWG + tid);
        const int64_t left = nb_total - (int64_t)st * MSTAGE;
        const int n = left < MSTAGE ? (int)left : MSTAGE;
        const ObjF *curf = stagef + cb * MSTAGE;

        // Exact evaluation of the queued survivors, one per lane.
        auto drain = [&]() {
            if (qn == 0) return;
            int hslot = -1;
            double val = 0.0;
            if (lane < qn) {
                const unsigned int code = candq[wave * 64 + lane];
                const int64_t ia = wa0 + (code >> 8);         // (r * 64 + lane) of the owner
                const int64_t ib = sb0 + (code & 0xffu);      // stage slot
                // issue all gathers before the first use: one memory latency per drain, not three
                const double ax = c2.x[ia], ay = c2.y[ia], az = c2.z[ia];
                const double bx = c1.x[ib], by = c1.y[ib], bz = c1.z[ib];
                const int kb = MERGED ? c1.k[ib] : 0;
                double wa = 1.0, wb = 1.0;
                if (WEIGHTED) {
                    if (c2.w) wa = c2.w[ia];
                    if (c1.w) wb = c1.w[ib];
                }
                __builtin_amdgcn_sched_barrier(0);
                const double dx = ax - bx;
                const double dy = ay - by;
                const double dz = az - bz;
                const double xx = dx * dx;
                const double yy = dy * dy;
                const double zz = dz * dz;
                const double sxy = xx + yy;
                const double s = sxy + zz;
                const double *tk = thr + kb * n_edges;
                if (s > tk[0] && s <= tk[n_edges - 1]) {
                    if (NF1) {
                        hslot = kb;
                    } else {
                        int cnt = 0;
                        for (int e = 0; e < n_edges; ++e) cnt += (s > tk[e]) ? 1 : 0;
                        hslot = kb * nf + cnt - 1;  // t[cnt-1] < s <= t[cnt], cnt >= 1 because s > t[0]
                    }
                    if (WEIGHTED) val = wa * wb;
                }
            }
            if (!WEIGHTED) {
                if (hslot >= 0) atomicAdd(reinterpret_cast<unsigned int *>(hist) + hslot, 1u);
            } else {
                // One LDS float64 atomic for the whole wave (ds_add_f64). The histogram belongs to this wave
                // alone and a wave's LDS instructions execute in program order, so the only freedom is the order
                // in which the LDS unit serialises lanes of ONE instruction that hit the same slot -- a fixed
                // property of the hardware, not a race: sums are bit-reproducible from run to run
                // (tests/test_gpu_scale_properties.py checks that at 10M x 10M).
                double *wh = reinterpret_cast<double *>(hist) + wave * nslots;
                if (hslot >= 0) atomicAdd(&wh[hslot], val);
            }
            qn = 0;
        };
        // Owner lanes of the survivors of stage slot i push their code on the wave's queue.
        auto enqueue = [&](int i, const float (&d)[R], float dmin) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool pass = d[r] >= dmin;
                const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
                if (m == 0ull) continue;  // uniform
                const int cnt = __popcll(m);
                if (qn + cnt > 64) drain();
                if (pass) {
                    const int pos = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    candq[wave * 64 + pos] = ((unsigned)(r * 64 + lane) << 8) | (unsigned)i;
                }
                qn += cnt;
            }
        };

        // this wave's sub-range of the (z-sorted) stage: entries below wz_lo / above wz_hi cannot pair with it
        int i_lo = 0, i_hi = 0;
#pragma unroll
        for (int j = 0; j < MSTAGE / 64; ++j) {
            const int e = j * 64 + lane;
            const float ze = (&curf[e].x)[c2.axis];  // float32 image of the sorted coordinate
            i_lo += __popcll(__builtin_amdgcn_ballot_w64(e < n && ze < wz_lo));
            i_hi += __popcll(__builtin_amdgcn_ballot_w64(e < n && ze <= wz_hi));
        }
        i_lo &= ~1;
        if (i_lo > MSTAGE - 2) i_lo = MSTAGE - 2;  // keeps the first read inside the stage; the loop is then empty
        // two streamed objects per trip, next pair prefetched from LDS while this one is evaluated.
        // Slots past the window hold a threshold of 2 (nothing passes), so an odd tail needs no test.
        // One trip = two streamed objects against the R lane objects, in packed float32 (v_pk_mul/fma_f32:
        // two lane objects per instruction). The loop is unrolled over two trips with alternating register
        // sets so that the LDS prefetch of the next pair needs no register moves.
        auto trip = [&](int i, const ObjF &c0, const ObjF &c1r) {
            v2f e0[RP], e1[RP];
#pragma unroll
            for (int q = 0; q < RP; ++q) {
                e0[q] = __builtin_elementwise_fma(pz[q], v2f{c0.z, c0.z}, __builtin_elementwise_fma(py[q], v2f{c0.y, c0.y}, px[q] * v2f{c0.x, c0.x}));
                e1[q] = __builtin_elementwise_fma(pz[q], v2f{c1r.z, c1r.z}, __builtin_elementwise_fma(py[q], v2f{c1r.y, c1r.y}, px[q] * v2f{c1r.x, c1r.x}));
            }
            float d0[R], d1[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                d0[r] = (r & 1) ? e0[r >> 1].y : e0[r >> 1].x;
                d1[r] = (r & 1) ? e1[r >> 1].y : e1[r >> 1].x;
            }
            float best0 = d0[0], best1 = d1[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                best0 = fmaxf(best0, d0[r]);
                best1 = fmaxf(best1, d1[r]);
            }
            const bool p0 = best0 >= c0.pad, p1 = best1 >= c1r.pad;
            // wave masks straight from the compares (a bool that goes through a VGPR costs two VALU per test)
            const unsigned long long m0 = __builtin_amdgcn_ballot_w64(p0), m1 = __builtin_amdgcn_ballot_w64(p1);
            if ((m0 | m1) != 0ull) {
                if (m0 != 0ull) enqueue(i, d0, c0.pad);
                if (m1 != 0ull) enqueue(i + 1, d1, c1r.pad);
            }
        };
        // Slots past the window hold a threshold of 2 (nothing passes), so an odd tail needs no test.
        ObjF a0r = curf[i_lo], a1r = curf[i_lo + 1];
        for (int i = i_lo; i < i_hi; i += 4) {
            const int ib = i + 2 < MSTAGE ? i + 2 : MSTAGE - 2;
            const ObjF b0r = curf[ib], b1r = curf[ib + 1];
            trip(i, a0r, a1r);
            const int ia = i + 4 < MSTAGE ? i + 4 : MSTAGE - 2;
            a0r = curf[ia];
            a1r = curf[ia + 1];
            if (i + 2 < i_hi) trip(i + 2, b0r, b1r);
        }
        drain();  // codes refer to this stage's slots
#pragma unroll
        for (int f = 0; f < NPF; ++f)
            if (have_next && f * MWG + tid < MSTAGE) stagef[(cb ^ 1) * MSTAGE + f * MWG + tid] = finish(nxt[f]);
        __syncthreads();
        if (!WEIGHTED && (st & MERGED_FLUSH_MASK) == MERGED_FLUSH_MASK && have_next) {  // 32-bit counters: see k_count
            flush_hist();
            __syncthreads();
        }
    }
    if (!WEIGHTED && nstages > MERGED_FLUSH_MASK / 4 && win + 1 < it.nwin) {  // a long window: do not carry its counts into the next
        flush_hist();
        __syncthreads();
    }
    }

    flush_hist();
}

// The kernel proper. With one or two objects per lane the body fits 64 VGPRs without spilling, so the compiler is
// told to keep 8 waves per SIMD (80 VGPRs / 6 waves otherwise: -9 % time at the headline); with four objects per
// lane that limit would spill, the default allocation stays.
template <int R, bool WEIGHTED, bool NF1, bool MERGED>
__global__ __launch_bounds__(MWG) void k_count_merged(const DevTab *__restrict__ tabs, const Item *__restrict__ items, int n_bins,
                                                      int n_edges, const double *__restrict__ t, const float *__restrict__ dthr,
                                                      const double *__restrict__ rwin_k, int64_t item_base,
                                                      unsigned long long *__restrict__ out_counts, double *__restrict__ partials,
                                                      const unsigned long long *__restrict__ counters) {
    count_merged_body<R, WEIGHTED, NF1, MERGED>(tabs, items, n_bins, n_edges, t, dthr, rwin_k, item_base, out_counts, partials, counters);
}
template <int R, bool WEIGHTED, bool NF1, bool MERGED>
__global__ __launch_bounds__(MWG) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_count_merged_occ8(
    const DevTab *__restrict__ tabs, const Item *__restrict__ items, int n_bins, int n_edges, const double *__restrict__ t,
    const float *__restrict__ dthr, const double *__restrict__ rwin_k, int64_t item_base, unsigned long long *__restrict__ out_counts,
    double *__restrict__ partials, const unsigned long long *__restrict__ counters) {
    count_merged_body<R, WEIGHTED, NF1, MERGED>(tabs, items, n_bins, n_edges, t, dthr, rwin_k, item_base, out_counts, partials, counters);
}

template <int R, bool WEIGHTED, bool NF1, bool MERGED>
auto pick_count_merged() -> decltype(&k_count_merged<R, WEIGHTED, NF1, MERGED>) {
    if constexpr (R <= 2) return k_count_merged_occ8<R, WEIGHTED, NF1, MERGED>;
    else return k_count_merged<R, WEIGHTED, NF1, MERGED>;
}

// ------------------------------------------------------------------------------------------------
// Band kernel (BAND, the default). Same work items as k_count_merged -- (lane tile of 64*R consecutive objects of a
// c2 run) x (the window of a c1 run that can hold their partners) -- but the window is not evaluated as a full
// rectangle. Both sides are sorted along u, so the partners of ONE lane object inside the window are the contiguous
// index range with |du| <= r_win: a band of ~2 r_win * (objects per unit u) entries, of which about half are real
// pairs when the strips are about r_win wide (disc / bounding box), against 64*R + band entries per lane object for
// the rectangle. So:
//   * the window is staged in LDS once, as float64 SoA columns (x, y, z, bin id, weight), BCAP objects at a time;
//   * every lane object finds its own band [lo, hi) by two branch-free binary searches on the staged sort-axis column;
//   * the lane walks its band: per step one staged object per lane (consecutive lanes read consecutive addresses:
//     conflict-free ds_read_b64), the exact float64 predicate, and the histogram update -- no float32 pre-filter,
//     no survivor queue, no gathers from global memory.
// At the headline density a lane object meets ~14 entries per strip instead of ~200; every evaluated entry costs
// 8 FP64 operations, which is what the parity contract asks for anyway.
// Work distribution: the grid is sized on the host from the number of POTENTIAL items (no host round trip for the
// number the builder kept); a workgroup takes the kept items v = blockIdx.x, blockIdx.x + gridDim.x, ... and maps v
// to the item list so that the workgroups of one XCD (blockIdx.x mod 8, MI355X_MICROARCH.md "Workgroup dispatch")
// walk one contiguous eighth of the list: consecutive items share c1 runs and lane tiles, which then hit in that
// XCD's L2 instead of being fetched by all eight.
//   UNI: all redshift bins share one threshold row (angular scales): edges live in registers.
// ------------------------------------------------------------------------------------------------
constexpr int BCAP = 192;       // window objects per LDS stage. 192: the window of a 128-object lane tile at equal densities (128 +- 11
                                // entries + one band) fits in one stage; 6.2 KB -> 26 single-wave workgroups per CU. Measured
                                // 160 / 176 / 192 / 208 / 224: count kernel 0.545 / 0.529 / 0.523 / 0.535 / 0.531 ms at the headline
constexpr int N_CTR = 8 + 8 * EVAL_SLOTS;  // counters: [0] kept items, [8 + 8 i] band entries, [9 + 8 i] exact re-evaluations, [10 + 8 i] lane-tile x window pairs

// LDS image of a band workgroup. The staged window lives in float64 SoA columns filled by LDS-DMA (global_load_lds_dwordx4:
// 16 bytes per lane straight from HBM into LDS, no staging registers, no ds_write), one entry of slack per column for the
// sentinel. The columns sit in a STATIC array at fixed offsets 2064 bytes apart, with the small tables in the gaps:
//   * the walk addresses x, y, z and the bin id from one register with immediate offsets;
//   * two ds_read_b64 less than 2041 bytes, or a multiple of 512 bytes, apart would be fused into ds_read2_b64 /
//     ds_read2st64_b64, which take twice their LDS cycles.
// Weights, edge tables and histograms too large for the gaps follow in dynamic LDS.
constexpr int band_apart(int at_least, int from1, int from2) {  // next 16-byte aligned offset >= at_least that is no multiple of
    int v = (at_least + 15) & ~15;                              // 512 bytes away from from1 and from2 (and >= 2048 away: caller)
    while ((v - from1) % 512 == 0 || (v - from2) % 512 == 0) v += 16;
    return v;
}
constexpr int band_max(int a, int b) { return a > b ? a : b; }
template <int CAP>
struct BandLds {  // byte offsets inside the static LDS image of a band workgroup whose stage holds CAP entries
    static constexpr int COL = (CAP + 2) * 8;   // a float64 column: CAP entries + sentinel, 16-byte multiple
    static constexpr int KCOL = (CAP + 4) * 4;  // the bin-id column
    static constexpr int X = 0, K = COL;
    static constexpr int Y = band_apart(band_max(K + KCOL, X + 2048), X, X);
    static constexpr int H = Y + COL;           // small histogram (H_BYTES), then 64 dummy cells
    static constexpr int H_BYTES = 512;
    static constexpr int Z = band_apart(band_max(H + H_BYTES + 256, Y + 2048), Y, X);
    static constexpr int FIXED = Z + COL;
};
static_assert(BandLds<160>::Y == 2064 && BandLds<160>::Z == 4128 && BandLds<160>::FIXED == 5424, "band LDS image");
static_assert(BandLds<192>::FIXED == 6208, "band LDS image");
// Stage capacities the band kernel is compiled for. A stage should hold the whole window of a lane tile (the tile's own
// extent in streamed entries plus one band): a window cut into stages makes every stage wait for the longest clipped band
// while the lanes whose bands lie in the other stage idle (50M x 50M, bands of 216 entries: 400 trips per 256 lane objects
// with 288-entry stages against 219 in one stage).
// (416-entry stages were measured too: never ahead of 288 -- 23.3 / 23.3 ms at 50M x 50M, 0.70 / 0.59 ms at the headline.)
constexpr int BCAP_MID = 288;
inline int band_lds_fixed(int cap) { return cap == BCAP_MID ? BandLds<BCAP_MID>::FIXED : BandLds<BCAP>::FIXED; }
__host__ __device__ inline bool band_small_hist(bool weighted, int nslots, int hp) { return (size_t)nslots * hp * (weighted ? 8 : 4) <= 512; }
// dynamic LDS bytes of a band workgroup (host and device agree through this one function)
__host__ __device__ inline size_t band_lds_dynamic(bool weighted, bool need_thr, int nkb, int n_edges, int hp, int cap, int thr_rows) {
    const int nslots = nkb * (n_edges - 1);
    return (weighted ? (size_t)(cap + 2) * 8 : 0) + (need_thr ? (size_t)thr_rows * n_edges * sizeof(double) : 0) +
           (band_small_hist(weighted, nslots, hp) ? 0 : (size_t)nslots * hp * (weighted ? 8 : 4)) + 16;
}
typedef __attribute__((address_space(3))) unsigned char lds_byte;
__device__ __forceinline__ __attribute__((address_space(3))) void *lds_ptr(unsigned addr) { return (__attribute__((address_space(3))) void *)(size_t)addr; }
__device__ __forceinline__ double lds_f64(unsigned addr) { return *(const __attribute__((address_space(3))) double *)(size_t)addr; }
__device__ __forceinline__ int lds_i32(unsigned addr) { return *(const __attribute__((address_space(3))) int *)(size_t)addr; }

// Maximum of a non-negative int over the 64 lanes of the wave, as a scalar: four row shifts, two row broadcasts (DPP, in
// the VALU) and one readlane -- the shuffle form goes through the LDS crossbar six times, each with its own wait.
__device__ __forceinline__ int wave_max_nonneg(int v) {
    // update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl): lanes without a source lane keep old = 0, the identity
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));  // row_shr:8 -> lane 15 of a row holds the row's maximum
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// Sum of an unsigned int over the 64 lanes, in lane 63 (same DPP steps; lanes without a source add 0).
__device__ __forceinline__ unsigned int wave_sum_lane63(unsigned int v) {
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// NE: edges per bin known at compile time (2: one fine bin; 3, 4: edges in registers when every bin -- or the item -- has one
// row of them); 0: any number, edge table in LDS.
template <int R, int CAP, bool WEIGHTED, int NE, bool MERGED, bool UNI>
__global__ __launch_bounds__(64) void k_count_band(const DevTab *__restrict__ tabs, const Item *__restrict__ items, int n_bins,
                                                   int n_edges, const double *__restrict__ t,
                                                   const double *__restrict__ rwin_k, unsigned flush_mask, int hp_shift,
                                                   int batch_log2, unsigned long long *__restrict__ out_counts,
                                                   double *__restrict__ partials,
                                                   unsigned long long *__restrict__ counters) {
    using HistT = typename std::conditional<WEIGHTED, double, unsigned int>::type;
    constexpr bool NF1 = NE == 2;
    constexpr bool REG_EDGES = NE >= 2 && (!MERGED || UNI);  // the item's edges live in registers
    constexpr bool NEED_THR = !REG_EDGES;                    // else: edge table in LDS
    constexpr int HB = WEIGHTED ? 3 : 2;                 // log2 of the bytes of a histogram cell
    using L = BandLds<CAP>;
    constexpr int LDS_X = L::X, LDS_K = L::K, LDS_Y = L::Y, LDS_H = L::H, LDS_Z = L::Z, LDS_H_BYTES = L::H_BYTES, BCOL = L::COL;
    __shared__ __attribute__((aligned(16))) unsigned char lds_fix[L::FIXED];
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
    const int nkb = MERGED ? n_bins : 1;  // bins one item can add to
    const int nf = NF1 ? 1 : n_edges - 1;
    const int nslots = nkb * nf;
    const int hp = 1 << hp_shift;  // copies of the histogram (lanes spread over them: fewer same-address LDS atomics)
    double *sx = reinterpret_cast<double *>(lds_fix + LDS_X);
    double *sy = reinterpret_cast<double *>(lds_fix + LDS_Y);
    double *sz = reinterpret_cast<double *>(lds_fix + LDS_Z);
    int *sk = reinterpret_cast<int *>(lds_fix + LDS_K);
    unsigned char *p = lds_dyn;
    double *sw = reinterpret_cast<double *>(p); if (WEIGHTED) p += BCOL;
    constexpr bool ROW1 = !(MERGED && !UNI);          // one edge row: every bin (or the item's only bin) shares it
    const int thr_rows = ROW1 ? 1 : nkb;
    double *thr = reinterpret_cast<double *>(p); if (NEED_THR) p += (size_t)thr_rows * n_edges * sizeof(double);  // [thr_rows][n_edges]
    const bool small_hist = band_small_hist(WEIGHTED, nslots, hp);
    HistT *hist = reinterpret_cast<HistT *>(small_hist ? lds_fix + LDS_H : p);                                // [nslots][hp]
    unsigned int *dummy = reinterpret_cast<unsigned int *>(lds_fix + LDS_H + LDS_H_BYTES);                    // [64] one cell per lane for misses
    const int lane = threadIdx.x;
    // LDS addresses (32 bit) the walk works with
    const unsigned a_sx = (unsigned)(size_t)(lds_byte *)(lds_fix + LDS_X);
    const unsigned a_sw = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(sw);
    const unsigned a_cell = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(hist) + ((lane & (hp - 1)) << HB);  // this lane's copy of cell 0
    const unsigned a_dummy = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(dummy + lane);
    const int ksh = hp_shift + HB;                  // slot number -> byte offset of its first histogram cell

    const unsigned long long n_kept = counters[0];
    const unsigned long long chunk = (n_kept + 7) >> 3;  // items per XCD
    // A workgroup takes 2^batch_log2 CONSECUTIVE items at a time (default: one) and carries its (unweighted) histogram from
    // one to the next while they add to the same output slot -- consecutive items are lane tiles of one job -- so that a
    // histogram of hundreds of cells goes to global memory once per batch. Off by default, see the launch.
    const unsigned long long n_batches = (chunk + (1ull << batch_log2) - 1) >> batch_log2;
    for (int e = lane; e < nslots * hp; e += 64) hist[e] = HistT(0);  // every flush leaves the histogram zeroed again
    unsigned int cnt1 = 0;             // NF1 && !MERGED: the only counter lives in a register
    unsigned stage_no = 0;
    int pend_slot = -1;                // output slot the histogram holds counts for (unweighted)
    int thr_k = -1;                    // bin whose edge row the LDS table holds
    auto flush_counts = [&](int slot_out) {  // LDS histogram / register counter -> global result (unweighted)
        if (NF1 && !MERGED) {
            if (lane == 0 && cnt1) atomicAdd(&out_counts[(int64_t)slot_out * nslots], (unsigned long long)cnt1);  // every lane holds the wave total
            cnt1 = 0;
            return;
        }
        __syncthreads();
        for (int idx = lane; idx < nslots; idx += 64) {
            unsigned int c = 0;
            for (int h = 0; h < hp; ++h) {
                c += (unsigned int)hist[idx * hp + h];
                hist[idx * hp + h] = HistT(0);
            }
            if (c) atomicAdd(&out_counts[(int64_t)slot_out * nslots + idx], (unsigned long long)c);
        }
    };
    for (unsigned long long v = blockIdx.x;; v += gridDim.x) {
        if ((v >> 3) >= n_batches) break;
      for (unsigned long long j = (v >> 3) << batch_log2; j < (((v >> 3) + 1) << batch_log2) && j < chunk; ++j) {
        const unsigned long long ticket = (v & 7) * chunk + j;
        if (ticket >= n_kept) break;  // short last eighth
        const Item it = items[ticket];
        const int o = item_orient(it), islot = item_slot(it);
        if (!WEIGHTED) {
            if (pend_slot >= 0 && pend_slot != islot) flush_counts(pend_slot);
            pend_slot = islot;
        }
        const DevTab c1 = tabs[o], c2 = tabs[3 + o];  // wave-uniform: scalar loads
        const int kfix = MERGED ? 0 : islot % n_bins;
        const double rwin = rwin_k[kfix];
        int64_t b0 = it.b0[0], nb_total = it.nb[0];  // the current window (an item of the strip builder carries up to three)

        __syncthreads();  // the previous item of this workgroup has left the LDS
        // stage of the window -> LDS, 16 bytes per lane and instruction; lanes past the stage stay out of it.
        // (wave-uniform 64-bit bases + 32-bit lane offsets: the loads take their base from scalar registers)
        auto stage_in = [&](int64_t first, int n) {
            const gf64p gx = c1.x + b0 + first, gy = c1.y + b0 + first, gz = c1.z + b0 + first;
#pragma unroll
            for (int c = 0; c < (CAP + 127) / 128; ++c) {
                const unsigned e = (unsigned)(c * 128 + 2 * lane);
                if (e < (unsigned)n) {
                    __builtin_amdgcn_global_load_lds(gx + e, lds_ptr(a_sx + c * 1024), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds(gy + e, lds_ptr(a_sx + (LDS_Y - LDS_X) + c * 1024), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds(gz + e, lds_ptr(a_sx + (LDS_Z - LDS_X) + c * 1024), 16, 0, 0);
                    if (WEIGHTED && c1.w) __builtin_amdgcn_global_load_lds(c1.w + b0 + first + e, lds_ptr(a_sw + c * 1024), 16, 0, 0);
                }
            }
            if (MERGED) {
#pragma unroll
                for (int c = 0; c < (CAP + 255) / 256; ++c) {
                    const unsigned e = (unsigned)(c * 256 + 4 * lane);
                    if (e < (unsigned)n)
                        __builtin_amdgcn_global_load_lds(c1.k + b0 + first + e, lds_ptr(a_sx + (LDS_K - LDS_X) + c * 1024), 16, 0, 0);
                }
            }
        };
        stage_in(0, (int)(nb_total < CAP ? nb_total : CAP));
        // lane objects and thresholds while the stage is in flight
        // A lane holds R NEIGHBOURING objects of the (u-sorted) tile: their bands overlap almost completely, so the lane
        // walks their union once -- one read of an entry serves R evaluations, two searches serve R objects.
        double ax[R], ay[R], az[R], aw[R];
        int n_own = (int)it.na - lane * R;  // objects of this lane (<= 0: none)
        n_own = n_own < 0 ? 0 : (n_own > R ? R : n_own);
        {
            const gf64p px = c2.x + it.a0, py = c2.y + it.a0, pz = c2.z + it.a0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool have = r < n_own;
                const unsigned ic = have ? (unsigned)(lane * R + r) : 0u;
                ax[r] = px[ic]; ay[r] = py[ic]; az[r] = pz[ic];
                aw[r] = (WEIGHTED && c2.w) ? (c2.w + it.a0)[ic] : 1.0;
            }
        }
        double ed[NE >= 2 ? NE : 1];  // edges of the item's bin (or of every bin) in registers
        if (REG_EDGES) {
#pragma unroll
            for (int q = 0; q < NE; ++q) ed[q] = t[(int64_t)kfix * n_edges + q];
        }
        if (NEED_THR && thr_k != kfix) {  // (the barriers of the first stage come before anyone reads it)
            for (int e = lane; e < thr_rows * n_edges; e += 64) thr[e] = t[(int64_t)kfix * n_edges + e];
            thr_k = kfix;
        }
        // outer edges of the one row in registers; largest power of two <= the number of inner edges (fine-bin search)
        const double e_lo = NEED_THR && ROW1 ? t[(int64_t)kfix * n_edges] : 0.0;
        const double e_hi = NEED_THR && ROW1 ? t[(int64_t)kfix * n_edges + n_edges - 1] : 0.0;
        const int edge_top = n_edges > 2 ? 1 << (31 - __builtin_clz(n_edges - 2)) : 0;
        // the lane's band: from the first object's lower to the last object's upper bound (the tile is sorted along u)
        double klo, khi;
        {
            const int last_r = n_own > 0 ? n_own - 1 : 0;
            double u_first = c2.axis == 0 ? ax[0] : (c2.axis == 1 ? ay[0] : az[0]), u_last = u_first;
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (r == last_r) u_last = c2.axis == 0 ? ax[r] : (c2.axis == 1 ? ay[r] : az[r]);
            klo = u_first - rwin;
            khi = u_last + rwin;
        }
#pragma unroll
        for (int r = 0; r < R; ++r)  // slots without an object sit beyond every edge of every entry
            if (r >= n_own) { ax[r] = PAD_COORD; ay[r] = PAD_COORD; az[r] = PAD_COORD; aw[r] = 0.0; }
        unsigned int nev = 0;              // band entries this lane evaluated
        auto flush_slab = [&]() {  // weighted: LDS histogram -> the item's slab
            __syncthreads();
            for (int idx = lane; idx < nslots; idx += 64) {
                double c = 0.0;
                for (int h = 0; h < hp; ++h) {  // fixed order: reproducible weighted sums
                    c += (double)hist[idx * hp + h];
                    hist[idx * hp + h] = HistT(0);
                }
                partials[(int64_t)it.pot * nslots + idx] = c;
            }
        };

        for (int win = 0; win < it.nwin; ++win) {
        if (win > 0) {
            b0 = win == 1 ? it.b0[1] : it.b0[2];
            nb_total = win == 1 ? it.nb[1] : it.nb[2];
        }
        for (int64_t st0 = 0; st0 < nb_total; st0 += CAP, ++stage_no) {
            const int n = (int)(nb_total - st0 < CAP ? nb_total - st0 : CAP);
            if (st0 > 0 || win > 0) {
                __syncthreads();  // every lane is done with the previous stage
                stage_in(st0, n);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stage has landed: only the wave's own vmcnt orders LDS reads behind its LDS-DMA
            __syncthreads();
            if (lane == 0) {  // sentinel behind the stage: lanes whose band has ended read it; it is beyond every edge
                sx[n] = PAD_COORD; sy[n] = PAD_COORD; sz[n] = PAD_COORD;
                if (WEIGHTED) sw[n] = 0.0;
                if (MERGED) sk[n] = 0;
            }
            if (WEIGHTED && !c1.w)
                for (int e = lane; e < n; e += 64) sw[e] = 1.0;
            __syncthreads();
            // band of the lane inside this stage: [lo, hi) = entries with klo <= key <= khi
            // Both searches run on LDS byte addresses: q = address of entry (lo - 1). A probe beyond the stage is clamped
            // onto the sentinel (4.0 > every key bound), which fails both comparisons by itself -- no index checks, and
            // hipcc keeps the loop free of branches (the index form compiled to twice the instructions, with the
            // second read under an exec branch).
            const unsigned a_key = a_sx + (c2.axis == 0 ? 0u : (c2.axis == 1 ? (unsigned)(LDS_Y - LDS_X) : (unsigned)(LDS_Z - LDS_X)));
            const unsigned a_sent = a_key + ((unsigned)n << 3);
            unsigned ql = a_key - 8u, qh = ql;
            for (unsigned step8 = 8u << (31 - __builtin_clz(n)); step8 >= 8u; step8 >>= 1) {  // largest power of two <= n
                const unsigned pl = ql + step8, ph = qh + step8;
                const double kl = lds_f64(pl < a_sent ? pl : a_sent), kh = lds_f64(ph < a_sent ? ph : a_sent);
                ql = kl < klo ? pl : ql;    // entries [0, lo) have key <  klo
                qh = kh <= khi ? ph : qh;   // entries [0, hi) have key <= khi
            }
            int lo = (int)((ql + 8u - a_key) >> 3), hi = (int)((qh + 8u - a_key) >> 3);
            if (n_own == 0) lo = hi = n;  // lanes without an object walk the sentinel
            int len = hi - lo;
            nev += (unsigned int)(len * n_own);
            const int steps = wave_max_nonneg(len);  // the longest band of the wave: uniform trip count

            // Walk the band, one entry per trip, evaluated against the lane's R objects. A lane whose band has ended moves
            // on through the window (entries beyond a band have |du| > r_win, hence s > every upper edge: they fail the
            // predicate by themselves, as do the band's entries that lie outside the narrower band of one of the R
            // objects) and parks on the sentinel. Occupancy, not a software pipeline inside the wave, covers the LDS
            // latency of a trip (the pipeline would cost the registers that occupancy needs).
            unsigned cur = a_sx + ((unsigned)lo << 3);  // LDS address of the next entry's x; y, z, bin id at fixed distances
            const unsigned last = a_sx + ((unsigned)n << 3);
            for (int s = 0; s < steps; ++s) {
                const unsigned a8 = cur < last ? cur : last;
                cur += 8;
                const double ex = lds_f64(a8);
                const double ey = lds_f64(a8 + (LDS_Y - LDS_X));
                const double ez = lds_f64(a8 + (LDS_Z - LDS_X));
                const double ew = WEIGHTED ? lds_f64(a8 - a_sx + a_sw) : 1.0;
                const int ek = MERGED ? lds_i32(((a8 - a_sx) >> 1) + a_sx + (LDS_K - LDS_X)) : 0;
                // edge row of the entry's bin and its outer edges: once per entry, not per evaluation, and without
                // conditions around the reads (hipcc turned `a && b` over two LDS reads into exec branches with full waits)
                const double *tk = thr + ((NEED_THR && !ROW1) ? ek * n_edges : 0);
                const double t_first = (NEED_THR && !ROW1) ? tk[0] : e_lo, t_last = (NEED_THR && !ROW1) ? tk[n_edges - 1] : e_hi;
                if constexpr (WEIGHTED && NF1 && R > 1) {
                    // One fine bin: the R evaluations of an entry add to the same cell (the entry's bin), and neighbouring
                    // objects mostly hit the same entries -- their products are summed in registers and go to the LDS as ONE
                    // float64 atomic (those are slow: ~1 lane per cycle). Fixed order inside the lane: still reproducible.
                    double acc = 0.0;
                    bool any = false;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double dx = ax[r] - ex, dy = ay[r] - ey, dz = az[r] - ez;
                        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                        const double sxy2 = xx + yy;
                        const double sd = sxy2 + zz;
                        const bool in = REG_EDGES ? (sd > ed[0]) & (sd <= ed[NE >= 2 ? NE - 1 : 0]) : (sd > t_first) & (sd <= t_last);
                        acc += in ? aw[r] * ew : 0.0;
                        any |= in;
                    }
                    if (any)
                        (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(size_t)(((unsigned)ek << ksh) + a_cell), acc,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if constexpr (!REG_EDGES && !NF1) {
                    // Many edges (separation weights: ~50 fine bins): the fine bins of the R evaluations are searched in
                    // lockstep and for every lane -- R independent chains of LDS reads instead of one after the other under a
                    // branch; a miss ends in some valid bin and goes to the dummy cell.
                    double sdv[R];
                    bool inv[R];
                    int c[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double dx = ax[r] - ex, dy = ay[r] - ey, dz = az[r] - ez;
                        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                        const double sxy2 = xx + yy;
                        sdv[r] = sxy2 + zz;
                        inv[r] = (sdv[r] > t_first) & (sdv[r] <= t_last);
                        c[r] = 0;
                    }
                    for (int step = edge_top; step > 0; step >>= 1) {  // fine bin = number of inner edges below s
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const int probe = c[r] + step;
                            c[r] = sdv[r] > tk[probe < n_edges - 1 ? probe : n_edges - 1] ? probe : c[r];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const unsigned cell = ((unsigned)(ek * nf + c[r]) << ksh) + a_cell;  // t[c] < s <= t[c + 1]
                        if constexpr (WEIGHTED) {
                            if (inv[r])
                                (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(size_t)cell, aw[r] * ew,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        } else {
                            (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)(inv[r] ? cell : a_dummy),
                                                         1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    double bx[R], by[R], bz[R], bw[R];
                    int kb[R];
                    bx[r] = ex; by[r] = ey; bz[r] = ez; bw[r] = ew; kb[r] = ek;
                    const double dx = ax[r] - bx[r];
                    const double dy = ay[r] - by[r];
                    const double dz = az[r] - bz[r];
                    const double xx = dx * dx;
                    const double yy = dy * dy;
                    const double zz = dz * dz;
                    const double sxy2 = xx + yy;
                    const double sd = sxy2 + zz;
                    bool in;
                    int slot = kb[r] * nf;
                    if constexpr (REG_EDGES) {
                        in = sd > ed[0] && sd <= ed[NE - 1];
                        if constexpr (NE >= 3) slot += (sd > ed[1]) ? 1 : 0;  // inner edges: t[c-1] < s <= t[c]
                        if constexpr (NE >= 4) slot += (sd > ed[2]) ? 1 : 0;
                    } else {
                        in = (sd > t_first) & (sd <= t_last);
                    }
                    if (NF1 && !MERGED && !WEIGHTED) {
                        cnt1 += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(in));
                    } else if ((REG_EDGES || NF1) && !WEIGHTED) {  // the slot is known without a search over the edges
                        // Branch-free: a miss adds to the lane's own dummy cell. (Under a branch the compiler can no longer
                        // count the LDS operations in flight and drains them all before every evaluation.)
                        const unsigned cell = in ? ((unsigned)slot << ksh) + a_cell : a_dummy;
                        (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)cell, 1u,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else if (in) {
                        if constexpr (!REG_EDGES) {
                            // fine bin = number of inner edges below s: a branch-free binary search over the sorted row
                            // (a probe past the inner edges reads the last edge, which s does not exceed)
                            int c = 0;
                            for (int step = edge_top; step > 0; step >>= 1) {
                                const int probe = c + step;
                                c = sd > tk[probe < n_edges - 1 ? probe : n_edges - 1] ? probe : c;
                            }
                            slot += c;  // t[c] < s <= t[c + 1]
                        }
                        // The histogram belongs to this wave alone: integer adds are exact; float64 adds of ONE instruction
                        // that hit the same cell are serialised by the LDS in a fixed lane order -> reproducible sums.
                        const unsigned cell = ((unsigned)slot << ksh) + a_cell;
                        if constexpr (WEIGHTED)
                            (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(size_t)cell, aw[r] * bw[r],
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        else
                            (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)cell, 1u,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                }
            }
            // 64*R lane objects x BCAP entries per stage: a uint32 counter cannot wrap within flush_mask + 1 stages
            if (!WEIGHTED && (stage_no & flush_mask) == flush_mask) flush_counts(islot);
        }
        }
        if (WEIGHTED) flush_slab();
        // evaluated band entries of the item -> one of EVAL_SLOTS counters (statistics)
        for (int off = 32; off > 0; off >>= 1) nev += __shfl_down(nev, off, 64);
        if (lane == 0 && nev) atomicAdd(&counters[8 + 8 * (ticket & (EVAL_SLOTS - 1))], (unsigned long long)nev);
      }
        if (!WEIGHTED && pend_slot >= 0) {  // end of the batch
            flush_counts(pend_slot);
            pend_slot = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Band kernel, float32 classification (BAND on strip layouts of unit vectors).
// Same items and the same walk as k_count_band, but an entry is decided in FLOAT32 wherever float32 can decide it:
//   * both catalogues keep a float32 image of every strip layout, 16 bytes per object {x, y, z, bin id} (DevTab::q);
//     the window is staged from it by LDS-DMA (one dwordx4 per entry) and read back with one ds_read_b128;
//   * s32 = fma(dz, dz, fma(dy, dy, dx * dx)) on the float32 images, two lane objects per packed instruction
//     (v_pk_add / v_pk_mul / v_pk_fma_f32: 7 VALU for two evaluations instead of 16 FP64 operations);
//   * for unit vectors |s32 - s| <= g(t) = 2.1e-7 sqrt(t) + 5e-7 t + 1e-12 around an edge t (rounding of the images to
//     float32: 2^-25 per coordinate -- |x| <= 1, and values a hair above 1 round to 1 --, of the differences: 2^-24
//     relative, hence |error of d_i| <= 6e-8 (1 + |d_i|) and 2 |d| sqrt(3) 6e-8 on the sum of squares; of the three-term
//     sum: 3 x 2^-24 relative), so s32 < t - g proves s <= t and
//     s32 > t + g proves s > t. The host turns every edge into the two float32 bounds (thr32, build_thr32);
//   * an evaluation that lands inside a guard band (~1e-4 of them at the headline) is UNCERTAIN: the wave branches, the
//     lanes concerned fetch both objects in float64 and apply the exact predicate of the parity contract
//     (((dx*dx + dy*dy) + dz*dz) against the host's float64 thresholds). Every pair is therefore decided exactly as
//     k_count_band decides it: results are bit-identical.
// The roles are swapped against k_count_band where one side is binned (MERGED, the cross-correlation counts): the
// lanes hold the BINNED objects (c1), the window streams the unbinned side (c2). A lane then knows the bin, the edge
// row and the counter of each of its objects: hits are counted in registers (add with carry) and go to the LDS
// histogram once per item, not once per evaluation.
//   NE == 2 (one annulus): classes by |s32 - c| against two half widths (certainly inside / possibly inside);
//   NE  > 2: cumulative counters per edge (s <= t_e), fine bin j = cum[j + 1] - cum[j] at the flush.
// ------------------------------------------------------------------------------------------------
// Items -> XCDs (float32 band kernels). Workgroup v runs on XCD v & 7 and takes the items of that XCD one after the other.
// The list arrives in the order of the jobs -- diagonal jobs first (dense lane tiles), then the tiles at patch borders
// (windows that reach a few lanes only) -- so eight contiguous eighths would give six XCDs the heavy items and two the light
// ones. The list is cut into BLOCKS of 2^bs consecutive items (consecutive items are neighbouring lane tiles: their windows
// overlap, which is what an XCD's L2 is for) and the blocks are dealt round robin to the XCDs.
// A list the builder kept in segments (append_items, seg_cap > 0) needs none of this: XCD x takes segment x.
struct TicketMap {
    unsigned long long per_xcd;  // tickets an XCD walks through (multiple of the block size)
    unsigned long long n_kept;   // tickets below this are items (segmented: end of this XCD's segment)
    unsigned long long seg_base; // segmented: first record of this XCD's segment
    unsigned bs;                 // log2 of the block size
    bool segmented;
    __device__ __forceinline__ unsigned long long ticket(unsigned long long v) const {
        const unsigned long long j = v >> 3;
        if (segmented) return seg_base + j;
        return ((((j >> bs) << 3) + (v & 7)) << bs) + (j & ((1ull << bs) - 1ull));
    }
};
__device__ __forceinline__ TicketMap ticket_map(const unsigned long long *__restrict__ counters, unsigned long long seg_cap) {
    TicketMap m;
    m.segmented = seg_cap != 0;
    if (m.segmented) {  // (gridDim.x is a multiple of 8: a workgroup stays with its XCD)
        const int seg = (int)(blockIdx.x % ITEM_SEGS);
        const unsigned long long n_seg = counters[ITEM_SEG_CTR(seg)];
        m.seg_base = (unsigned long long)seg * seg_cap;
        m.per_xcd = n_seg;
        m.n_kept = m.seg_base + n_seg;
        m.bs = 0;
        return m;
    }
    const unsigned long long n_kept = counters[0];
    m.n_kept = n_kept;
    m.seg_base = 0;
    const unsigned long long want = n_kept >> 7;  // ~16 blocks per XCD
    int bs = want > 1 ? 63 - __builtin_clzll(want) : 0;
    bs = bs < 6 ? 6 : (bs > 12 ? 12 : bs);
    m.bs = (unsigned)bs;
    const unsigned long long nblocks = (n_kept + (1ull << bs) - 1ull) >> bs;
    m.per_xcd = ((nblocks + 7ull) >> 3) << bs;
    return m;
}

constexpr float PAD_COORD32 = 4.0f;
constexpr double BAND32_GUARD_SQRT = 2.1e-7;  // coefficient of sqrt(t) in the float32 guard g(t), see k_count_band32
// float32 words per bin of the threshold table: NE == 2: {c, h_in, h_out, 0}; else per edge {t - g, t + g}
__host__ __device__ constexpr int thr32_width(int ne) { return ne == 2 ? 4 : 2 * ne; }
// dynamic LDS of a k_count_band32 workgroup (host and device agree through this one function)
__host__ __device__ inline size_t band32_lds(bool weighted, int cap, int nslots, int thr_rows, int ne) {
    return (size_t)3 * (cap + 4) * 4 + (weighted ? (size_t)(cap + 4) * 8 : 0) + (size_t)nslots * (weighted ? 8 : 4) +
           (size_t)thr_rows * thr32_width(ne) * 4 + 32;
}

// The exact predicate of the parity contract on the float64 columns, for an evaluation the float32 classes left undecided
// (rare: kept out of line so that its addresses and temporaries do not live in the walk loop's registers). The float64
// thresholds the caller will compare with travel in the same round trip as the coordinates: an undecided evaluation stalls
// its wave for ONE memory latency (coordinates, then thresholds one after the other, were two to four; at 51 edges per bin
// one trip in nine of the walk meets an undecided evaluation and the stalls were a third of the kernel's time).
template <int NT>
struct ExactEval {
    double s;        // ((dx*dx + dy*dy) + dz*dz), rounded product by product
    double th[NT];   // tk[0 .. NT)
};
template <int NT>
__device__ __attribute__((noinline)) ExactEval<NT> band32_exact(gf64p lx, gf64p ly, gf64p lz, int64_t li, gf64p sx, gf64p sy, gf64p sz,
                                                               int64_t gi, const double *__restrict__ tk,
                                                               unsigned long long *__restrict__ counters) {
    atomicAdd(counters, 1ull);  // statistics: evaluations decided by the exact predicate (the caller passes one of EVAL_SLOTS
                                // counters: tens of thousands of adds per launch on ONE address cost 0.4 ms at the headline)
    ExactEval<NT> r;
    const double ax = lx[li], ay = ly[li], az = lz[li], bx = sx[gi], by = sy[gi], bz = sz[gi];
#pragma unroll
    for (int e = 0; e < NT; ++e) r.th[e] = tk[e];
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const double sxy = xx + yy;
    r.s = sxy + zz;
    return r;
}

// Stage of k_count_band32 (entries, 12 bytes each + 8 with weights). 320 holds two windows of a typical lane tile (128 objects
// at equal densities: ~142 entries each) -- measured 192 / 288 / 320 / 448 at the headline: 0.367 / 0.355 / 0.350 / 0.360 ms,
// weighted 0.521 / 0.519 / 0.511 / 0.556, RR of config #4 4.65 / 4.44 / 4.41 / 4.89 (the larger the stage, the fewer workgroups
// a CU holds). The big one is for lane tiles whose single window would not fit (denser streamed side, four objects per lane).
constexpr int B32_CAP = 320;
constexpr int B32_CAP_BIG = 512;
// Waves per SIMD the variants of k_count_band32 are compiled for (the second argument of their __launch_bounds__):
constexpr int B32_WAVES_PLAIN = 7; // the plain count, one annulus, one threshold row: 72 VGPRs instead of 79, 0.359 against 0.371 ms at the
                                   // headline (8 spills: 0.405)
constexpr int B32_WAVES_BIG = 6;   // ... with the big stage: its 6.3 KB of LDS admit 25 workgroups per CU anyway, and at 80 registers
                                   // nothing is spilled (headline 0.305 -> 0.286 ms; 8: 0.343)
constexpr int B32_WAVES_W = 5;     // the weighted one-annulus variants (96 VGPRs; the compiler took 97 by itself: 4 waves, 0.57 against 0.51 ms)
constexpr int B32_WAVES_W1 = 5;    // ... with one object per lane (DD / RR of an autocorrelation: 82 VGPRs)
constexpr int B32_WAVES_LT = 1;    // the plain count with per-bin thresholds (physical scales): the compiler's choice (87 registers, 5 waves)
constexpr int band32_min_waves(int R, int CAP, bool WEIGHTED, int NE, bool UNI) {
    if (NE == 2 && UNI) {
        if (WEIGHTED) return R == 1 ? B32_WAVES_W1 : B32_WAVES_W;
        return CAP >= B32_CAP_BIG ? B32_WAVES_BIG : B32_WAVES_PLAIN;
    }
    return NE == 2 && !WEIGHTED ? B32_WAVES_LT : 1;  // everything else: the compiler's choice
}
// The kernel itself: csrc/yawhip_band32.inc, compiled twice -- k_count_band32 stages up to three windows (or pieces of one)
// in a round, k_count_band32_one a single one, for calls whose items all have one window (merged triple runs, items of
// k_build_items): the bookkeeping of two more chunks costs scalar registers (spilled) and instructions per item, 0.283 against
// 0.274 ms at the headline.

#define YAW_B32_NAME k_count_band32
#define YAW_B32_CH 3
#include "yawhip_band32.inc"
#undef YAW_B32_NAME
#undef YAW_B32_CH
#define YAW_B32_NAME k_count_band32_one
#define YAW_B32_CH 1
#include "yawhip_band32.inc"
#undef YAW_B32_NAME
#undef YAW_B32_CH

// ------------------------------------------------------------------------------------------------
// Band kernel for FINE radial grids (separation weights: `resolution` + 1 log-spaced edges per redshift bin,
// reference src/yaw/catalog/trees.py:107-117,358-360). Items, staging, band search and the float32 distance are
// k_count_band32's; what differs is how an evaluation finds its fine bin among ~50:
//   * the edges of a bin are log-spaced, so f = (log2 s32 - log2 t_0) * m puts edge j near f = j: j = round(f), clamped to
//     the table, is the NEAREST edge -- one v_log_f32, one fma, one round instead of a six-step binary search;
//   * the lane reads the float32 bounds {t_j - g, t_j + g} of that edge (g: the guard of k_count_band32) from an LDS table:
//     s32 below the lower bound is in fine bin j - 1, above the upper bound in bin j; the host admits a table only if f is
//     off by less than half a bin everywhere (build_fine32), so the edges on the other side of s32 need no look;
//   * inside the guard band (~1e-3 of the evaluations in range) the exact float64 predicate on the float64 columns decides,
//     against the host's float64 thresholds.
// Hits go to an LDS histogram [bin][fine bin] with one atomic per evaluation (a miss adds to the lane's dummy cell).
// Rows of the float32 table (fine32): {m, a = m log2 t_0, 0, 0}, then {t_j - g, t_j + g} per edge.
// (The first version guessed the bin as floor(f) and was certain only if f kept a distance eps(s32) = e0 + e1 / sqrt(s32)
// from the grid, with a second look at the table otherwise: 32 instruction slots per evaluation against 18 now, and a
// third of the walk's trips took the second look. 2.09 -> 1.25 ms then, -> see DESIGN.md for this one.)
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int fine32_width(int n_edges) { return 4 + 2 * n_edges; }
__host__ __device__ inline size_t band32_fine_lds(bool weighted, int cap, int nslots, int rows, int n_edges) {
    return (size_t)3 * (cap + 4) * 4 + (weighted ? (size_t)(cap + 2) * 8 : 0) + (size_t)nslots * (weighted ? 8 : 4) + 64 * 8 +
           (size_t)rows * fine32_width(n_edges) * 4 + 48;
}

template <int R, int CAP, bool WEIGHTED, bool MERGED, bool UNI>
__global__ __launch_bounds__(64) void k_count_band32_fine(const DevTab *__restrict__ tabs, const Item *__restrict__ items, int n_bins,
                                                          int n_edges, const double *__restrict__ t, const float *__restrict__ fine32,
                                                          const double *__restrict__ rwin_k, const float *__restrict__ ucap,
                                                          unsigned flush_mask, int swap,
                                                          unsigned long long *__restrict__ out_counts,
                                                          double *__restrict__ partials,
                                                          unsigned long long *__restrict__ counters, unsigned long long seg_cap) {
    using HistT = typename std::conditional<WEIGHTED, double, unsigned int>::type;
    constexpr int HB = WEIGHTED ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
    const int nkb = MERGED ? n_bins : 1;
    const int nf = n_edges - 1;
    const int nslots = nkb * nf;
    const int tw = fine32_width(n_edges);
    const int rows = UNI ? 1 : n_bins;
    unsigned char *p = lds_dyn;
    constexpr unsigned COLB = (CAP + 4) * 4;
    float *stage = reinterpret_cast<float *>(p); p += (size_t)3 * COLB;
    double *sw = reinterpret_cast<double *>(p); if (WEIGHTED) p += (size_t)(CAP + 2) * 8;
    HistT *hist = reinterpret_cast<HistT *>(p); p += (size_t)nslots * sizeof(HistT);
    p = reinterpret_cast<unsigned char *>(((size_t)p + 15) & ~(size_t)15);
    double *dummy = reinterpret_cast<double *>(p); p += 64 * 8;  // one cell per lane for misses
    float *stab = reinterpret_cast<float *>(p);                  // [rows][tw]
    const int lane = threadIdx.x;
    const unsigned a_stage = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(stage);
    const unsigned a_sw = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(sw);
    const unsigned a_hist = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(hist);
    const unsigned a_dummy = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(dummy + lane);

    const TicketMap tmap = ticket_map(counters, seg_cap);
    const unsigned long long n_kept = tmap.n_kept;
    for (int e = lane; e < nslots; e += 64) hist[e] = HistT(0);  // every flush leaves the histogram zeroed again
    for (int e = lane; e < rows * tw; e += 64) stab[e] = fine32[e];
    unsigned stage_no = 0;
    for (unsigned long long v = blockIdx.x;; v += gridDim.x) {
        if ((v >> 3) >= tmap.per_xcd) break;
        const unsigned long long ticket = tmap.ticket(v);
        if (ticket >= n_kept) continue;
        const Item it = items[ticket];
        const int o = item_orient(it), islot = item_slot(it);
        const DevTab cl = tabs[swap ? o : 3 + o], cs = tabs[swap ? 3 + o : o];  // lane side, streamed side
        const int kfix = MERGED ? 0 : islot % n_bins;
        const float rwin = (float)(rwin_k[kfix] * 1.000001 + 4e-7);
        int64_t b0 = it.b0[0], nb_total = it.nb[0];

        __syncthreads();
        auto stage_in = [&](int64_t first, int n) {
            const gf32p gx = cs.qx + b0 + first, gy = cs.qy + b0 + first, gz = cs.qz + b0 + first;
#pragma unroll
            for (int c = 0; c < (CAP + 255) / 256; ++c) {
                const unsigned e = (unsigned)(c * 256 + 4 * lane);
                if (e < (unsigned)n) {
                    __builtin_amdgcn_global_load_lds(gx + e, lds_ptr(a_stage + c * 1024), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds(gy + e, lds_ptr(a_stage + COLB + c * 1024), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds(gz + e, lds_ptr(a_stage + 2 * COLB + c * 1024), 16, 0, 0);
                }
            }
            if (WEIGHTED && cs.w) {
#pragma unroll
                for (int c = 0; c < (CAP + 127) / 128; ++c) {
                    const unsigned e = (unsigned)(c * 128 + 2 * lane);
                    if (e < (unsigned)n) __builtin_amdgcn_global_load_lds(cs.w + b0 + first + e, lds_ptr(a_sw + c * 1024), 16, 0, 0);
                }
            }
        };
        stage_in(0, (int)(nb_total < CAP ? nb_total : CAP));
        float ax[R], ay[R], az[R];
        double aw[R];
        int kb[R];
        int n_own = (int)it.na - lane * R;
        n_own = n_own < 0 ? 0 : (n_own > R ? R : n_own);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool have = r < n_own;
            const unsigned ic = have ? (unsigned)(lane * R + r) : 0u;
            ax[r] = have ? (cl.qx + it.a0)[ic] : PAD_COORD32;
            ay[r] = have ? (cl.qy + it.a0)[ic] : PAD_COORD32;
            az[r] = have ? (cl.qz + it.a0)[ic] : PAD_COORD32;
            kb[r] = MERGED ? (have ? (cl.k + it.a0)[ic] : 0) : 0;
            aw[r] = (WEIGHTED && cl.w) ? (have ? (cl.w + it.a0)[ic] : 0.0) : (have ? 1.0 : 0.0);
        }
        float klo, khi;
        {
            const int last_r = n_own > 0 ? n_own - 1 : 0;
            float u_first = cl.axis == 0 ? ax[0] : (cl.axis == 1 ? ay[0] : az[0]), u_last = u_first;
#pragma unroll
            for (int r = 1; r < R; ++r)
                if (r == last_r) u_last = cl.axis == 0 ? ax[r] : (cl.axis == 1 ? ay[r] : az[r]);
            klo = u_first - rwin;
            khi = u_last + rwin;
            const float cap_c = ucap[2 * kfix], cap_s = ucap[2 * kfix + 1];  // band_trim, as in k_count_band32
            if (cap_s > 0.0f) {
                klo = cap_lo32(u_first, cap_c, cap_s);
                khi = cap_hi32(u_last, cap_c, cap_s);
            }
        }
        unsigned int nev = 0;
        auto flush_counts = [&]() {  // LDS histogram -> global result (unweighted)
            __syncthreads();
            for (int idx = lane; idx < nslots; idx += 64) {
                const unsigned int c = (unsigned int)hist[idx];
                hist[idx] = HistT(0);
                if (c) atomicAdd(&out_counts[(int64_t)islot * nslots + idx], (unsigned long long)c);
            }
        };
        // row of every lane object in the float32 table: model parameters in registers, LDS addresses of its edge bounds
        // and of its row of the histogram
        float pm[R], pa[R];
        unsigned a_edges[R], a_rowh[R];
        const float nf_f = (float)nf;
        const unsigned a_stab = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(stab);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int trow = (UNI ? 0 : (MERGED ? kb[r] : kfix)) * tw;
            pm[r] = stab[trow]; pa[r] = stab[trow + 1];
            a_edges[r] = a_stab + (unsigned)(trow + 4) * 4u;
            a_rowh[r] = a_hist + ((unsigned)(kb[r] * nf) << HB);
        }
        f32x2 ax2[R / 2 > 0 ? R / 2 : 1], ay2[R / 2 > 0 ? R / 2 : 1], az2[R / 2 > 0 ? R / 2 : 1];  // packed pairs (R even)
        if constexpr (R >= 2) {
#pragma unroll
            for (int h = 0; h < R / 2; ++h) {
                ax2[h] = f32x2{ax[2 * h], ax[2 * h + 1]}; ay2[h] = f32x2{ay[2 * h], ay[2 * h + 1]}; az2[h] = f32x2{az[2 * h], az[2 * h + 1]};
            }
        }

        for (int win = 0; win < it.nwin; ++win) {
        if (win > 0) {
            b0 = win == 1 ? it.b0[1] : it.b0[2];
            nb_total = win == 1 ? it.nb[1] : it.nb[2];
        }
        for (int64_t st0 = 0; st0 < nb_total; st0 += CAP, ++stage_no) {
            const int n = (int)(nb_total - st0 < CAP ? nb_total - st0 : CAP);
            if (st0 > 0 || win > 0) {
                __syncthreads();
                stage_in(st0, n);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stage has landed (see k_count_band32)
            __syncthreads();
            if (lane == 0) {
                stage[n] = PAD_COORD32; stage[COLB / 4 + n] = PAD_COORD32; stage[2 * (COLB / 4) + n] = PAD_COORD32;
                if (WEIGHTED) sw[n] = 0.0;
            }
            if (WEIGHTED && !cs.w)
                for (int e = lane; e < n; e += 64) sw[e] = 1.0;
            __syncthreads();
            const unsigned a_key = a_stage + COLB * (unsigned)cl.axis;
            const unsigned a_sent = a_key + ((unsigned)n << 2);
            unsigned ql = a_key - 4u, qh = ql;
            for (unsigned step = 4u << (31 - __builtin_clz(n)); step >= 4u; step >>= 1) {
                const unsigned pl = ql + step, ph = qh + step;
                const float kl = *(const __attribute__((address_space(3))) float *)(size_t)(pl < a_sent ? pl : a_sent);
                const float kh = *(const __attribute__((address_space(3))) float *)(size_t)(ph < a_sent ? ph : a_sent);
                ql = kl < klo ? pl : ql;
                qh = kh <= khi ? ph : qh;
            }
            int lo = (int)((ql + 4u - a_key) >> 2), hi = (int)((qh + 4u - a_key) >> 2);
            if (n_own == 0) lo = hi = n;
            const int len = hi - lo;
            nev += (unsigned int)(len * n_own);
            const int steps = wave_max_nonneg(len);

            unsigned cur = a_stage + ((unsigned)lo << 2);
            const unsigned last = a_stage + ((unsigned)n << 2);
            // The walk is a chain of LDS round trips (entry -> nearest edge -> its bounds -> histogram): the next entry is
            // fetched while this one is classified, and the edge bounds of all lane objects are fetched together.
            struct Entry { float x, y, z; double w; unsigned at; };
            auto fetch = [&](unsigned at) {
                Entry e;
                e.at = at < last ? at : last;
                e.x = *(const __attribute__((address_space(3))) float *)(size_t)e.at;
                e.y = *(const __attribute__((address_space(3))) float *)(size_t)(e.at + COLB);
                e.z = *(const __attribute__((address_space(3))) float *)(size_t)(e.at + 2 * COLB);
                e.w = WEIGHTED ? lds_f64(((e.at - a_stage) << 1) + a_sw) : 1.0;
                return e;
            };
            unsigned pend[R];  // cells of the previous entry's hits (unweighted)
#pragma unroll
            for (int r = 0; r < R; ++r) pend[r] = a_dummy;
            Entry nxt = fetch(cur);
            // (consumed here, so that the compiler's wait-count bookkeeping enters the loop with nothing of the prologue pending:
            // a wait at the loop header has to satisfy every incoming edge, and "the reads just issued" of the prologue would
            // turn it into a full drain -- of the previous trip's histogram updates, every trip)
            if constexpr (WEIGHTED) asm volatile("" :: "v"(nxt.x), "v"(nxt.y), "v"(nxt.z), "v"(nxt.w));
            else asm volatile("" :: "v"(nxt.x), "v"(nxt.y), "v"(nxt.z));
            for (int s = 0; s < steps; ++s) {
                const Entry en = nxt;
                cur += 4;
                nxt = fetch(cur);  // (past the longest band: an entry beyond every band, or the sentinel -- never used)
                const unsigned a16 = en.at;
                const float ex = en.x, ey = en.y, ez = en.z;
                const double ew = en.w;
                float s32[R];
                if constexpr (R >= 2) {
#pragma unroll
                    for (int h = 0; h < R / 2; ++h) {
                        const f32x2 dx = ax2[h] - ex, dy = ay2[h] - ey, dz = az2[h] - ez;
                        const f32x2 sq = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
                        s32[2 * h] = sq.x; s32[2 * h + 1] = sq.y;
                    }
                } else {
                    const float dx = ax[0] - ex, dy = ay[0] - ey, dz = az[0] - ez;
                    s32[0] = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                }
                int jj[R];
                bool unc[R];
                unsigned long long any_unc_mask = 0ull;
                f32x2 tb[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // nearest edge of the object's grid (s32 = 0: f = -inf -> edge 0) and its float32 bounds
                    const float fr = __builtin_rintf(__builtin_fmaf(__builtin_amdgcn_logf(s32[r]), pm[r], -pa[r]));
                    jj[r] = (int)__builtin_amdgcn_fmed3f(fr, 0.0f, nf_f);
                    tb[r] = *(const __attribute__((address_space(3))) f32x2 *)(size_t)(a_edges[r] + ((unsigned)jj[r] << 3));
                }
                if constexpr (!WEIGHTED) {
                    // the histogram updates of the PREVIOUS entry go out behind this entry's reads: by the time the loop comes
                    // round to anything that waits for the LDS, they have long been absorbed
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)pend[r], 1u,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int j = jj[r];
                    // the side of the edge s32 lies on; "inside the guard band of edge j" = neither below nor above (spelled
                    // !below && !(s32 > hi) the compiler issues a third compare for the negation)
                    const bool below = s32[r] < tb[r].x, above = s32[r] > tb[r].y;
                    const int bin = j - (below ? 1 : 0);
                    unc[r] = !(below | above);
                    any_unc_mask |= ~(__builtin_amdgcn_ballot_w64(below) | __builtin_amdgcn_ballot_w64(above));  // scalar unit only
                    const bool hit = ((unsigned)bin < (unsigned)nf) & !unc[r];
                    const unsigned cell = a_rowh[r] + ((unsigned)bin << HB);
                    if constexpr (WEIGHTED) {
                        if (hit)
                            (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(size_t)cell, aw[r] * ew,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        pend[r] = hit ? cell : a_dummy;  // a miss adds to the lane's dummy cell
                    }
                }
                if (any_unc_mask != 0ull) {
                    // the exact float64 predicate on the float64 columns decides, against the host's float64 thresholds (rare)
                    const unsigned eidx = (a16 - a_stage) >> 2;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (unc[r] && eidx < (unsigned)n && r < n_own) {
                            const int j = jj[r];
                            // (the admission rule of build_fine32 leaves edge j as the only one s can be confused with)
                            const ExactEval<1> ev = band32_exact<1>(cl.x, cl.y, cl.z, it.a0 + lane * R + r, cs.x, cs.y, cs.z,
                                                                    cs.idx ? (int64_t)cs.idx[b0 + st0 + eidx] : b0 + st0 + (int64_t)eidx,
                                                                    t + (size_t)(MERGED ? kb[r] : kfix) * n_edges + j,
                                                                    counters + 9 + 8 * (ticket & (EVAL_SLOTS - 1)));
                            const int bin = ev.s <= ev.th[0] ? j - 1 : j;  // t[bin] < s <= t[bin + 1]
                            if ((unsigned)bin < (unsigned)nf) {
                                const unsigned cell = a_rowh[r] + ((unsigned)bin << HB);
                                if constexpr (WEIGHTED)
                                    (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(size_t)cell, aw[r] * ew,
                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                else
                                    (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)cell, 1u,
                                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                    }
                }
            }
            if constexpr (!WEIGHTED) {  // the last entry's updates
#pragma unroll
                for (int r = 0; r < R; ++r)
                    (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)pend[r], 1u,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (!WEIGHTED && (stage_no & flush_mask) == flush_mask) flush_counts();
        }
        }
        if constexpr (WEIGHTED) {
            __syncthreads();
            for (int idx = lane; idx < nslots; idx += 64) {
                partials[(int64_t)it.pot * nslots + idx] = (double)hist[idx];
                hist[idx] = HistT(0);
            }
        } else {
            flush_counts();
        }
        nev = wave_sum_lane63(nev);  // (DPP: the shuffle form is six trips through the LDS crossbar, per item, for a statistic)
        if (lane == 63 && nev) atomicAdd(&counters[8 + 8 * (ticket & (EVAL_SLOTS - 1))], (unsigned long long)nev);
    }
}

// Evaluated pairs per job (na * nb of the job's kept items): the cost the host balances over GPUs.
__global__ void k_item_work(const Item *__restrict__ items, const unsigned long long *__restrict__ counters,
                            int slots_per_job, unsigned long long *__restrict__ job_work) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= counters[0]) return;
    const Item it = items[i];
    unsigned long long streamed = 0;
    for (int w = 0; w < it.nwin; ++w) streamed += (unsigned long long)it.nb[w];
    atomicAdd(&job_work[item_slot(it) / slots_per_job], (unsigned long long)it.na * streamed);
}

// Weighted sums: every kept item left a slab of `slab` float64 values at partials[pot]. They are added per output
// slot in a fixed two-level order -- chunks of REDUCE_CHUNK consecutive potential items, then the chunks of a slot in
// order -- so the result is bit-reproducible and the reduction is parallel over (chunk, value). Dropped potential
// items (kept[pot] == 0, their slab is never written) are skipped; kept == nullptr means every item was kept.
constexpr int REDUCE_CHUNK = 32;
__global__ void k_reduce_chunks(const double *__restrict__ partials, const unsigned char *__restrict__ kept,
                                const int64_t *__restrict__ prefix, const int64_t *__restrict__ cprefix, int n_slots,
                                int slab, double *__restrict__ chunk_sums, unsigned long long *__restrict__ counters) {
    stamp_start(counters, CTR_T_COUNTED);  // the first kernel behind the count kernels
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = idx / slab;
    if (g >= cprefix[n_slots]) return;
    const int e = (int)(idx - g * slab);
    int lo = 0, hi = n_slots;  // slot = largest s with cprefix[s] <= g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cprefix[mid] <= g) lo = mid; else hi = mid;
    }
    const int64_t p0 = prefix[lo] + (g - cprefix[lo]) * REDUCE_CHUNK;
    const int64_t p1 = p0 + REDUCE_CHUNK < prefix[lo + 1] ? p0 + REDUCE_CHUNK : prefix[lo + 1];
    double acc = 0.0;
    for (int64_t pot = p0; pot < p1; ++pot)
        if (!kept || kept[pot]) acc += partials[pot * slab + e];
    chunk_sums[idx] = acc;
}

__global__ void k_reduce_slots(const double *__restrict__ chunk_sums, const int64_t *__restrict__ cprefix, int n_slots,
                               int slab, double *__restrict__ out, unsigned long long *__restrict__ stamp) {
    if (stamp) stamp_start(stamp, CTR_T_COUNTED);  // (no chunks: this is the first kernel behind the count kernels)
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n_slots * slab) return;
    const int slot = (int)(idx / slab), e = (int)(idx - (int64_t)slot * slab);
    double acc = 0.0;
    for (int64_t g = cprefix[slot]; g < cprefix[slot + 1]; ++g) acc += chunk_sums[g * slab + e];
    out[idx] = acc;
}

__global__ void k_counts_to_double(const unsigned long long *__restrict__ in, double *__restrict__ out, int64_t n,
                                   unsigned long long *__restrict__ counters) {
    stamp_start(counters, CTR_T_COUNTED);  // the first kernel behind the count kernel
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

// The last kernel of a count call: the first n_copy 16-byte units of the slot's result block [counters][counts][sums] go to
// its pinned image, and the first n_clean of them are zeroed behind the read, so that the next call of the slot finds
// counters and counts at zero without a fill (sums are always fully written and are not cleaned). Plain loads: the kernel
// boundary has made the count kernel's atomics visible. The words of the call's own bookkeeping are not copied: the ticket
// (device only), the completion word (host only) and the two stamps this kernel supplies.
// Completion: every thread fences its stores to the host, every workgroup then draws a ticket, and the one that draws the
// last writes the call's sequence number into the pinned block with a system-scope release -- the host polls that word
// (count_finish). The ticket word wraps to zero with the last draw. No workgroup waits for another.
constexpr int TAIL_WG = 256;
constexpr unsigned TAIL_MAX_GRID = 64;
__global__ __launch_bounds__(TAIL_WG) void k_call_tail(uint4 *__restrict__ dev, uint4 *__restrict__ host, unsigned n_copy,
                                                      unsigned n_clean, unsigned long long seq) {
    const unsigned long long t0 = wall_clock64();
    static_assert(CTR_T_COUNTED == 2 && CTR_T_TAIL == 3 && CTR_TICKET == 4 && CTR_DONE == 6, "units 1, 2 and 3 of the block");
    for (unsigned u = blockIdx.x * TAIL_WG + threadIdx.x; u < n_copy; u += gridDim.x * TAIL_WG) {
        if (u == CTR_TICKET / 2 || u == CTR_DONE / 2) continue;
        uint4 v = dev[u];
        if (u == CTR_T_COUNTED / 2) {  // (a thread of the first workgroup)
            if ((v.x | v.y) == 0u) { v.x = (unsigned)t0; v.y = (unsigned)(t0 >> 32); }  // no kernel behind the count kernel
            v.z = (unsigned)t0; v.w = (unsigned)(t0 >> 32);
        }
        host[u] = v;
        if (u < n_clean) dev[u] = make_uint4(0u, 0u, 0u, 0u);
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned *ticket = reinterpret_cast<unsigned *>(dev) + 2 * CTR_TICKET;
        if (atomicInc(ticket, gridDim.x - 1) == gridDim.x - 1) {
            __threadfence_system();
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(host) + CTR_DONE, seq, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

inline DevTab make_tab(const double *x, const double *y, const double *z, const double *w, const int32_t *k, const int64_t *off,
                       const int64_t *vbase, const int64_t *slo, const int64_t *tiles, const TileRec *tile_rec, const RunGrid *grid,
                       int axis, const float *q = nullptr, int64_t q_stride = 0, const int32_t *idx = nullptr) {
    return DevTab{(gf64p)x, (gf64p)y, (gf64p)z, (gf64p)w, (gi32p)k, (gi64p)off, (gi64p)vbase, (gi64p)slo, (gi64p)tiles,
                  tile_rec, grid, (gf32p)q, (gf32p)(q ? q + q_stride : nullptr), (gf32p)(q ? q + 2 * q_stride : nullptr), (gi32p)idx,
                  (gi32p)nullptr, axis, 0};
}

// One launch of a count kernel: its dynamic-LDS limit raised first where it needs more than 64 KiB.
template <typename... Params, typename... Args>
hipError_t launch(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args &...args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// Kernel variant dispatch: f(T{}) for the T among Ts whose ::value equals v. The variants named at the call sites are the
// ones compiled, and make_plan plans only those: a value that names none is an error, not a fall-back.
template <typename... Ts, typename V, typename F>
hipError_t pick(const V &v, F &&f) {
    hipError_t e = hipErrorInvalidValue;
    (void)(((v == Ts::value) && (e = f(Ts{}), true)) || ...);
    return e;
}
template <bool B> using Bool = std::integral_constant<bool, B>;
template <int I> using Int = std::integral_constant<int, I>;
// (objects per lane, entries per LDS stage) of a band kernel
template <int R_, int CAP_> struct Stage {
    static constexpr int R = R_, CAP = CAP_;
    static constexpr std::pair<int, int> value{R_, CAP_};
};
// (MERGED, UNI) of a band kernel: one item for all bins; one threshold row for all of an item's bins
template <bool MERGED_, bool UNI_> struct Rows {
    static constexpr bool MERGED = MERGED_, UNI = UNI_;
    static constexpr std::pair<bool, bool> value{MERGED_, UNI_};
};

inline int64_t seg_len(const yawhip_catalog *c, int patch, int k) {
    const int kk = c->nb == 1 ? 0 : k;
    const int64_t i = (int64_t)patch * c->nb + kk;
    return c->h_off[i + 1] - c->h_off[i];
}

// yawhip_stats.count_variant*: the family and template arguments of a count kernel (code layout: include/yawhip.h)
enum VariantFamily : int32_t { VF_COUNT = 1, VF_MERGED, VF_MERGED_OCC8, VF_BAND, VF_BAND32, VF_BAND32_ONE, VF_BAND32_FINE };
constexpr int32_t variant_code(int32_t family, int R, int cap, bool weighted, int ne = 0, bool merged = false, bool uni = false,
                               bool priv = false, bool filter = false, bool nf1 = false) {
    return family | R << 4 | cap << 8 | (int32_t)weighted << 18 | ne << 19 | (int32_t)merged << 22 | (int32_t)uni << 23 |
           (int32_t)priv << 24 | (int32_t)filter << 25 | (int32_t)nf1 << 26;
}
// the variant of a call from those of its pieces: pieces that launched none do not count, different ones make it mixed
int32_t merge_variant(int32_t a, int32_t b) { return a == 0 || a == b ? b : (b == 0 ? a : YAWHIP_VARIANT_MIXED); }

// Float32 bounds of every edge for k_count_band32 (see there): for unit vectors rounded to float32,
//   |s32 - s| <= g(t) = 2.1e-7 sqrt(t) + 5e-7 t + 1e-12 near s = t,
// so s32 < t - g proves s <= t and s32 > t + g proves s > t; in between the kernel evaluates in float64.
//   n_edges == 2: {c, h_in, h_out, 0}: |s32 - c| < h_in proves t0 < s <= t1, |s32 - c| >= h_out proves the opposite
//                 (s32 - c is what the kernel's three fused multiply-adds deliver; both widths carry their rounding);
//   else per edge {t - g rounded down, t + g rounded up}.
std::vector<float> build_thr32(const double *t, int n_bins, int n_edges) {
    auto down = [](double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; };
    auto up = [](double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; };
    auto guard = [](double te) { return BAND32_GUARD_SQRT * std::sqrt(te) + 5e-7 * te + 1e-12; };
    const int tw = thr32_width(n_edges);
    std::vector<float> out((size_t)n_bins * tw, 0.f);
    for (int k = 0; k < n_bins; ++k) {
        const double *tk = t + (size_t)k * n_edges;
        float *row = &out[(size_t)k * tw];
        if (n_edges == 2) {
            const double g0 = guard(tk[0]), g1 = guard(tk[1]);
            const float c = (float)(0.5 * (tk[0] + tk[1]));
            const double cd = (double)c;
            // q = fma(dz, dz, fma(dy, dy, fma(dx, dx, -c))): three roundings of intermediate sums that stay below 2 c wherever
            // a class is claimed (|q| < h_in <= c, or s inside the annulus: s32 <= t1 + g1 <= 2 c) -> 6 x 2^-24 x c = 3.6e-7 c
            const double fold = 4e-7 * cd;
            const double h_in = (std::min(cd - (tk[0] + g0), (tk[1] - g1) - cd) - fold) * (1.0 - 1e-6);
            const double h_out = (std::max(cd - (tk[0] - g0), (tk[1] + g1) - cd) + fold) * (1.0 + 1e-6);
            row[0] = c;
            row[1] = h_in > 0.0 ? down(h_in) : 0.f;   // |q| < 0 never holds: nothing is certain
            row[2] = up(std::max(h_out, 0.0));
            row[3] = 0.f;
        } else {
            for (int e = 0; e < n_edges; ++e) {
                const double g = guard(tk[e]);
                row[2 * e] = down(tk[e] - g);
                row[2 * e + 1] = up(tk[e] + g);
            }
        }
    }
    return out;
}

// Float32 table of k_count_band32_fine (see there), one row per redshift bin: {m, a, e0, e1}, then {t_j - g, t_j + g} per edge.
// Empty when the edges of some bin do not follow the log-spaced model closely enough for float32 (the caller then counts
// with the float64 band kernel): deviation above 0.05 fine bins, a guard wider than a fifth of a fine bin, t_0 = 0.
std::vector<float> build_fine32(const double *t, int n_bins, int n_edges) {
    auto down = [](double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; };
    auto up = [](double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; };
    auto guard = [](double te) { return BAND32_GUARD_SQRT * std::sqrt(te) + 5e-7 * te + 1e-12; };
    const int tw = fine32_width(n_edges), nf = n_edges - 1;
    std::vector<float> out((size_t)n_bins * tw, 0.f);
    for (int k = 0; k < n_bins; ++k) {
        const double *tk = t + (size_t)k * n_edges;
        if (!(tk[0] > 1e-12) || !(tk[nf] > tk[0])) return {};
        const double l0 = std::log2(tk[0]), l1 = std::log2(tk[nf]);
        const double m = (double)nf / (l1 - l0), a = l0 * m;
        double dev = 0.0;
        for (int j = 0; j <= nf; ++j) {
            if (j > 0 && !(tk[j] > tk[j - 1])) return {};
            dev = std::max(dev, std::fabs((std::log2(tk[j]) - l0) * m - (double)j));
        }
        // error of the device's f: hardware log2 (1 ulp of a result below 64), float32 images of m and a, the fma
        const double dev_f = m * (1e-5 + 6e-8 * 64.0) + 2.0 * 6e-8 * std::fabs(a) + 4e-5 + 6e-8 * (nf + 2);
        const double per_s = 1.05 * m / std::log(2.0);  // d f / (d s / s), with room for the second order
        // Admission: an s32 between the guard bands of edges j and j + 1 must round to one of the two, i.e. f may be off by
        // less than half a bin: the model's deviation at the edges, the device's arithmetic, and the guard (widest,
        // relative to t, at the first edge).
        if (dev + dev_f + per_s * guard(tk[0]) / tk[0] > 0.45) return {};
        float *row = &out[(size_t)k * tw];
        row[0] = (float)m; row[1] = (float)a; row[2] = 0.f; row[3] = 0.f;
        for (int j = 0; j <= nf; ++j) {
            const double g = guard(tk[j]);
            row[4 + 2 * j] = down(tk[j] - g);
            row[5 + 2 * j] = up(tk[j] + g);
        }
    }
    return out;
}

}  // namespace

namespace yawhip_detail {  // what the other units call (declared in yawhip_internal.h)

CallKey::CallKey(const yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs_, const int32_t *jobs_,
                 int32_t n_bins_, int32_t n_edges_, const double *t_, int32_t kernel_, bool want_counts_, bool want_sums_,
                 bool for_work_, int32_t n_dev_)
    : c1_uid(c1->uid), c2_uid(c2->uid), opt_gen(ctx->opt_gen), n_jobs(n_jobs_), n_bins(n_bins_), n_edges(n_edges_),
      kernel(kernel_), n_dev(n_dev_), want_counts(want_counts_), want_sums(want_sums_), for_work(for_work_), jobs(jobs_), t(t_) {
    // word by word: a job is one 64-bit word, a threshold another
    auto mix = [this](uint64_t w) { hash = (hash ^ w) * 0x100000001b3ull; hash ^= hash >> 29; };
    for (uint64_t w : {c1_uid, c2_uid, opt_gen, (uint64_t)(uint32_t)n_jobs << 32 | (uint32_t)n_bins,
                       (uint64_t)(uint32_t)n_edges << 32 | (uint32_t)kernel,
                       (uint64_t)(uint32_t)n_dev << 32 | (uint64_t)(want_counts | want_sums << 1 | for_work << 2)})
        mix(w);
    for (size_t j = 0; j < (size_t)n_jobs; ++j) {
        uint64_t w;
        memcpy(&w, jobs + 2 * j, sizeof w);
        mix(w);
    }
    for (size_t i = 0; i < (size_t)n_bins * n_edges; ++i) {
        uint64_t w;
        memcpy(&w, t + i, sizeof w);
        mix(w);
    }
}

// What a count call derives from its inputs on the HOST before anything is launched -- kernel choice, layouts, tile and stage
// sizes, the job records / prefix / threshold tables of the item builder and the count kernel (uploaded once, into the plan's
// own device buffer) -- kept for the next call with the same inputs (CallKey). A repeated call (the next step of a bench, the
// same count of the next measurement, DR after DD with the same job list is ANOTHER plan) then marshals no tables at all; the
// item builder and the count kernels run every call. Plans die with their catalogues and options.
struct HostPlan {
    CallKey key;
    uint64_t stamp = 0;
    // decisions
    bool empty = false;   // nothing to count (no output values)
    bool split = false;   // the job list has to be counted in pieces (SPLIT_JOBS)
    int grid_div = 8;  // band kernels: workgroups = potential items / this
    int R = 0, band_ne = 0, cap = 0, hp_shift = 0, lean_bins = 0, mode = 0, reach = 0, kernel = 0, nf = 0, n_orient = 0;
    bool band = false, band32 = false, band_fine = false, filter = false, lean = false, merged = false, run_unweighted = false,
         run_weighted = false, strip_items = false, swap = false, sweep = false, triple = false, uni = false, uniform_t = false,
         weighted = false;
    int64_t abytes = 0, cand = 0, n_items = 0, n_out = 0, n_pslots = 0, n_sjobs = 0, n_slots = 0, slab = 0, tile = 0;
    double rwin_max = 0.0;
    double cap_c = 1.0, cap_s = 0.0;  // cos / sin of sep_angle(rwin_max): the strip builder's trimmed windows (cap_s = 0: untrimmed)
    size_t lds_band = 0, lds_merged = 0;
    // device tables, in one allocation (d_in) made when the plan's table image is uploaded (Planner::tables): jobs / job records,
    // prefix, thresholds, pre-filter thresholds, window widths, float32 classes, layout table, and -- weighted calls -- the chunk
    // prefix of the slab reduction
    DevPtr<unsigned char> d_in;
    int32_t *d_jobs = nullptr;
    int64_t *d_prefix = nullptr, *d_cprefix = nullptr;
    double *d_t = nullptr, *d_rwin = nullptr;
    float *d_dthr = nullptr, *d_ucap = nullptr, *d_thr32 = nullptr;
    DevTab *d_tabs = nullptr;
    int64_t n_chunks = 0;
};

// Forget the plans that involve catalogue `c` (nullptr: all of them).
void drop_plans(yawhip_ctx *ctx, const yawhip_catalog *c) {
    for (size_t i = 0; i < ctx->plans.size();) {
        if (!c || ctx->plans[i]->key.c1_uid == c->uid || ctx->plans[i]->key.c2_uid == c->uid) {
            delete ctx->plans[i];
            ctx->plans[i] = ctx->plans.back();
            ctx->plans.pop_back();
        } else ++i;
    }
}

// The argument checks of a count call, made by every entry point before any device work: handles, sizes, bin counts of the
// catalogues, thresholds and the patch ids of the jobs.
int check_call(const yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs, const int32_t *jobs,
               int32_t n_bins, int32_t n_edges, const double *t) {
    if (!ctx || !c1 || !c2) return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs: NULL handle");
    if (n_jobs < 0 || n_bins <= 0 || n_edges < 2 || n_edges > MAX_EDGES || !t || (n_jobs > 0 && !jobs))
        return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs: bad sizes (n_jobs=%d n_bins=%d n_edges=%d, max edges %d)",
                    n_jobs, n_bins, n_edges, MAX_EDGES);
    if (c1->ctx != ctx || c2->ctx != ctx) return fail(YAWHIP_ERR_MISMATCH, "catalogues belong to another context");
    if (c1->n_patches != c2->n_patches)
        return fail(YAWHIP_ERR_MISMATCH, "patch counts differ (%d vs %d)", c1->n_patches, c2->n_patches);
    if ((c1->nb != 1 && c1->nb != n_bins) || (c2->nb != 1 && c2->nb != n_bins))
        return fail(YAWHIP_ERR_MISMATCH, "catalogue bin counts (%d, %d) do not fit n_bins=%d", c1->nb, c2->nb, n_bins);
    for (int k = 0; k < n_bins; ++k)
        for (int e = 0; e < n_edges; ++e) {
            const double v = t[(size_t)k * n_edges + e];
            if (!(v >= 0.0) || (e > 0 && !(v >= t[(size_t)k * n_edges + e - 1])))
                return fail(YAWHIP_ERR_INVALID, "thresholds of bin %d are not ascending non-negative numbers", k);
        }
    for (int j = 0; j < n_jobs; ++j)
        if (jobs[2 * j] < 0 || jobs[2 * j] >= c1->n_patches || jobs[2 * j + 1] < 0 || jobs[2 * j + 1] >= c1->n_patches)
            return fail(YAWHIP_ERR_INVALID, "job %d has a patch id outside [0,%d)", j, c1->n_patches);
    return YAWHIP_OK;
}

// The band_cap option (yawhip_ctx_set_option): 0, or a stage capacity the band kernels are compiled for.
int check_band_cap(int64_t value) {
    if (value != 0 && value != BCAP && value != BCAP_MID && value != B32_CAP && value != B32_CAP_BIG)
        return fail(YAWHIP_ERR_INVALID, "band_cap must be 0 (auto), 192 or 288 (float64 / fine-grid band kernels), %d or %d (float32 band kernel)",
                    B32_CAP, B32_CAP_BIG);
    return YAWHIP_OK;
}

}  // namespace yawhip_detail

namespace {

// make_plan in steps, run in this order: each one fills its own fields of the plan; what a later step needs and the plan does
// not keep stays in the planner.
struct Planner {
    yawhip_ctx *ctx;
    const yawhip_catalog *c1, *c2;
    int32_t n_jobs;
    const int32_t *jobs;
    int32_t n_bins, n_edges;
    const double *t;
    bool for_work;
    HostPlan &P;
    bool unit = false, auto_pick = false, half_ok = false;
    int tile_idx = 0;  // tile table of the layouts (R = 1, 2, 4)
    double layout_sep = 0.0;
    std::vector<double> rwin;     // window half width per bin
    std::vector<int32_t> orient;  // sort axis of the strip layouts of every job
    const StripLayout *L1[3] = {nullptr, nullptr, nullptr}, *L2[3] = {nullptr, nullptr, nullptr};
    const yawhip_catalog *c_lane = nullptr, *c_strm = nullptr;
    const StripLayout *const *LL = nullptr, *const *LS = nullptr;  // lane side, streamed side
    std::vector<float> fine32;
    std::vector<int64_t> prefix;
    std::vector<JobRec> job_recs;  // strip path, per job: what the builder needs of the two groups (JobRec)
    void sides(bool swap) {
        c_lane = swap ? c1 : c2; c_strm = swap ? c2 : c1;
        LL = swap ? L1 : L2; LS = swap ? L2 : L1;
    }
    int kernel_and_sizes(int32_t kernel, bool want_counts, bool want_sums);
    int layouts();
    int tile_and_stage();
    int histogram();
    int items();
    int tables();
};

// Step 1: the kernel, and the sizes of the output.
int Planner::kernel_and_sizes(int32_t kernel, bool want_counts, bool want_sums) {
    if (kernel == YAWHIP_KERNEL_AUTO) kernel = ctx->default_kernel;
    auto_pick = kernel == YAWHIP_KERNEL_AUTO;  // BAND or SWEEP, whichever suits the layouts (decided below)
    if (kernel == YAWHIP_KERNEL_AUTO) kernel = YAWHIP_KERNEL_BAND;
    if (kernel < YAWHIP_KERNEL_EXACT || kernel > YAWHIP_KERNEL_BAND)
        return fail(YAWHIP_ERR_INVALID, "unknown kernel id %d", kernel);
    // the FP32 pre-filter assumes unit vectors; anything else is evaluated pair by pair in FP64
    unit = c1->unit_norm && c2->unit_norm;
    if (kernel == YAWHIP_KERNEL_FILTER && !unit) kernel = YAWHIP_KERNEL_EXACT;
    // the window search compares the sorted coordinate of both sides: the axes must agree
    if ((kernel == YAWHIP_KERNEL_SWEEP || kernel == YAWHIP_KERNEL_BAND) && c1->axis != c2->axis)
        kernel = unit ? YAWHIP_KERNEL_FILTER : YAWHIP_KERNEL_EXACT;
    // the band kernels park finished lanes on a sentinel at coordinate 4.0 and bound their searches by it: unit vectors only
    if (kernel == YAWHIP_KERNEL_BAND && !unit) kernel = YAWHIP_KERNEL_EXACT;
    P.kernel = kernel;
    P.band = kernel == YAWHIP_KERNEL_BAND;
    P.sweep = kernel == YAWHIP_KERNEL_SWEEP || P.band;
    P.filter = unit && kernel != YAWHIP_KERNEL_EXACT;

    P.nf = n_edges - 1;
    P.n_slots = (int64_t)n_jobs * n_bins;
    P.n_out = P.n_slots * P.nf;
    P.weighted = (c1->w != nullptr) || (c2->w != nullptr);
    P.run_weighted = P.weighted && want_sums;
    P.run_unweighted = want_counts || (!P.weighted && want_sums);
    if (P.n_out == 0) { P.empty = true; return YAWHIP_OK; }
    if (P.n_slots > (1ll << 30)) return fail(YAWHIP_ERR_INVALID, "too many (job,bin) slots");
    HIP_TRY(hipSetDevice(ctx->device));

    // tile size: objects per lane. Larger tiles amortise the streamed-object read; small segments
    // prefer small tiles so that padded lanes do not dominate.
    // Lean path (k_count_merged): z-window culling + FP32 pre-filter + queued exact evaluation. Its merged
    // form (one item for all bins, strip layouts on both sides) serves c1 binned x c2 unbinned, i.e. every
    // count of a cross-correlation.
    P.lean = P.sweep && (P.filter || P.band);  // single-wave workgroups on windowed items (k_count_merged / k_count_band)
    return YAWHIP_OK;
}

// Step 2: layout mode, orientations and strip layouts, the float32 band kernels, the sides, BAND or SWEEP.
int Planner::layouts() {
    const int nf = P.nf;
    rwin.resize((size_t)n_bins);
    double rwin_max = 0.0;  // widest window half width over the bins
    for (int k = 0; k < n_bins; ++k) {
        rwin[(size_t)k] = std::sqrt(t[(size_t)k * n_edges + n_edges - 1]) * (1.0 + 1e-12) + 1e-15;
        rwin_max = std::max(rwin_max, rwin[(size_t)k]);
    }
    P.rwin_max = rwin_max;
    // strip pairing pays while a run has few partner runs; for separations far beyond the grid spacing the
    // ordinary (patch, bin) layout is used instead
    // (grid_sep: the largest separation in the grid's own unit -- chord for a grid linear in v, angle for one in latitude)
    const double grid_sep = c1->strip_grid ? sep_angle(rwin_max) : rwin_max;
    const bool strips = P.lean && c1->has_strips && c2->has_strips && c1->strip_width == c2->strip_width &&
                        c1->strip_grid == c2->strip_grid &&
                        (c1->strip_width <= 0.0 || grid_sep / c1->strip_width <= (double)MAX_STRIP_REACH);
    // mode 3: binned x binned on the per-segment strip layouts: ordinary (job, bin) items whose lane tiles and windows
    // come from (patch, bin, strip) runs -- it pays when the lane side is dense: runs of at least a few lane tiles per
    // (patch, bin, strip); estimated from the patch-level layout the upload built (B times as many runs)
    bool seg_ok = false;
    if (strips && c1->nb == n_bins && c2->nb == n_bins && n_bins > 1 && ctx->seg_strips) {
        const StripLayout &base2 = c2->strips[c2->axis];
        const int64_t seg_runs = base2.h_vbase[(size_t)base2.n_groups] * (int64_t)c2->nb;
        seg_ok = c2->n / std::max<int64_t>(seg_runs, 1) >= ctx->seg_min_run;
    }
    bool uniform_t = true;  // every bin has the same threshold row (angular scales)
    for (int k = 1; k < n_bins && uniform_t; ++k)
        uniform_t = memcmp(t, t + (size_t)k * n_edges, sizeof(double) * n_edges) == 0;
    P.uniform_t = uniform_t;
    // One item for all bins needs a histogram of B x (E - 1) cells (and B edge rows when they differ) in LDS. Where that
    // does not fit (hundreds of bins times dozens of separation-weight bins), the count falls back to ordinary
    // (job, bin) items, whose histogram has E - 1 cells.
    const size_t merged_lds = (size_t)n_bins * nf * (P.weighted ? 8 : 4) + (size_t)(uniform_t ? 1 : n_bins) * n_edges * sizeof(double) +
                              (size_t)n_bins * sizeof(float) + BandLds<BCAP_MID>::FIXED + (BCAP_MID + 2) * 8 + 2 * MSTAGE * sizeof(ObjF) + 1024;
    const bool merged_fits = merged_lds <= (size_t)ctx->lds_limit;
    const int mode = P.mode = !strips ? 0 : (c1->nb > 1 && c2->nb == 1) ? (merged_fits ? 1 : 0) : (seg_ok ? 3 : 0);
    // per-segment strip layouts keep the grid linear in v (build_strip_layout): their short runs make items of fixed cost, and
    // the latitude grid's narrower strips away from v = 0 only add items there
    layout_sep = mode == 3 ? rwin_max : grid_sep;
    const bool merged = P.merged = mode == 1;                // one item covers all bins, output slot = job
    const bool strip_items = P.strip_items = mode != 0;      // items come from strip runs (k_build_items_strips)
    // Orientation of every job: the (u, v) projection that compresses the sphere least around its two patches, i.e.
    // the one that drops the coordinate w in which the patches lie farthest from the origin. (Projected along an
    // axis the patches are nearly perpendicular to, objects pile up in (u, v) -- density grows like 1 / |w| -- and
    // the opposite hemisphere folds onto the same cells: every u-window then holds several times the partners.)
    orient.assign((size_t)n_jobs, (int32_t)c1->axis);
    if (strip_items) {
        bool need[3] = {false, false, false};
        for (int j = 0; j < n_jobs; ++j) {
            if (ctx->auto_orient) {
                const double *b1 = &c1->h_box[(size_t)6 * jobs[2 * j]], *b2 = &c2->h_box[(size_t)6 * jobs[2 * j + 1]];
                double best = -1.0;
                int wax = (c1->axis + 1) % 3;
                for (int a = 0; a < 3; ++a) {
                    const double m = (b1[a] <= b1[3 + a] ? 0.5 * (b1[a] + b1[3 + a]) : 0.0) +
                                     (b2[a] <= b2[3 + a] ? 0.5 * (b2[a] + b2[3 + a]) : 0.0);
                    if (std::fabs(m) > best) { best = std::fabs(m); wax = a; }
                }
                orient[(size_t)j] = (wax + 2) % 3;  // sort axis u whose dropped axis (u + 1) % 3 is wax
            }
            need[orient[(size_t)j]] = true;
        }
        for (int o = 0; o < 3; ++o) {
            if (!need[o]) continue;
            int rc = build_strip_layout(ctx, const_cast<yawhip_catalog *>(c1), o, mode == 3);
            if (rc == YAWHIP_OK && c2 != c1) rc = build_strip_layout(ctx, const_cast<yawhip_catalog *>(c2), o, mode == 3);
            if (rc != YAWHIP_OK) return rc;
            L1[o] = mode == 3 ? &c1->seg[o] : &c1->strips[o];
            L2[o] = mode == 3 ? &c2->seg[o] : &c2->strips[o];
        }
    }
    // Float32 classification (k_count_band32) on strip layouts of unit vectors with up to four edges per bin. Where one
    // side is binned (merged items) the roles are swapped against k_count_band: lane tiles come from the binned catalogue
    // c1, the windows from the unbinned c2 (see the kernel).
    const bool want32 = P.band && strip_items && unit && n_edges <= 4 && ctx->band_fp32 != 0 &&
                        band32_lds(P.weighted, BCAP_MID, (merged ? n_bins : 1) * nf, merged && !uniform_t ? n_bins : 0, n_edges) <=
                            (size_t)ctx->lds_limit;
    // ... and the fine radial grids of separation weights (k_count_band32_fine), when their edges follow the log-spaced model
    if (P.band && strip_items && unit && n_edges > 4 && ctx->band_fp32 != 0 &&
        band32_fine_lds(P.weighted, BCAP_MID, (merged ? n_bins : 1) * nf, uniform_t ? 1 : n_bins, n_edges) <= (size_t)ctx->lds_limit)
        fine32 = build_fine32(t, n_bins, n_edges);
    const bool want_fine = !fine32.empty();
    // (Binned x binned counts of two different catalogues keep c2 on the lanes whichever is sparser: with the 10M data on the
    // lanes and the 100M randoms streamed, DR of config #4 has 570 k items instead of 1.28 M but walks 2.3 x the entries --
    // neighbouring lane objects of a sparse run lie far apart, their common band is long -- 4.1 against 2.2 ms.)
    P.swap = (want32 || want_fine) && merged;
    sides(P.swap);
    if (auto_pick && P.band && unit) {
        // The band kernel decides every entry of a per-object band: unbeatable while a band is a handful of entries of which
        // half are pairs (strip layouts). Without strips a band is the whole u-window of a segment, nearly all of it far away
        // along v -- the FP32 pre-filter of the sweep kernel is made for that. Sparse streamed runs (a few dozen objects: an
        // item is all fixed cost) went to the sweep kernel while the band kernel evaluated in float64; the float32 band kernel
        // has the smaller fixed cost (measured: DD of config #4 0.61 against 0.83 ms, 1M x 1M / 64 patches 0.047 against 0.102,
        // 3M x 0.3M 0.09 against 0.28; sweep stays ahead only where the two sides differ tenfold in density and the items are
        // tiny: DR of config #4 2.09 against 2.23 ms, 0.3M x 3M 0.092 against 0.119) -- so only the float64 band kernel
        // (band_fp32 = 0, more than four edges off the log grid) keeps the density rule.
        bool use_sweep = mode == 0;
        if (!use_sweep && !want32 && !want_fine) {
            double obj_run = 0.0;  // of the densest built orientation
            for (int o = 0; o < 3; ++o)
                if (LS[o]) obj_run = std::max(obj_run, LS[o]->obj_run);
            use_sweep = obj_run < (double)BAND_MIN_STREAM_RUN;
        }
        if (use_sweep) {
            P.kernel = YAWHIP_KERNEL_SWEEP;
            P.band = false;
        }
    }
    P.band32 = want32 && P.band;
    P.band_fine = want_fine && P.band;
    if (!P.band32 && !P.band_fine && P.swap) {  // the sweep kernel streams c1 past lane tiles of c2
        P.swap = false;
        sides(false);
    }
    P.uni = merged || P.band_fine ? uniform_t : true;  // UNI of the band kernels (per-bin items of the others: one threshold row)
    return YAWHIP_OK;
}

// Step 3: objects per lane, the expected window, merged triple runs, the stage capacity.
int Planner::tile_and_stage() {
    const bool band = P.band, strip_items = P.strip_items;
    const int mode = P.mode;
    int R = ctx->tile_r;
    double est_window = 0.0;  // band kernel: expected entries of one window
    if (R == 0) {
        int64_t max_seg = 0;
        if (strip_items) {  // lanes hold runs of a strip layout: their typical (mean) length decides
            int64_t n_runs = 1;
            for (int o = 0; o < 3; ++o)
                if (LL[o]) n_runs = std::max(n_runs, LL[o]->h_vbase[(size_t)LL[o]->n_groups]);
            max_seg = c_lane->n / std::max<int64_t>(n_runs, 1);
            if (mode == 3) max_seg = std::max<int64_t>(max_seg, 4 * MWG * 2);  // at least two objects per lane: per-bin runs are
                                                                                // sparse, the per-item cost outweighs the wider window
        } else {
            for (int j = 0; j < n_jobs; ++j)
                for (int k = 0; k < (c2->nb == 1 ? 1 : n_bins); ++k) max_seg = std::max(max_seg, seg_len(c2, jobs[2 * j + 1], k));
        }
        const int wg = P.lean ? MWG : WG;
        R = max_seg >= 8 * wg * 4 ? 4 : (max_seg >= 4 * wg * 2 ? 2 : 1);
        if (strip_items && R > 2) R = 2;  // on strip runs two objects per lane beat four at every size measured (10M: 2.25 / 2.5 ms, 50M: 68 / 72 ms)
        if (band && strip_items) {
            // band kernel: two neighbouring objects per lane at every density measured once a stage holds the whole
            // window (four per lane: 0.66 / 0.59 ms at the headline, 33 / 24 ms at 50M x 50M, 7.0 / 5.7 ms for RR of
            // config #4). Expected window = the tile's own extent in streamed entries + one band of
            // 2 r_win x (streamed objects of a run per unit of u).
            R = 2;
            auto per_u = [](const auto *c, const StripLayout *const *Ls) {
                int64_t runs = 1;
                for (int o = 0; o < 3; ++o)
                    if (Ls[o]) runs = std::max(runs, Ls[o]->h_vbase[(size_t)Ls[o]->n_groups]);
                double extent = 0.0;
                int n_ext = 0;
                for (int p = 0; p < c->n_patches; ++p) {
                    const double *b = &c->h_box[(size_t)6 * p];
                    double widest = 0.0;
                    for (int a = 0; a < 3; ++a) widest = std::max(widest, b[3 + a] - b[a]);
                    if (widest > 0.0) { extent += widest; ++n_ext; }
                }
                extent = n_ext ? extent / n_ext : 1.0;
                return ((double)c->n / (double)runs) / std::max(extent, 1e-6);
            };
            const double d1 = per_u(c_strm, LS), d2 = per_u(c_lane, LL);
            // binned x binned counts on per-(patch, bin) strip runs: runs are short (35 objects at 10 M, 350 at 100 M objects in
            // 30 bins), bands a handful of entries -- ONE object per lane then evaluates its own band instead of the union of
            // two (DD of config #4: 2.7e7 instead of 5.6e7 entries, 0.63 -> 0.41 ms; RR 3.74 -> 3.57), unless the streamed side
            // is much the sparser one and items are all fixed cost (DR: 2.05e6 items instead of 1.28e6, 1.86 -> 2.25 ms)
            if (mode == 3 && d1 >= 0.5 * d2) R = 1;
            est_window = 64.0 * R * d1 / std::max(d2, 1e-12) + 2.0 * P.rwin_max * d1;
        }
    }
    if (band && R == 0) R = 2;
    // Merged triple runs on the streamed side: one window per item instead of three (k_merge_triples), when the partner
    // strips are exactly c - 1, c, c + 1 (grid at least as wide as the largest separation) AND the merged window still goes
    // through the stage in one piece: cut in pieces it costs more than three whole windows (100M x 100M: 22.0 against 14.9 ms,
    // 50M x 50M with three scales 25.8 against 17.9). The fine-grid kernel has less room (a larger stage costs it residency:
    // 51 fine bins 1.25 against 1.06 ms in a 512-entry stage), so it merges only windows that fit the stage it uses anyway
    // (sparse streamed sides: DR of config #4 2.07 against 2.43). Weighted counts merge like unweighted ones since the kernel
    // with one chunk per round exists: the count kernel takes the same 0.48 ms at the headline in the big stage, the builder
    // searches one window per item instead of three (0.045 against 0.063 ms).
    bool triple = false;
    if ((P.band32 || P.band_fine) && strip_items && ctx->triple_runs && c_strm->n < (1ll << 31) && c1->strip_width > 0.0 &&
        (int)std::floor(layout_sep / c1->strip_width + 1e-6) + 1 == 1) {
        const double est3 = 3.0 * est_window;
        triple = ctx->triple_runs == 2 ||
                 (P.band32 ? est3 <= 0.88 * (B32_CAP_BIG - 4) : est3 <= 0.9 * BCAP_MID);
        for (int o = 0; o < 3 && triple; ++o) {
            if (!LS[o]) continue;
            const int rc = build_triples(ctx, const_cast<yawhip_catalog *>(c_strm), o, mode == 3);
            if (rc == YAWHIP_ERR_OOM) triple = false;  // no room for the copies: three windows per item as before
            else if (rc != YAWHIP_OK) return rc;
        }
        if (triple) est_window = est3;
    }
    P.triple = triple;
    if (g_trace.on) fprintf(stderr, "[yawhip trace] est_window %.1f (triple %d) R %d mode %d\n", est_window, (int)triple, R, mode);
    // stage capacity of the band kernel: the smallest compiled one that holds a whole window (see BCAP_MID)
    int cap = ctx->band_cap == BCAP || ctx->band_cap == BCAP_MID ? ctx->band_cap : 0;
    if (band && cap == 0) cap = R >= 4 || est_window > 0.95 * BCAP ? BCAP_MID : BCAP;
    if (band) {  // (R, stage) pairs that are compiled (the Stage lists of count_enqueue): the plan names one of them
        if (R == 1) cap = BCAP;
        if (R == 4 && cap == BCAP) cap = BCAP_MID;
    }
    int cap32 = ctx->band_cap == B32_CAP || ctx->band_cap == B32_CAP_BIG ? ctx->band_cap
                                                                         : (est_window > 0.75 * (B32_CAP - 4) ? B32_CAP_BIG : B32_CAP);
    // (0.75: window lengths scatter around the estimate, and a window cut in two costs more than a larger stage -- 50M x 50M
    // with windows of ~265 entries: 21.0 ms in the 320-entry stage, 18.3 ms in a 448-entry one)
    if (R == 1) cap32 = B32_CAP;  // (compiled pairs, as above)
    if (R >= 4) cap32 = B32_CAP_BIG;
    if (P.band32) cap = cap32;  // (the fine-grid kernel still stages window by window, with the capacities of k_count_band)
    P.R = R;
    tile_idx = R == 1 ? 0 : (R == 2 ? 1 : 2);
    P.cap = cap;
    P.tile = (int64_t)(P.lean ? MWG : WG) * R;
    P.lean_bins = P.merged ? n_bins : 1;
    P.lds_merged = 2 * MSTAGE * sizeof(ObjF) + (size_t)P.lean_bins * n_edges * sizeof(double) +
                   (size_t)P.lean_bins * P.nf * (P.weighted ? 8 * (MWG / 64) : 4) + (size_t)P.lean_bins * sizeof(float) +
                   (size_t)MWG * sizeof(unsigned int) + 16;
    return YAWHIP_OK;
}

// Step 4: copies of the band kernel's LDS histogram, its compile-time edge count, its LDS.
int Planner::histogram() {
    const int lean_bins = P.lean_bins, nf = P.nf;
    const bool merged = P.merged, uniform_t = P.uniform_t;
    // Copies of the LDS histogram, lanes spread over them by lane id: same-address atomics of one instruction are
    // serialised. Four copies when there are few slots and the bins of neighbouring entries are unrelated (headline:
    // 0.535 ms with four, 0.565 with eight -- the flush grows with the copies). When the histogram has only the fine bins
    // of ONE redshift bin (per-bin items: every hit of the wave lands in 1-3 cells), or when redshift follows position
    // (same_bin: neighbours of the layout's order sharing their bin; clustered survey: 108 -> 62 ms weighted cross count,
    // 31 -> 18 ms autocorrelation count), more copies pay: up to 16 within 2 KB.
    int hp_shift = lean_bins * nf <= 32 ? 2 : 0;
    if (P.band) {
        double coherence = merged ? 0.0 : 1.0;
        if (merged)
            for (int o = 0; o < 3; ++o)
                if (L1[o]) coherence = std::max(coherence, L1[o]->same_bin);
        if (coherence > 0.25) {
            const int cell = P.weighted ? 8 : 4;
            while (hp_shift < (merged ? 3 : 4) && ((size_t)lean_bins * nf * cell << (hp_shift + 1)) <= 2048) ++hp_shift;
        }
    }
    if (ctx->hist_copies_log2 >= 0) hp_shift = ctx->hist_copies_log2;
    P.band_ne = (!merged || uniform_t) && n_edges <= 4 ? n_edges : (nf == 1 ? 2 : 0);  // compile-time edge count of k_count_band
    const bool band_thr = !(P.band_ne >= 2 && (!merged || uniform_t));
    const size_t LDS_FIXED = (size_t)band_lds_fixed(P.cap);
    auto band_lds_for = [&](int shift) {
        return band_lds_dynamic(P.weighted, band_thr, lean_bins, n_edges, 1 << shift, P.cap, merged && !uniform_t ? lean_bins : 1);
    };
    while (P.band && hp_shift > 0 && band_lds_for(hp_shift) + LDS_FIXED > (size_t)ctx->lds_limit) --hp_shift;  // copies are a tunable, not a need
    P.hp_shift = hp_shift;
    P.lds_band = band_lds_for(hp_shift);
    if (P.lean && (P.band ? P.lds_band + LDS_FIXED : P.lds_merged) > (size_t)ctx->lds_limit)
        return fail(YAWHIP_ERR_INVALID, "too many bins x edges for the LDS histogram (%zu bytes)", P.band ? P.lds_band + LDS_FIXED : P.lds_merged);
    return YAWHIP_OK;
}

// Step 5: the item table -- job records, prefix, candidates and bytes, half bands -- and whether the job list has to be split.
int Planner::items() {
    const bool strip_items = P.strip_items;
    const int mode = P.mode;
    // item table: prefix[slot] = first item of the slot; items of a slot are its lane tiles.
    // standard path: slot = (job, bin); merged path: slot = job (one item covers all bins).
    // strip path: slot = job; its potential items = (lane tiles of patch q) x (groups of up to MAX_WIN of the 2*reach+1
    // neighbouring strips), enumerated by the builder kernel from the catalogues' run tables.
    int64_t n_items = 0, cand = 0, abytes = 0;
    const int obj_bytes1 = c1->w ? 32 : 24, obj_bytes2 = c2->w ? 32 : 24;
    // strip paths: the builder's job table. Modes 1/2: the jobs themselves (groups = patches); mode 3: one pseudo job
    // per (job, bin) between the segments (p, k) and (q, k) (groups = segments), numbered like the output slots.
    P.n_sjobs = mode == 3 ? P.n_slots : (int64_t)n_jobs;
    // Half bands: a catalogue counted against ITSELF meets every unordered pair of a diagonal job twice -- a as lane object with b
    // in its window, b as lane object with a in its. On merged triple runs with one object per lane the lane walks only the
    // entries BEHIND its own place in the triple of its strip (one total order of objects in all triples, k_merge_triples): every
    // pair is met once and counts twice (an exact doubling, also of weighted sums). Half the walk of DD / RR of an autocorrelation.
    half_ok = P.band32 && P.triple && P.R == 1 && c1 == c2 && !P.swap && ctx->half_bands != 0 && !for_work;
    if (strip_items) {
        const double width = c1->strip_width;
        // |dv| <= rwin_max (|d latitude| <= sep_angle(rwin_max))  ->  grid indices differ by at most floor(layout_sep / width) + 1
        const int reach = P.reach = width > 0.0 ? (int)std::floor(layout_sep / width + 1e-6) + 1 : 0;
        std::vector<int32_t> sjobs((size_t)2 * P.n_sjobs);
        for (int j = 0; j < n_jobs; ++j)
            for (int k = 0; k < (mode == 3 ? n_bins : 1); ++k) {
                const int64_t sj = mode == 3 ? (int64_t)j * n_bins + k : j;
                sjobs[(size_t)2 * sj] = mode == 3 ? jobs[2 * j] * n_bins + k : jobs[2 * j];
                sjobs[(size_t)2 * sj + 1] = mode == 3 ? jobs[2 * j + 1] * n_bins + k : jobs[2 * j + 1];
            }
        prefix.resize((size_t)P.n_sjobs + 1);
        job_recs.assign((size_t)P.n_sjobs, JobRec{0, 0, 0, 0, 0});
        for (int64_t j = 0; j < P.n_sjobs; ++j) {
            const int p = sjobs[(size_t)2 * j + (P.swap ? 1 : 0)], q = sjobs[(size_t)2 * j + (P.swap ? 0 : 1)];  // streamed, lane side
            const int o = orient[(size_t)(mode == 3 ? j / n_bins : j)];
            const StripLayout &sl1 = *LS[o], &sl2 = *LL[o];
            const std::vector<int64_t> &tiles = sl2.h_tiles[tile_idx];
            JobRec &jr = job_recs[(size_t)j];
            jr.o = o | (half_ok && p == q ? 4 : 0);
            prefix[(size_t)j] = n_items;
            // strips of q whose grid index lies within `reach` of the strips group p occupies
            const int64_t cnt1 = sl1.h_vbase[(size_t)p + 1] - sl1.h_vbase[(size_t)p], lo1 = sl1.h_slo[(size_t)p];
            const int64_t cnt2 = sl2.h_vbase[(size_t)q + 1] - sl2.h_vbase[(size_t)q], lo2 = sl2.h_slo[(size_t)q];
            const int64_t s_lo = std::max<int64_t>(lo1 - reach - lo2, 0), s_hi = std::min<int64_t>(lo1 + cnt1 - 1 + reach - lo2, cnt2 - 1);
            if (cnt1 > 0 && s_hi >= s_lo) {
                const int64_t r0 = sl2.h_vbase[(size_t)q] + s_lo;
                jr.t_lo = tiles[(size_t)r0];
                jr.k_off = lo2 - sl2.h_vbase[(size_t)q] - lo1;  // strip index of lane run r2 on the common grid, relative to group p
                jr.vbase1 = sl1.h_vbase[(size_t)p];
                jr.n_strips1 = (int32_t)cnt1;
                if (P.triple) {  // triple runs of group p: strips [lo1 - 1, lo1 + cnt1], the first one at vbase + 2 p
                    jr.k_off += 1;
                    jr.vbase1 += 2 * (int64_t)p;
                    jr.n_strips1 += 2;
                }
                n_items += (tiles[(size_t)(r0 + s_hi - s_lo + 1)] - tiles[(size_t)r0]) * ((2 * reach + 1 + MAX_WIN - 1) / MAX_WIN);
            }
        }
        prefix[(size_t)P.n_sjobs] = n_items;
    } else {
        prefix.resize((size_t)P.n_slots + 1);
    }
    P.n_pslots = P.merged ? (int64_t)n_jobs : P.n_slots;
    auto patch_total = [](const yawhip_catalog *c, int patch) {  // objects of a patch over all its bins
        return c->h_off[(size_t)(patch + 1) * c->nb] - c->h_off[(size_t)patch * c->nb];
    };
    for (int j = 0; j < n_jobs; ++j) {
        const int p = jobs[2 * j], q = jobs[2 * j + 1];
        if (strip_items && (c1->nb == 1 || c2->nb == 1)) {
            // an unbinned side is one segment used for every bin: sum_k N1(p,k) N2(q,k) factorises
            cand += c1->nb == 1 ? patch_total(c1, p) * patch_total(c2, q) * (c2->nb == 1 ? n_bins : 1)
                                : patch_total(c1, p) * patch_total(c2, q);
        } else {
            for (int k = 0; k < n_bins; ++k) {
                const int64_t n1 = seg_len(c1, p, k), n2 = seg_len(c2, q, k);
                if (!strip_items) prefix[(size_t)j * n_bins + k] = n_items;
                if (n1 > 0 && n2 > 0) {
                    if (!strip_items) n_items += (n2 + P.tile - 1) / P.tile;
                    cand += n1 * n2;
                }
            }
        }
        // algorithmic bytes of a job = every object of the two patches once (Bobj * (N1 + N2))
        abytes += patch_total(c1, p) * obj_bytes1 + patch_total(c2, q) * obj_bytes2;
    }
    if (!strip_items) prefix[(size_t)P.n_pslots] = n_items;
    P.n_items = n_items;
    P.cand = cand;
    P.abytes = abytes;
    P.slab = P.merged ? (int64_t)n_bins * P.nf : P.nf;  // float64 values per item of the weighted slab
    // A weighted call keeps one slab of partial sums per potential item; long job lists of big catalogues would need
    // tens of GB (50M x 50M, three scales: 40 GB). Above the budget -- and when the items no longer fit 31 bits -- the
    // caller cuts the job list in two and counts the halves one after the other (rows of the result are independent).
    P.split = n_jobs > 1 && !for_work &&
              ((P.run_weighted && n_items * P.slab * (int64_t)sizeof(double) > ctx->slab_budget) || n_items >= (1ll << 31));
    return YAWHIP_OK;
}

// Step 6: the per-bin tables and the layout table; all tables packed into one image, uploaded once; the grid divisor.
int Planner::tables() {
    std::vector<float> dthr((size_t)3 * n_bins);  // per bin: pre-filter threshold, certain-band lower / upper bound
    auto round_down = [](double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -4.0f); return f; };
    for (int k = 0; k < n_bins; ++k) {
        const double thi = t[(size_t)k * n_edges + n_edges - 1];
        float thr32 = ctx->debug_no_hits ? 2.0f : round_down(1.0 - 0.5 * thi - FILTER_GUARD);
        dthr[(size_t)3 * k] = thr32;
        dthr[(size_t)3 * k + 1] = 0.f;  // reserved
        dthr[(size_t)3 * k + 2] = 0.f;
    }
    if (P.merged) rwin[0] = P.rwin_max;  // one window for all bins of the merged run
    // band_trim: {cos, sin} of the largest separation angle per row of rwin, float32 for the band kernels ({1, 0}: untrimmed).
    // The caps assume |a|^2 within UNIT_NORM_TOL of 1 (sep_angle).
    const bool trim = ctx->band_trim && c1->unit_norm && c2->unit_norm;
    std::vector<float> ucap((size_t)2 * n_bins);
    for (int k = 0; k < n_bins; ++k) {
        const double th = sep_angle(rwin[(size_t)k]);
        ucap[(size_t)2 * k] = trim ? (float)std::cos(th) : 1.0f;
        ucap[(size_t)2 * k + 1] = trim ? (float)std::sin(th) : 0.0f;
    }
    if (trim) {
        P.cap_c = std::cos(sep_angle(P.rwin_max));
        P.cap_s = std::sin(sep_angle(P.rwin_max));
    }
    // layout table of the call: [o] = c1, [3 + o] = c2 for orientation o (plain layouts: entries 0 and 3)
    DevTab h_tabs[6];
    memset(h_tabs, 0, sizeof h_tabs);
    if (P.strip_items) {
        for (int o = 0; o < 3; ++o) {
            if (!L1[o]) continue;
            const StripLayout &a = *L1[o], &b = *L2[o];
            h_tabs[o] = make_tab(a.x, a.y, a.z, a.w, P.merged ? a.k : nullptr, a.off, a.d_vbase, a.d_slo, a.d_tiles[tile_idx],
                                 a.d_tile_rec[tile_idx], a.d_grid, o, a.q, a.q_stride);
            h_tabs[3 + o] = make_tab(b.x, b.y, b.z, b.w, nullptr, b.off, b.d_vbase, b.d_slo, b.d_tiles[tile_idx],
                                     b.d_tile_rec[tile_idx], b.d_grid, o, b.q, b.q_stride);
            if (P.triple) {
                // the streamed side as merged triple runs: images, weights, offsets and grid index of the triples; the float64
                // columns stay the layout's own (reached through idx by the exact re-evaluation)
                const StripLayout &st = P.swap ? b : a;
                DevTab &tb = h_tabs[P.swap ? 3 + o : o];
                tb = make_tab(st.x, st.y, st.z, st.w3, nullptr, st.off3, st.d_vbase, st.d_slo, st.d_tiles[tile_idx],
                              st.d_tile_rec[tile_idx], st.d_grid3, o, st.q3, st.q3_stride, st.idx3);
                if (half_ok) h_tabs[3 + o].pos3 = (gi32p)(const int32_t *)b.pos3;  // (c1 == c2: the lane side's layout is the streamed one)
            }
        }
    } else {
        h_tabs[0] = make_tab(c1->x, c1->y, c1->z, c1->w, nullptr, c1->off, nullptr, nullptr, nullptr, nullptr, nullptr, c1->axis);
        h_tabs[3] = make_tab(c2->x, c2->y, c2->z, c2->w, nullptr, c2->off, nullptr, nullptr, nullptr, nullptr, nullptr, c2->axis);
    }
    // the tables of the call, packed into the pinned staging buffer and sent with one copy
    static_assert(sizeof(JobRec) == 8 * sizeof(int32_t), "JobRec is 32 bytes");
    const std::vector<float> thr32 = P.band32 ? build_thr32(t, n_bins, n_edges) : (P.band_fine ? fine32 : std::vector<float>());
    // weighted calls: the two-level ordered reduction of the slabs needs the first chunk of every output slot
    std::vector<int64_t> cprefix;
    if (P.run_weighted) {
        cprefix.assign((size_t)P.n_pslots + 1, 0);
        for (int64_t sl = 0; sl < P.n_pslots; ++sl)
            cprefix[(size_t)sl + 1] = cprefix[(size_t)sl] + (prefix[(size_t)sl + 1] - prefix[(size_t)sl] + REDUCE_CHUNK - 1) / REDUCE_CHUNK;
    }
    P.n_chunks = cprefix.empty() ? 0 : cprefix.back();
    const void *src[9] = {P.strip_items ? (const void *)job_recs.data() : (const void *)jobs, prefix.data(), t, dthr.data(),
                          rwin.data(), ucap.data(), thr32.data(), h_tabs, cprefix.data()};
    const size_t bytes[9] = {P.strip_items ? sizeof(JobRec) * (size_t)P.n_sjobs : sizeof(int32_t) * 2 * (size_t)n_jobs,
                             sizeof(int64_t) * ((size_t)P.n_pslots + 1), sizeof(double) * n_bins * n_edges, sizeof(float) * 3 * n_bins,
                             sizeof(double) * n_bins, sizeof(float) * 2 * n_bins, sizeof(float) * thr32.size(), sizeof h_tabs,
                             sizeof(int64_t) * cprefix.size()};
    size_t off[9], off_in = 0;
    for (int i = 0; i < 9; ++i) { off[i] = off_in; off_in = align16(off_in + bytes[i]); }
    std::vector<unsigned char> image(off_in, 0);
    for (int i = 0; i < 9; ++i)
        if (bytes[i]) memcpy(image.data() + off[i], src[i], bytes[i]);
    HIP_TRY(P.d_in.alloc(std::max<size_t>(off_in, 16)));
    HIP_TRY(hipMemcpy(P.d_in, image.data(), off_in, hipMemcpyHostToDevice));  // once per plan
    P.d_jobs = reinterpret_cast<int32_t *>(P.d_in + off[0]);
    P.d_prefix = reinterpret_cast<int64_t *>(P.d_in + off[1]);
    P.d_t = reinterpret_cast<double *>(P.d_in + off[2]);
    P.d_dthr = reinterpret_cast<float *>(P.d_in + off[3]);
    P.d_rwin = reinterpret_cast<double *>(P.d_in + off[4]);
    P.d_ucap = reinterpret_cast<float *>(P.d_in + off[5]);
    P.d_thr32 = reinterpret_cast<float *>(P.d_in + off[6]);
    P.d_tabs = reinterpret_cast<DevTab *>(P.d_in + off[7]);
    P.d_cprefix = reinterpret_cast<int64_t *>(P.d_in + off[8]);
    P.n_orient = (L1[0] ? 1 : 0) + (L1[1] ? 1 : 0) + (L1[2] ? 1 : 0);
    // Workgroups of the band kernels = potential items / grid_div (the kernel loops over the rest). Uniform catalogues, whose
    // items are alike, run best with few, longer-lived workgroups: / 8, / 16 for the per-bin items of binned x binned counts, of
    // which the builder keeps a third (headline 4 / 8 / 16 -> 0.277 / 0.275 / 0.292 ms; config #4 DR 1.59 / 1.53 / 1.48, RR 3.08 /
    // 3.04 / 3.02). On CLUSTERED catalogues items differ a hundredfold and the hardware's dispatch of many short workgroups is the
    // load balancer: / 4 (clustered survey, 3M x 4M: cross count 40.1 against 43.3 ms with / 8, autocorrelation count 7.1
    // against 8.2 with / 16). Clustered = the run the typical OBJECT sits in (sum len^2 / sum len) is more than twice the mean run.
    double skew = 1.0;
    for (const StripLayout *const *LX : {L1, L2})
        for (int o = 0; o < 3; ++o)
            if (LX[o] && LX[o]->built) {
                const yawhip_catalog *cx = LX == L1 ? c1 : c2;
                const double runs = (double)std::max<int64_t>(LX[o]->h_vbase[(size_t)LX[o]->n_groups], 1);
                skew = std::max(skew, LX[o]->obj_run / std::max((double)cx->n / runs, 1.0));
            }
    P.grid_div = ctx->band_grid_div > 0 ? ctx->band_grid_div : (skew > 2.0 ? 4 : (P.mode == 3 ? 16 : 8));
    if (g_trace.on) fprintf(stderr, "[yawhip trace] run skew %.2f -> grid / %d\n", skew, P.grid_div);
    return YAWHIP_OK;
}

// The host half of a count call (its arguments passed check_call): every decision, the tables -- into a plan (see HostPlan).
// for_work: the plan of a cost estimate (count_enqueue's job_work).
int make_plan(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs, const int32_t *jobs,
              int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel, bool want_counts, bool want_sums, bool for_work,
              HostPlan &P) {
    Planner pl{ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, for_work, P};
    int rc = pl.kernel_and_sizes(kernel, want_counts, want_sums);
    if (rc == YAWHIP_OK && !P.empty) rc = pl.layouts();
    if (rc == YAWHIP_OK && !P.empty) rc = pl.tile_and_stage();
    if (rc == YAWHIP_OK && !P.empty) rc = pl.histogram();
    if (rc == YAWHIP_OK && !P.empty) rc = pl.items();
    if (rc == YAWHIP_OK && !P.empty && !P.split) rc = pl.tables();
    if (rc == YAWHIP_OK) g_trace.mark("planned");
    return rc;
}

}  // namespace

namespace yawhip_detail {

// First half of yawhip_count_pairs on ONE device: everything up to and including the copy of the results into the
// context's pinned buffer is put on the context's stream; nothing waits for the device (SWEEP's grid sizing aside).
// The host side of it (make_plan) is done once per distinct set of inputs and looked up afterwards.
// job_work != nullptr: cost estimate only -- the item builder runs, evaluated pairs per job are returned, no counting.
int count_enqueue(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                  const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                  bool want_counts, bool want_sums, int64_t *job_work, CallState &cs, bool fetch_results) {
    cs = CallState{};
    cs.wall0 = std::chrono::steady_clock::now();
    g_trace.mark("enqueue");
    cs.want_counts = want_counts;
    cs.want_sums = want_sums;
    HIP_TRY(hipSetDevice(ctx->device));
    CallKey key(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, want_counts, want_sums, job_work != nullptr);
    HostPlan *plan = nullptr;
    for (HostPlan *cand_plan : ctx->plans)
        if (cand_plan->key == key) {
            plan = cand_plan;
            break;
        }
    if (!plan) {
        std::unique_ptr<HostPlan> fresh(new (std::nothrow) HostPlan());
        if (!fresh) return fail(YAWHIP_ERR_OOM, "host allocation failed");
        const int rc = make_plan(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, want_counts, want_sums, job_work != nullptr, *fresh);
        if (rc != YAWHIP_OK) return rc;
        key.keep();
        fresh->key = std::move(key);
        if (ctx->plans.size() >= MAX_PLANS) {  // evict the least recently used one (nothing of it is in flight: calls are blocking,
            size_t old = 0;                    // and a batch is never longer than the plans kept)
            for (size_t i = 1; i < ctx->plans.size(); ++i)
                if (ctx->plans[i]->stamp < ctx->plans[old]->stamp) old = i;
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            delete ctx->plans[old];
            ctx->plans[old] = ctx->plans.back();
            ctx->plans.pop_back();
        }
        plan = fresh.release();
        ctx->plans.push_back(plan);
    }
    plan->stamp = ++ctx->plan_clock;
    const HostPlan &P = *plan;
    cs.n_out = P.n_out;
    if (P.empty) return YAWHIP_OK;
    if (P.split) return SPLIT_JOBS;
    if (P.run_weighted) HIP_TRY(reserve_call(ctx->d_partials, (size_t)std::max<int64_t>(P.n_items, 1) * P.slab));
    g_trace.mark("plan");
    // results: [counters][counts][sums] in one device buffer; counters and counts are zero when no call of the slot is in
    // flight (CallBufs::dirty; sums are always fully written), and k_call_tail brings back what was asked for
    const size_t o_ctr = 0, o_counts = align16(N_CTR * sizeof(unsigned long long)),
                 o_sums = o_counts + align16((size_t)P.n_out * sizeof(unsigned long long));
    const size_t out_bytes = o_sums + align16((size_t)P.n_out * sizeof(double));
    const unsigned char *const block_was = ctx->out.d;
    HIP_TRY(ctx->out.reserve(out_bytes));
    if (ctx->out.d != block_was) {  // a new block: nothing is known of it, and no call has signed it off
        ctx->dirty = true;
        reinterpret_cast<unsigned long long *>(ctx->out.h)[CTR_DONE] = 0;
    }
    ctx->d_ctr = reinterpret_cast<unsigned long long *>(ctx->out.d + o_ctr);
    ctx->d_counts = reinterpret_cast<unsigned long long *>(ctx->out.d + o_counts);
    ctx->d_sums = reinterpret_cast<double *>(ctx->out.d + o_sums);
    // (no items: no kernel writes the sums either)
    const size_t zero_needed = P.n_items > 0 ? o_sums : out_bytes;
    if (ctx->dirty) ctx->zero_upto = 0;
    if (ctx->zero_upto < zero_needed) {
        HIP_TRY(hipMemsetAsync(ctx->out.d + ctx->zero_upto, 0, zero_needed - ctx->zero_upto, ctx->stream));
        ctx->zero_upto = zero_needed;
    }
    ctx->dirty = true;  // until count_finish has seen this call's tail complete
    cs.seq = ++ctx->seq;
    cs.stamps = P.n_items > 0;  // a builder runs

    int launches = 0;
    const int64_t n_pot = P.n_items;
    int64_t n_items = P.n_items;  // the count grid: all potential items, or what the builder kept (SWEEP)
    unsigned long long seg_cap = 0;  // > 0: the item list is kept in ITEM_SEGS segments of this many records
    g_trace.mark("memset");
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (n_pot > 0) {
        if (n_pot >= (1ll << 31))
            return fail(YAWHIP_ERR_INVALID, "too many work items (%lld) in one job", (long long)n_pot);
        const int bwg = build_wg_for(n_pot);
        const unsigned bgrid = (unsigned)((n_pot + bwg - 1) / bwg);
        // item list in segments (append_items): where the float32 band kernels consume what the strip builder keeps
        if (P.strip_items && (P.band32 || P.band_fine) && !job_work && ctx->item_segments)
            seg_cap = (unsigned long long)((bgrid + ITEM_SEGS - 1) / ITEM_SEGS) * (unsigned long long)bwg;
        HIP_TRY(reserve_call(ctx->d_items, seg_cap ? (size_t)(seg_cap * ITEM_SEGS) : (size_t)n_pot));
        unsigned char *kept_flags = nullptr;  // weighted runs of the culling builders: which potential items write a slab
        if (P.run_weighted && P.sweep) {
            HIP_TRY(reserve_call(ctx->d_kept, (size_t)n_pot));
            HIP_TRY(hipMemsetAsync(ctx->d_kept.ptr, 0, (size_t)n_pot, ctx->stream));
            kept_flags = ctx->d_kept.ptr;
        }
        if (P.strip_items)
            hipLaunchKernelGGL(k_build_items_strips, dim3(bgrid), dim3(bwg), 0, ctx->stream, P.d_tabs,
                               reinterpret_cast<const JobRec *>(P.d_jobs), P.d_prefix, (int)P.n_sjobs,
                               P.triple ? 0 : P.reach, (int)P.tile, P.rwin_max, P.cap_c, P.cap_s, P.swap ? 1 : 0, P.triple ? 1 : 0,
                               n_pot, ctx->d_items.ptr,
                               ctx->d_ctr, kept_flags, seg_cap);
        else if (P.sweep)
            hipLaunchKernelGGL(k_build_items<true>, dim3(bgrid), dim3(bwg), 0, ctx->stream, view_of(c1), view_of(c2),
                               P.d_jobs, P.d_prefix, (int)P.n_pslots, n_bins, (int)P.tile,
                               P.d_rwin, n_pot, ctx->d_items.ptr, ctx->d_ctr, kept_flags);
        else
            hipLaunchKernelGGL(k_build_items<false>, dim3(bgrid), dim3(bwg), 0, ctx->stream, view_of(c1), view_of(c2),
                               P.d_jobs, P.d_prefix, (int)P.n_pslots, n_bins, (int)P.tile, P.d_rwin, n_pot,
                               ctx->d_items.ptr, ctx->d_ctr, nullptr);
        HIP_TRY(hipGetLastError());
        ++launches;
        // The count kernels are launched over all potential items and return at once for indices beyond the
        // number the builder kept (device counter): no host round trip between the two kernels.
        n_items = n_pot;
        if (P.strip_items && !P.band && n_pot > SYNC_GRID_MIN_ITEMS) {
            // SWEEP: the strip path keeps about one potential item in five; a grid over all of them spends ~0.2 ms
            // dispatching workgroups that exit at once (measured at 1.6e6 potential items, 10M x 10M), more than
            // this round trip (~0.05 ms) costs. Small calls (one GPU's share of a sharded job list) skip it.
            // (The band kernel sizes its grid from the potential items and loops: no round trip.)
            HIP_TRY(hipMemcpyAsync(ctx->out.h, ctx->d_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            n_items = (int64_t)reinterpret_cast<unsigned long long *>(ctx->out.h)[0];
        }
    }
    if (job_work) {  // cost estimate only: evaluated pairs per job from the item list, no counting
        HIP_TRY(reserve_call(ctx->d_jobwork, (size_t)n_jobs));
        HIP_TRY(hipMemsetAsync(ctx->d_jobwork.ptr, 0, sizeof(unsigned long long) * (size_t)n_jobs, ctx->stream));
        if (n_pot > 0) {
            hipLaunchKernelGGL(k_item_work, dim3((unsigned)((n_pot + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_items.ptr,
                               ctx->d_ctr, P.merged ? 1 : n_bins, ctx->d_jobwork.ptr);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(job_work, ctx->d_jobwork.ptr, sizeof(int64_t) * (size_t)n_jobs, hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return YAWHIP_OK;
    }
    // two-level ordered reduction of the weighted slabs (k_reduce_chunks / k_reduce_slots), per output slot; prefix = first
    // potential item of every output slot, chunk prefix = first chunk of every output slot
    auto reduce_partials = [&]() -> hipError_t {
        const int64_t n_oslots = P.n_pslots, values = P.slab, n_chunks = P.n_chunks;
        hipError_t er = reserve_call(ctx->d_chunk_sums, (size_t)std::max<int64_t>(n_chunks, 1) * values);
        if (er != hipSuccess) return er;
        const int thr = 256;
        const bool all_kept = !(P.run_weighted && P.sweep);
        if (n_chunks > 0)
            hipLaunchKernelGGL(k_reduce_chunks, dim3((unsigned)((n_chunks * values + thr - 1) / thr)), dim3(thr), 0, ctx->stream,
                               ctx->d_partials.ptr, all_kept ? nullptr : ctx->d_kept.ptr, P.d_prefix, P.d_cprefix,
                               (int)n_oslots, (int)values, ctx->d_chunk_sums.ptr, ctx->d_ctr);
        hipLaunchKernelGGL(k_reduce_slots, dim3((unsigned)((n_oslots * values + thr - 1) / thr)), dim3(thr), 0, ctx->stream,
                           ctx->d_chunk_sums.ptr, P.d_cprefix, (int)n_oslots, (int)values, ctx->d_sums,
                           n_chunks > 0 ? nullptr : ctx->d_ctr);
        return hipGetLastError();
    };
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->evc0, ctx->stream));
    // The count kernels. Their variants are picked from the plan (pick; each list runs from the last variant to the first:
    // the compiler lays the kernels out in the reverse order, which keeps the code object as it was).
    // Every launch records its variant in cs.variant[weighted] (yawhip_stats.count_variant*).
    // Band kernels: grid from the number of POTENTIAL items (known on the host); the kernel reads the number the builder kept
    // from the device counter, workgroups beyond it exit, workgroups loop if more were kept than the grid holds.
    // The strip builder keeps about one potential item in five, ordinary items are all kept.
    int64_t grid = P.strip_items && n_pot > 65536 ? n_pot / P.grid_div : n_pot;
    // Batches of consecutive items (one flush of the histogram per batch) are a tunable, off by default: consecutive
    // items are tiles of the same run, so on clustered data a batch strings the heaviest items together on one
    // workgroup (measured: DD of the clustered survey with 31 fine bins 7.2 -> 20.6 ms with batches of four), and on
    // uniform data the flush they save is not what the time goes to (2.27 ms either way at the headline, 51 fine bins).
    const int batch_log2 = ctx->band_batch_log2 >= 0 ? ctx->band_batch_log2 : 0;
    if (!P.run_weighted) grid = std::max<int64_t>(grid >> batch_log2, 8);
    grid = std::min<int64_t>((grid + 7) & ~7ll, 1ll << 22);
    const dim3 band_grid((unsigned)grid), wave(64);
    // 32-bit LDS counters: one stage adds at most 64 R x CAP to a cell, so flush at the latest every
    // 2^32 / (64 R CAP) stages (2^17 for two objects per lane and 192-entry stages, 2^15 for four and 288)
    int flush_log2 = ctx->flush_log2;
    while (flush_log2 > 0 && ((uint64_t)64 * P.R * 2 * P.cap << flush_log2) >= (1ull << 32)) --flush_log2;  // (x 2: half bands count double)
    const unsigned flush_mask = (1u << flush_log2) - 1u;
    const std::pair<int, int> stage{P.R, P.cap};
    const std::pair<bool, bool> rows{P.merged, P.uni};
    auto launch_band32 = [&](bool wgt) -> hipError_t {
        const size_t lds = band32_lds(P.weighted, P.cap, P.lean_bins * P.nf, P.merged && !P.uniform_t ? n_bins : 0, n_edges);
        const bool one_chunk = P.triple || !P.strip_items;  // every item has one window
        return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
            return pick<Int<4>, Int<3>, Int<2>>(n_edges, [&](auto ne) {
                return pick<Rows<true, false>, Rows<true, true>, Rows<false, true>>(rows, [&](auto r) {
                    return pick<Stage<4, B32_CAP_BIG>, Stage<2, B32_CAP_BIG>, Stage<2, B32_CAP>, Stage<1, B32_CAP>>(stage, [&](auto s) {
                        using S = decltype(s);
                        using M = decltype(r);
                        auto kern = one_chunk ? k_count_band32_one<S::R, S::CAP, w, ne, M::MERGED, M::UNI>
                                              : k_count_band32<S::R, S::CAP, w, ne, M::MERGED, M::UNI>;
                        cs.variant[w] = variant_code(one_chunk ? VF_BAND32_ONE : VF_BAND32, S::R, S::CAP, w, ne, M::MERGED, M::UNI);
                        return launch(kern, band_grid, wave, lds, ctx->stream, P.d_tabs, ctx->d_items.ptr, n_bins, P.d_t,
                                      P.d_thr32, P.d_rwin, P.d_ucap, flush_mask, P.swap ? 1 : 0, ctx->d_counts,
                                      ctx->d_partials.ptr, ctx->d_ctr, seg_cap);
                    });
                });
            });
        });
    };
    auto launch_band64 = [&](bool wgt) -> hipError_t {
        return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
            return pick<Int<0>, Int<4>, Int<3>, Int<2>>(P.band_ne, [&](auto ne) {
                return pick<Rows<true, false>, Rows<true, true>, Rows<false, true>>(rows, [&](auto r) {
                    return pick<Stage<4, BCAP_MID>, Stage<2, BCAP_MID>, Stage<2, BCAP>, Stage<1, BCAP>>(stage, [&](auto s) {
                        using S = decltype(s);
                        using M = decltype(r);
                        cs.variant[w] = variant_code(VF_BAND, S::R, S::CAP, w, ne, M::MERGED, M::UNI);
                        return launch(k_count_band<S::R, S::CAP, w, ne, M::MERGED, M::UNI>, band_grid, wave, P.lds_band, ctx->stream,
                                      P.d_tabs, ctx->d_items.ptr, n_bins, n_edges, P.d_t, P.d_rwin, flush_mask,
                                      P.hp_shift, w ? 0 : batch_log2, ctx->d_counts, ctx->d_partials.ptr, ctx->d_ctr);
                    });
                });
            });
        });
    };
    auto launch_fine = [&](bool wgt) -> hipError_t {
        const size_t lds = band32_fine_lds(P.weighted, P.cap, P.lean_bins * P.nf, P.uniform_t ? 1 : n_bins, n_edges);
        return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
            return pick<Rows<true, false>, Rows<true, true>, Rows<false, false>, Rows<false, true>>(rows, [&](auto r) {
                return pick<Stage<4, BCAP_MID>, Stage<2, BCAP_MID>, Stage<2, BCAP>, Stage<1, BCAP>>(stage, [&](auto s) {
                    using S = decltype(s);
                    using M = decltype(r);
                    cs.variant[w] = variant_code(VF_BAND32_FINE, S::R, S::CAP, w, 0, M::MERGED, M::UNI);
                    return launch(k_count_band32_fine<S::R, S::CAP, w, M::MERGED, M::UNI>, band_grid, wave, lds, ctx->stream,
                                  P.d_tabs, ctx->d_items.ptr, n_bins, n_edges, P.d_t, P.d_thr32, P.d_rwin,
                                  P.d_ucap, flush_mask, P.swap ? 1 : 0, ctx->d_counts, ctx->d_partials.ptr, ctx->d_ctr, seg_cap);
                });
            });
        });
    };
    // The lean kernel (k_count_merged / _occ8) and k_count, one workgroup per item: grids in pieces of at most 2^32 - 1
    // work-items per launch dimension.
    auto in_pieces = [&](int wg, auto &&launch_at) -> hipError_t {
        const int64_t max_grid = (1ll << 31) / wg;
        for (int64_t base = 0; base < n_items; base += max_grid) {
            const hipError_t e = launch_at(dim3((unsigned)std::min(max_grid, n_items - base)), base);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    auto launch_lean = [&](bool wgt) -> hipError_t {
        return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
            return pick<Bool<false>, Bool<true>>(P.nf == 1, [&](auto nf1) {
                return pick<Bool<false>, Bool<true>>(P.merged, [&](auto m) {
                    return pick<Int<4>, Int<2>, Int<1>>(P.R, [&](auto r) {
                        cs.variant[w] = variant_code(r <= 2 ? VF_MERGED_OCC8 : VF_MERGED,  // (the choice of pick_count_merged)
                                                      r, 0, w, 0, m, false, false, false, nf1);
                        return in_pieces(MWG, [&](dim3 g, int64_t base) {
                            return launch(pick_count_merged<r, w, nf1, m>(), g, dim3(MWG), P.lds_merged, ctx->stream, P.d_tabs,
                                          ctx->d_items.ptr, n_bins, n_edges, P.d_t, P.d_dthr, P.d_rwin, base,
                                          ctx->d_counts, ctx->d_partials.ptr, ctx->d_ctr);
                        });
                    });
                });
            });
        });
    };
    // LDS of k_count: two stages + thresholds + histogram(s)
    const size_t lds_fixed = 2 * STAGE * (sizeof(Obj) + sizeof(ObjF)) + (size_t)((n_edges + 1) & ~1) * sizeof(double);
    auto lds_for = [&](bool w, bool priv) { return lds_fixed + (size_t)P.nf * (priv ? WG : 1) * (w ? 8 : 4); };
    auto launch_plain = [&](bool wgt) -> hipError_t {
        const bool priv = lds_for(wgt, true) <= (size_t)ctx->lds_limit;
        return pick<Bool<true>, Bool<false>>(wgt, [&](auto w) {
            return pick<Bool<false>, Bool<true>>(priv, [&](auto pv) {
                return pick<Bool<false>, Bool<true>>(P.filter, [&](auto f) {
                    return pick<Int<4>, Int<2>, Int<1>>(P.R, [&](auto r) {
                        cs.variant[w] = variant_code(VF_COUNT, r, 0, w, 0, false, false, pv, f);
                        return in_pieces(WG, [&](dim3 g, int64_t base) {
                            return launch(k_count<r, w, pv, f>, g, dim3(WG), lds_for(w, pv), ctx->stream, view_of(c1), view_of(c2),
                                          ctx->d_items.ptr, n_bins, n_edges, P.d_t, P.d_dthr, base, ctx->d_counts,
                                          ctx->d_partials.ptr, ctx->d_ctr);
                        });
                    });
                });
            });
        });
    };
    const bool band_ran = n_items > 0 && P.lean && P.band;
    auto launch_count = [&](bool wgt) {
        if (band_ran) return P.band32 ? launch_band32(wgt) : (P.band_fine ? launch_fine(wgt) : launch_band64(wgt));
        return P.lean ? launch_lean(wgt) : launch_plain(wgt);
    };
    if (n_items > 0 && P.run_unweighted) {
        HIP_TRY(launch_count(false));
        ++launches;
    }
    if (n_items > 0 && P.run_weighted) {
        HIP_TRY(launch_count(true));
        ++launches;
        HIP_TRY(reduce_partials());
        launches += 2;
    }
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->evc1, ctx->stream));
    if (!P.weighted && want_sums) {
        const int thr = 256;
        hipLaunchKernelGGL(k_counts_to_double, dim3((unsigned)((P.n_out + thr - 1) / thr)), dim3(thr), 0, ctx->stream,
                           ctx->d_counts, ctx->d_sums, P.n_out, ctx->d_ctr);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    // the tail brings back the counters and whatever was asked for, into pinned memory, and cleans behind itself
    // (fetch_results = false: the caller reduces the results on the device first and fetches what is left; counters only here,
    // and the counts stay where they are: the slot stays dirty)
    const size_t fetch = !fetch_results ? o_counts : (want_sums ? out_bytes : (want_counts ? o_sums : o_counts));
    const size_t clean = std::min(fetch, o_sums);
    const bool sums_written = P.n_items > 0 && (P.run_weighted || want_sums);
    cs.cleaned = clean == o_sums;
    cs.zero_after = sums_written ? o_sums : ctx->zero_upto;
    const unsigned n_copy = (unsigned)(fetch / 16), n_clean = (unsigned)(clean / 16);
    static_assert(N_CTR * sizeof(unsigned long long) % 16 == 0 && (CTR_DONE + 2) * sizeof(unsigned long long) <= N_CTR * sizeof(unsigned long long),
                  "the tail's words lie inside the counter block");
    if (fetch / 16 > 0xffffffffull) return fail(YAWHIP_ERR_INVALID, "result block too large (%zu bytes)", fetch);
    unsigned char *const out_d = ctx->out.d;
    hipLaunchKernelGGL(k_call_tail, dim3(std::min((n_copy + TAIL_WG - 1) / TAIL_WG, TAIL_MAX_GRID)), dim3(TAIL_WG), 0, ctx->stream,
                       reinterpret_cast<uint4 *>(out_d), reinterpret_cast<uint4 *>(ctx->out.h), n_copy, n_clean,
                       (unsigned long long)cs.seq);
    HIP_TRY(hipGetLastError());
    ++launches;
    cs.pending = true;
    cs.o_ctr = o_ctr; cs.o_counts = o_counts; cs.o_sums = o_sums;
    cs.band_ran = band_ran; cs.run_unweighted = P.run_unweighted; cs.run_weighted = P.run_weighted;
    cs.cand = P.cand; cs.abytes = P.abytes; cs.n_pot = n_pot; cs.segmented = seg_cap != 0;
    cs.launches = launches; cs.kernel = P.kernel; cs.mode = P.mode;
    cs.n_orient = P.n_orient;
    cs.band_variant = !band_ran ? 0 : (P.band32 ? 32 : (P.band_fine ? 33 : 64));
    cs.merged_triples = band_ran && P.triple ? 1 : 0;
    g_trace.mark("launched");
    return YAWHIP_OK;
}

// Second half: wait for the context's stream, hand the results (contiguous rows of the jobs given to count_enqueue) and
// the statistics over.
// row_index != nullptr: row r of this call's result goes to row row_index[r] of the caller's arrays (rows of row_len values):
// the devices of a multi-device call write their shares straight into place.
// wait_done: wait for the active slot's ev_done (recorded by the caller behind everything this call put on the stream)
// instead of the whole stream -- the requests of a batch behind it keep running.
int count_finish(yawhip_ctx *ctx, const CallState &cs, int64_t *fine_counts, double *fine_sums, yawhip_stats *stats,
                 const int32_t *row_index, int64_t row_len, bool wait_done) {
    if (stats) memset(stats, 0, sizeof *stats);
    const int64_t n_rows = !row_index ? 1 : (row_len > 0 ? cs.n_out / row_len : 0), row = row_index ? row_len : cs.n_out;
    if (!cs.pending) {
        place_rows<int64_t>(fine_counts, nullptr, n_rows, row, row_index);
        place_rows<double>(fine_sums, nullptr, n_rows, row, row_index);
        return YAWHIP_OK;
    }
    g_trace.mark("meanwhile");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->spin_wait) {
        // poll for up to 2 ms (a headline call takes 0.5 ms; the wake-up of a blocked thread costs ~0.01 ms), then block.
        // What is polled is the completion word k_call_tail writes into the slot's pinned block behind the results -- no
        // runtime call per look -- unless the caller put more behind the tail: then the stream or the slot's ev_done, as before.
        const unsigned long long *done_word = reinterpret_cast<const unsigned long long *>(ctx->out.h) + CTR_DONE;
        auto query = [&]() { return wait_done ? hipEventQuery(ctx->ev_done) : hipStreamQuery(ctx->stream); };
        hipError_t qe = hipErrorNotReady;
        const auto spin0 = std::chrono::steady_clock::now();
        do {
            if (cs.word_wait) {
                if (__atomic_load_n(done_word, __ATOMIC_ACQUIRE) == cs.seq) qe = hipSuccess;
            } else {
                qe = query();
            }
            if (qe != hipErrorNotReady) break;
            __builtin_ia32_pause();
        } while (std::chrono::steady_clock::now() - spin0 < std::chrono::milliseconds(2));
        if (qe == hipSuccess && cs.word_wait) {  // one look at the runtime: an asynchronous error surfaces here, not a call later
            const hipError_t late = query();
            if (late != hipErrorNotReady) qe = late;  // (not ready: the packets behind the tail, or other slots' requests)
        }
        if (qe == hipErrorNotReady) qe = wait_done ? hipEventSynchronize(ctx->ev_done) : hipStreamSynchronize(ctx->stream);
        HIP_TRY(qe);
    } else {
        HIP_TRY(wait_done ? hipEventSynchronize(ctx->ev_done) : hipStreamSynchronize(ctx->stream));
    }
    g_trace.mark("waited");
    if (cs.cleaned) {  // the tail has left [counters][counts] of the slot's block at zero
        ctx->dirty = false;
        ctx->zero_upto = cs.zero_after;
    }
    place_rows(fine_counts, reinterpret_cast<const int64_t *>(ctx->out.h + cs.o_counts), n_rows, row, row_index);
    place_rows(fine_sums, reinterpret_cast<const double *>(ctx->out.h + cs.o_sums), n_rows, row, row_index);
    const unsigned long long *ctr = reinterpret_cast<const unsigned long long *>(ctx->out.h + cs.o_ctr);
    g_trace.mark("copied");
    if (stats) {
        float ms = 0.f, cms = 0.f;
        if (cs.stamps) {
            // device clock stamps (see CTR_T_BUILD): the builder's start to the tail's start, and the latest builder exit to the
            // start of the first kernel behind the count kernel(s) -- the count kernels with the dispatch gaps on either side
            unsigned long long built = 0;
            for (int sg = 0; sg < ITEM_SEGS; ++sg) built = std::max(built, ctr[SEG_EXIT_CTR(sg)]);
            ms = (float)((double)(ctr[CTR_T_TAIL] - ctr[CTR_T_BUILD]) * CLOCK_MS);
            cms = (float)((double)(ctr[CTR_T_COUNTED] - built) * CLOCK_MS);
        } else {
            HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            HIP_TRY(hipEventElapsedTime(&cms, ctx->evc0, ctx->evc1));
        }
        stats->count_ms = cms;
        stats->candidate_pairs = cs.cand;
        unsigned long long tile_pairs = 0;
        for (int i = 0; i < EVAL_SLOTS; ++i) tile_pairs += ctr[10 + 8 * (size_t)i];
        stats->evaluated_pairs = (int64_t)tile_pairs * ((cs.run_unweighted ? 1 : 0) + (cs.run_weighted ? 1 : 0));
        if (cs.band_ran) {  // band kernel: the entries its lanes really walked (both launches of a weighted + counts call)
            unsigned long long ev = 0;
            for (int i = 0; i < EVAL_SLOTS; ++i) ev += ctr[8 + 8 * (size_t)i];
            stats->evaluated_pairs = (int64_t)ev;
        }
        stats->algorithmic_bytes = cs.abytes;
        stats->n_workgroups = cs.n_pot > 0 ? (int64_t)ctr[0] : 0;
        if (cs.segmented && cs.n_pot > 0)
            for (int sg = 0; sg < ITEM_SEGS; ++sg) stats->n_workgroups += (int64_t)ctr[ITEM_SEG_CTR(sg)];
        stats->n_launches = cs.launches;
        stats->kernel_used = cs.kernel;
        stats->layout_mode = cs.mode;
        stats->n_orientations = cs.n_orient;
        stats->band_variant = cs.band_variant;
        stats->merged_triples = cs.merged_triples;
        stats->count_variant = cs.variant[0];
        stats->count_variant_weighted = cs.variant[1];
        if (cs.band_ran)
            for (int i = 0; i < EVAL_SLOTS; ++i) stats->exact_reevaluations += (int64_t)ctr[9 + 8 * (size_t)i];
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - cs.wall0).count();
    }
    g_trace.mark("stats");
    return YAWHIP_OK;
}

void add_stats(yawhip_stats &total, const yawhip_stats &part, bool side_by_side) {
    total.candidate_pairs += part.candidate_pairs;
    total.evaluated_pairs += part.evaluated_pairs;
    total.algorithmic_bytes += part.algorithmic_bytes;
    total.n_workgroups += part.n_workgroups;
    total.n_launches += part.n_launches;
    total.kernel_used = part.kernel_used;
    total.layout_mode = part.layout_mode;
    total.n_orientations = std::max(total.n_orientations, part.n_orientations);
    total.band_variant = part.band_variant;
    total.merged_triples = part.merged_triples;
    total.count_variant = merge_variant(total.count_variant, part.count_variant);
    total.count_variant_weighted = merge_variant(total.count_variant_weighted, part.count_variant_weighted);
    total.exact_reevaluations += part.exact_reevaluations;
    if (side_by_side) {  // devices of one call run at the same time: the slowest counts
        total.kernel_ms = std::max(total.kernel_ms, part.kernel_ms);
        total.count_ms = std::max(total.count_ms, part.count_ms);
    } else {             // pieces of one job list on one device run one after the other
        total.kernel_ms += part.kernel_ms;
        total.count_ms += part.count_ms;
    }
}

// One job list on one device, cut in halves as often as count_enqueue asks for (SPLIT_JOBS).
int run_single(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs, const int32_t *jobs,
               int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel, int64_t *fine_counts, double *fine_sums,
               yawhip_stats *stats, const std::function<void()> *meanwhile) {
    // meanwhile: host work of the caller that does not need the result, done while the device counts (once)
    CallState cs;
    int rc = count_enqueue(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, fine_counts != nullptr, fine_sums != nullptr,
                           nullptr, cs);
    if (meanwhile && (rc == YAWHIP_OK || rc == SPLIT_JOBS)) (*meanwhile)();
    if (rc == YAWHIP_OK) return count_finish(ctx, cs, fine_counts, fine_sums, stats);
    if (rc != SPLIT_JOBS) return rc;
    const int32_t half = n_jobs / 2;
    const size_t row = (size_t)n_bins * (size_t)(n_edges - 1);
    yawhip_stats a{}, b{};
    rc = run_single(ctx, c1, c2, half, jobs, n_bins, n_edges, t, kernel, fine_counts, fine_sums, &a);
    if (rc != YAWHIP_OK) return rc;
    rc = run_single(ctx, c1, c2, n_jobs - half, jobs + 2 * (size_t)half, n_bins, n_edges, t, kernel,
                    fine_counts ? fine_counts + (size_t)half * row : nullptr, fine_sums ? fine_sums + (size_t)half * row : nullptr, &b);
    if (rc != YAWHIP_OK) return rc;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        add_stats(*stats, a, false);
        add_stats(*stats, b, false);
        stats->total_ms = a.total_ms + b.total_ms;
    }
    return YAWHIP_OK;
}

}  // namespace yawhip_detail

extern "C" {

int yawhip_count_pairs(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                       const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                       int64_t *fine_counts, double *fine_sums, yawhip_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const int rc_args = check_call(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t);
    if (rc_args != YAWHIP_OK) return rc_args;
    if (ctx->peers.empty() || n_jobs < 2)
        return run_single(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, fine_counts, fine_sums, stats);
    // ---- several devices: the independent jobs are split over them (replaces the reference's process pool,
    // src/yaw/utils/parallel.py:251-346). Every device holds both catalogues; a job's rows of the result come from
    // exactly one device, so nothing has to be reduced: the rows are copied into place.
    const size_t n_dev = ctx->peers.size() + 1;
    if (c1->replicas.size() != n_dev - 1 || c2->replicas.size() != n_dev - 1)
        return fail(YAWHIP_ERR_MISMATCH, "catalogue was not uploaded to every device of the context");
    const auto wall0 = std::chrono::steady_clock::now();
    // the plan: evaluated pairs per job from the item builder (device 0), longest-processing-time-first over the devices;
    // it depends on the inputs only and is kept for the next call with the same inputs
    // (the inputs of the cost estimate below, and the device count)
    CallKey key(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, false, false, true, (int32_t)n_dev);
    if (!(ctx->plan.key == key)) {
        std::vector<int64_t> work((size_t)n_jobs, 0);
        CallState cs;
        int rc = count_enqueue(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, false, false, work.data(), cs);
        if (rc != YAWHIP_OK) return rc;
        std::vector<int32_t> order((size_t)n_jobs);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return work[(size_t)a] > work[(size_t)b]; });
        std::vector<double> load(n_dev, 0.0);
        ctx->plan.parts.assign(n_dev, {});
        const double fixed = 2.0e5;  // evaluated-pair equivalent of touching a job at all
        for (int32_t j : order) {
            const size_t d = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
            ctx->plan.parts[d].push_back(j);
            load[d] += (double)work[(size_t)j] + fixed;
        }
        for (auto &part : ctx->plan.parts) std::sort(part.begin(), part.end());
        key.keep();
        ctx->plan.key = std::move(key);
    }
    const int64_t row = (int64_t)n_bins * (n_edges - 1);
    std::vector<CallState> states(n_dev);
    std::vector<std::vector<int32_t>> sub(n_dev);
    std::vector<char> later(n_dev, 0);  // shares that have to be cut in pieces: counted after the others, one by one
    for (size_t d = 0; d < n_dev; ++d) {  // enqueue everywhere first: the devices work side by side
        for (int32_t j : ctx->plan.parts[d]) { sub[d].push_back(jobs[2 * j]); sub[d].push_back(jobs[2 * j + 1]); }
        yawhip_ctx *dc = d == 0 ? ctx : ctx->peers[d - 1];
        const yawhip_catalog *a = d == 0 ? c1 : c1->replicas[d - 1], *b = d == 0 ? c2 : c2->replicas[d - 1];
        const int rc = count_enqueue(dc, a, b, (int32_t)ctx->plan.parts[d].size(), sub[d].data(), n_bins, n_edges, t, kernel,
                                     fine_counts != nullptr, fine_sums != nullptr, nullptr, states[d]);
        if (rc == SPLIT_JOBS) {
            later[d] = 1;
        } else if (rc != YAWHIP_OK) {
            for (size_t e = 0; e < d; ++e) (void)hipStreamSynchronize((e == 0 ? ctx : ctx->peers[e - 1])->stream);
            return rc;
        }
    }
    std::vector<int64_t> rows_c;
    std::vector<double> rows_s;
    yawhip_stats total{}, part{};
    int rc_all = YAWHIP_OK;
    for (size_t d = 0; d < n_dev; ++d) {  // every device's copy into its pinned buffer is already under way: drain in turn
        yawhip_ctx *dc = d == 0 ? ctx : ctx->peers[d - 1];
        const yawhip_catalog *a = d == 0 ? c1 : c1->replicas[d - 1], *b = d == 0 ? c2 : c2->replicas[d - 1];
        const size_t nj = ctx->plan.parts[d].size();
        int rc;
        if (later[d]) {  // a share that is counted in pieces: through a temporary, then into place
            if (fine_counts) rows_c.resize(nj * (size_t)row);
            if (fine_sums) rows_s.resize(nj * (size_t)row);
            rc = run_single(dc, a, b, (int32_t)nj, sub[d].data(), n_bins, n_edges, t, kernel, fine_counts ? rows_c.data() : nullptr,
                            fine_sums ? rows_s.data() : nullptr, &part);
            if (rc == YAWHIP_OK) {
                place_rows(fine_counts, (const int64_t *)rows_c.data(), (int64_t)nj, row, ctx->plan.parts[d].data());
                place_rows(fine_sums, (const double *)rows_s.data(), (int64_t)nj, row, ctx->plan.parts[d].data());
            }
        } else {         // rows go from the device's pinned buffer straight into the caller's arrays
            rc = count_finish(dc, states[d], fine_counts, fine_sums, &part, ctx->plan.parts[d].data(), row);
        }
        if (rc != YAWHIP_OK) { rc_all = rc; continue; }  // keep draining the other devices
        add_stats(total, part, true);
    }
    (void)hipSetDevice(ctx->device);  // leave the thread on the context's first device, as single-device calls do
    if (rc_all != YAWHIP_OK) return rc_all;
    total.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (stats) *stats = total;
    return YAWHIP_OK;
}

int yawhip_job_work(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs, const int32_t *jobs,
                    int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel, int64_t *work) {
    if (!ctx || !work) return fail(YAWHIP_ERR_INVALID, "yawhip_job_work: NULL argument");
    for (int j = 0; j < n_jobs; ++j) work[j] = 0;
    const int rc = check_call(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t);
    if (rc != YAWHIP_OK) return rc;
    CallState cs;
    return count_enqueue(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, false, false, work, cs);
}

}  // extern "C"
