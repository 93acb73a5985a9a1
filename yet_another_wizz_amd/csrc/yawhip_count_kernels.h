// What the count kernels (the kernel units: yawhip.hip and yawhip_kernel_*.hip, one per kernel family) and the count call that
// plans and launches them (yawhip_count.hip) have to agree on, said once: the geometry of the kernels (workgroup, stage and
// tile sizes, the LDS a variant takes), the layout of the counter block at the head of a call's result block, and the launch
// interface -- one record of what a launch needs from the call and the functions that put the kernels on its stream. Included
// by yawhip_count.hip and, through yawhip_count_device.h, by the kernel units; private like yawhip_internal.h.
#ifndef YAWHIP_COUNT_KERNELS_H
#define YAWHIP_COUNT_KERNELS_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "yawhip_internal.h"

#pragma GCC visibility push(hidden)

namespace yawhip_detail {

// ------------------------------------------------------------------------------------------------
// Geometry
// ------------------------------------------------------------------------------------------------
constexpr int WG = 256;      // threads per workgroup = 4 waves of 64
constexpr int STAGE = 256;   // streamed objects per LDS stage (one per thread)
constexpr int MSTAGE = 64;   // stage of the merged path: smaller -> less LDS -> more workgroups per CU
constexpr int MAX_EDGES = 512;
constexpr int BAND_MIN_STREAM_RUN = 64;  // AUTO: objects per run of the streamed side (as the typical object sees it) from which the band kernel is used
constexpr int64_t SYNC_GRID_MIN_ITEMS = 400000;  // potential items from which the count grid is sized exactly (one host sync)
constexpr int MAX_STRIP_REACH = 12;  // strip pairing is used while sqrt(t_max) <= 12 grid spacings

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
// (cap_lo64 / cap_hi64 and cap_lo32 / cap_hi32 of the kernels evaluate the second one.)
inline double sep_angle(double rwin) { return 2.0 * std::asin(std::min(1.0, 0.5 * (rwin + 2e-9))); }

constexpr int EVAL_SLOTS = 256;  // statistics counters, one 64-byte line each (a single hot address would serialise)
constexpr int BUILD_WG = 1024;       // most threads per workgroup of the item builders
// Builder workgroups: one atomic per workgroup appends its items, so few large workgroups suit long lists (16 k atomics on
// the one counter cost 0.15 ms at 4 M potential items), but 1024 threads make 300 workgroups for 256 CUs at the headline
// and half the chip waits for the CUs that got two (+0.07 ms): 256 threads while that keeps the atomics below 4096.
constexpr int BUILD_WG_SMALL = 256;
inline int build_wg_for(int64_t n_pot) { return n_pot / 256 <= 4096 ? BUILD_WG_SMALL : BUILD_WG; }
constexpr int BUILD_PREFIX_LDS = 1024;  // job tables up to this many entries are searched in LDS by the strip builder (8 KB: no occupancy cost)
// Segments of the item list where the strip builder feeds the float32 band kernels (append_items): eight addresses take the
// appends of a launch side by side, and the band kernels give XCD x segment x.
constexpr int ITEM_SEGS = 8;

constexpr int BCAP = 192;       // window objects per LDS stage. 192: the window of a 128-object lane tile at equal densities (128 +- 11
                                // entries + one band) fits in one stage; 6.2 KB -> 26 single-wave workgroups per CU. Measured
                                // 160 / 176 / 192 / 208 / 224: count kernel 0.545 / 0.529 / 0.523 / 0.535 / 0.531 ms at the headline
// Stage capacities the band kernel is compiled for. A stage should hold the whole window of a lane tile (the tile's own
// extent in streamed entries plus one band): a window cut into stages makes every stage wait for the longest clipped band
// while the lanes whose bands lie in the other stage idle (50M x 50M, bands of 216 entries: 400 trips per 256 lane objects
// with 288-entry stages against 219 in one stage).
// (416-entry stages were measured too: never ahead of 288 -- 23.3 / 23.3 ms at 50M x 50M, 0.70 / 0.59 ms at the headline.)
constexpr int BCAP_MID = 288;
// Stage of k_count_band32 (entries, 12 bytes each + 8 with weights). 320 holds two windows of a typical lane tile (128 objects
// at equal densities: ~142 entries each) -- measured 192 / 288 / 320 / 448 at the headline: 0.367 / 0.355 / 0.350 / 0.360 ms,
// weighted 0.521 / 0.519 / 0.511 / 0.556, RR of config #4 4.65 / 4.44 / 4.41 / 4.89 (the larger the stage, the fewer workgroups
// a CU holds). The big one is for lane tiles whose single window would not fit (denser streamed side, four objects per lane).
constexpr int B32_CAP = 320;
constexpr int B32_CAP_BIG = 512;

constexpr double BAND32_GUARD_SQRT = 2.1e-7;  // coefficient of sqrt(t) in the float32 guard g(t), see k_count_band32
// float32 words per bin of the threshold table: NE == 2: {c, h_in, h_out, 0}; else per edge {t - g, t + g}
__host__ __device__ constexpr int thr32_width(int ne) { return ne == 2 ? 4 : 2 * ne; }
// ... and per row of the table of k_count_band32_fine: {m, a, 0, 0}, then {t_j - g, t_j + g} per edge
__host__ __device__ constexpr int fine32_width(int n_edges) { return 4 + 2 * n_edges; }

constexpr int REDUCE_CHUNK = 32;  // consecutive potential items whose slabs k_reduce_chunks adds into one chunk sum
constexpr int TAIL_WG = 256;
constexpr unsigned TAIL_MAX_GRID = 64;
constexpr double CLOCK_MS = 1.0e-5;  // milliseconds per tick of wall_clock64

// LDS of a workgroup, per kernel family: the plan checks it against the limit, the launch asks for it, and where the kernel
// lays out its dynamic LDS by the same sizes, host and device agree through the one function.
int band_lds_fixed(int cap);  // k_count_band: its static image (BandLds<cap>::FIXED; defined with it, yawhip_kernel_band64.hip)
__host__ __device__ inline bool band_small_hist(bool weighted, int nslots, int hp) { return (size_t)nslots * hp * (weighted ? 8 : 4) <= 512; }
// dynamic LDS bytes of a band workgroup (host and device agree through this one function)
__host__ __device__ inline size_t band_lds_dynamic(bool weighted, bool need_thr, int nkb, int n_edges, int hp, int cap, int thr_rows) {
    const int nslots = nkb * (n_edges - 1);
    return (weighted ? (size_t)(cap + 2) * 8 : 0) + (need_thr ? (size_t)thr_rows * n_edges * sizeof(double) : 0) +
           (band_small_hist(weighted, nslots, hp) ? 0 : (size_t)nslots * hp * (weighted ? 8 : 4)) + 16;
}
// dynamic LDS of a k_count_band32 workgroup (host and device agree through this one function)
__host__ __device__ inline size_t band32_lds(bool weighted, int cap, int nslots, int thr_rows, int ne) {
    // (+ 48: the plain one-annulus count with one threshold row walks its bands downwards onto four sentinel entries in front
    // of each column, yawhip_band32.inc DOWN)
    return (size_t)3 * (cap + 4) * 4 + (weighted ? (size_t)(cap + 4) * 8 : 0) + (size_t)nslots * (weighted ? 8 : 4) +
           (size_t)thr_rows * thr32_width(ne) * 4 + 32 + (!weighted && ne == 2 && thr_rows == 0 ? 48 : 0);
}
__host__ __device__ inline size_t band32_fine_lds(bool weighted, int cap, int nslots, int rows, int n_edges) {
    return (size_t)3 * (cap + 4) * 4 + (weighted ? (size_t)(cap + 2) * 8 : 0) + (size_t)nslots * (weighted ? 8 : 4) + 64 * 8 +
           (size_t)rows * fine32_width(n_edges) * 4 + 48;
}
// (these rest on the records the kernels stage: defined with them, yawhip_kernel_plain.hip and yawhip_kernel_lean.hip)
size_t count_lds(bool weighted, bool priv, int n_edges);   // k_count: two stages + thresholds + histogram(s)
size_t merged_stage_lds();                                 // k_count_merged: its two float32 stages ...
size_t merged_lds(bool weighted, int bins, int n_edges);   // ... + thresholds, histogram(s), pre-filter thresholds, survivor queue

// ------------------------------------------------------------------------------------------------
// Counter block: N_CTR 64-bit words at the head of a call's result block, zero when the call starts, brought to the host by
// k_call_tail with the results.
//   CTR_KEPT            items the builder kept (a list kept in segments: ITEM_SEG_CTR)
//   BAND_ENTRY_CTR(i)   band entries the lanes walked          } statistics, spread over EVAL_SLOTS slots i of one 64-byte
//   EXACT_EVAL_CTR(i)   exact float64 re-evaluations           } line each by item (ticket) or builder workgroup
//   TILE_PAIR_CTR(i)    lane-tile x window pairs of the kept items (the builder's estimate of the evaluated pairs)
//   ITEM_SEG_CTR(s)     items in segment s of the list; with SEG_EXIT_CTR(s) (below) in free words of the first slots' lines
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
// ------------------------------------------------------------------------------------------------
constexpr int CTR_KEPT = 0, CTR_T_BUILD = 1, CTR_T_COUNTED = 2, CTR_T_TAIL = 3, CTR_TICKET = 4, CTR_DONE = 6;
constexpr int CTR_SLOT_WORDS = 8;  // words of a slot's line
// (the index keeps the type of i: the kernels index with 32- and 64-bit slot numbers)
template <typename I> __host__ __device__ constexpr auto BAND_ENTRY_CTR(I i) { return 8 + CTR_SLOT_WORDS * i; }
template <typename I> __host__ __device__ constexpr auto EXACT_EVAL_CTR(I i) { return 9 + CTR_SLOT_WORDS * i; }
template <typename I> __host__ __device__ constexpr auto TILE_PAIR_CTR(I i) { return 10 + CTR_SLOT_WORDS * i; }
__host__ __device__ constexpr int ITEM_SEG_CTR(int seg) { return 12 + CTR_SLOT_WORDS * seg; }  // counters[]: one 64-byte line each
__host__ __device__ constexpr int SEG_EXIT_CTR(int seg) { return ITEM_SEG_CTR(seg) + 1; }
constexpr int N_CTR = 8 + CTR_SLOT_WORDS * EVAL_SLOTS;
static_assert(BAND_ENTRY_CTR(0) % CTR_SLOT_WORDS == 0 && EXACT_EVAL_CTR(0) % CTR_SLOT_WORDS == 1 && TILE_PAIR_CTR(0) % CTR_SLOT_WORDS == 2 &&
                  ITEM_SEG_CTR(0) % CTR_SLOT_WORDS == 4 && SEG_EXIT_CTR(0) % CTR_SLOT_WORDS == 5,
              "the segment words and the per-slot words take different places of a slot's line");
static_assert(CTR_DONE < BAND_ENTRY_CTR(0) && ITEM_SEGS <= EVAL_SLOTS && TILE_PAIR_CTR(EVAL_SLOTS - 1) < N_CTR, "counter block");

// ------------------------------------------------------------------------------------------------
// Launch interface: what the kernels of a call need from it, filled by count_enqueue from the plan and the active call
// buffers. The launch functions (kernel units) put kernels on L.stream and return the launch's status; they decide nothing --
// which variant of a count kernel runs follows from the selectors, and a combination that is not compiled is
// hipErrorInvalidValue.
// ------------------------------------------------------------------------------------------------
enum class CountFamily : int32_t { PLAIN, LEAN, BAND64, BAND32, BAND32_FINE };  // k_count, k_count_merged(_occ8), k_count_band, k_count_band32(_one), k_count_band32_fine
struct CountLaunch {
    hipStream_t stream = nullptr;
    // variant selectors
    CountFamily family = CountFamily::PLAIN;
    int R = 0, cap = 0, band_ne = 0;  // objects per lane, entries per stage, compile-time edge count of k_count_band
    bool merged = false, uni = false, nf1 = false, filter = false, priv = false, one_chunk = false;
    // grids and sizes
    unsigned build_grid = 0, build_wg = 0, band_grid = 0;
    int64_t n_pot = 0;    // potential items: the builder's threads
    int64_t n_items = 0;  // k_count, k_count_merged: one workgroup per item
    int64_t n_build_jobs = 0;  // entries of the builder's job table (strip builder: its jobs; else output slots)
    int64_t n_oslots = 0;      // output slots of the slab reduction
    int64_t tile = 0, slab = 0, n_chunks = 0;
    size_t lds = 0;       // dynamic LDS of the count kernel
    unsigned flush_mask = 0;
    int batch_log2 = 0, hp_shift = 0, n_bins = 0, n_edges = 0, reach = 0;
    bool swap = false, triple = false;
    unsigned long long seg_cap = 0;
    double rwin_max = 0.0, cap_c = 1.0, cap_s = 0.0;
    // tables of the plan
    CatView c1{}, c2{};  // the catalogues' plain layouts (k_build_items, k_count)
    const DevTab *d_tabs = nullptr;
    const int32_t *d_jobs = nullptr;
    const int64_t *d_prefix = nullptr, *d_cprefix = nullptr;
    const double *d_t = nullptr, *d_rwin = nullptr;
    const float *d_dthr = nullptr, *d_ucap = nullptr, *d_thr32 = nullptr;
    // buffers of the call
    Item *d_items = nullptr;
    unsigned char *d_kept = nullptr;  // weighted runs of the culling builders: which potential items write a slab, else null
    unsigned long long *d_ctr = nullptr, *d_counts = nullptr;
    double *d_partials = nullptr, *d_chunk_sums = nullptr, *d_sums = nullptr;
};

hipError_t launch_build_strips(const CountLaunch &L);   // k_build_items_strips
hipError_t launch_build_windows(const CountLaunch &L);  // k_build_items<true>: windowed items, empty ones dropped
hipError_t launch_build_whole(const CountLaunch &L);    // k_build_items<false>: every item streams its whole segment
hipError_t launch_item_work(const CountLaunch &L, int slots_per_job, unsigned long long *job_work);
// the count kernel of L.family; its variant code (yawhip_stats.count_variant*) goes to *variant
hipError_t launch_count(const CountLaunch &L, bool weighted, int32_t *variant);
// ... which is one of these, each defined in the unit of its kernel family (launch_count chooses by L.family and L.one_chunk)
hipError_t launch_plain(const CountLaunch &L, bool weighted, int32_t *variant);
hipError_t launch_lean(const CountLaunch &L, bool weighted, int32_t *variant);
hipError_t launch_band64(const CountLaunch &L, bool weighted, int32_t *variant);
hipError_t launch_band32(const CountLaunch &L, bool weighted, int32_t *variant);
hipError_t launch_band32_one(const CountLaunch &L, bool weighted, int32_t *variant);
hipError_t launch_fine(const CountLaunch &L, bool weighted, int32_t *variant);
hipError_t launch_reduce_chunks(const CountLaunch &L);
hipError_t launch_reduce_slots(const CountLaunch &L);
hipError_t launch_counts_to_double(const CountLaunch &L, int64_t n_out);
hipError_t launch_call_tail(hipStream_t stream, unsigned char *dev, unsigned char *host, unsigned n_copy, unsigned n_clean,
                            unsigned long long seq);

}  // namespace yawhip_detail

#pragma GCC visibility pop
#endif
