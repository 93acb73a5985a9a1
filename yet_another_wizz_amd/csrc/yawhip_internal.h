// Shared by the translation units behind the C ABI of include/yawhip.h -- yawhip.hip and yawhip_kernel_*.hip (count kernels and their
// launch layer), yawhip_count.hip (the count call that plans and launches them; they share yawhip_count_kernels.h besides),
// yawhip_ingest.hip (catalogue upload and layouts), yawhip_dense.hip (dense epilogue) and yawhip_api.hip (contexts, options,
// error reporting, wrappers of the other units): error reporting, the records the kernels and the layouts share, the context
// and catalogue handles, and the few functions that cross units. Private: never installed, not part of the C ABI.
#ifndef YAWHIP_INTERNAL_H
#define YAWHIP_INTERNAL_H
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "yawhip.h"
#include "yawhip_devmem.h"
#include "yawhip_healpix.h"
#include "yawhip_sort.h"

#pragma GCC visibility push(hidden)  // nothing declared here is exported: the library's symbols are the yawhip_* functions

namespace yawhip_detail {
// YAWHIP_TRACE=1: wall-clock marks of a call's host side, printed to stderr when the call returns (diagnostics; two
// clock reads per mark when off)
struct Trace {
    bool on = getenv("YAWHIP_TRACE") != nullptr;
    int n = 0;
    const char *name[32];
    std::chrono::steady_clock::time_point at[32];
    void mark(const char *what) {
        if (on && n < 32) { name[n] = what; at[n++] = std::chrono::steady_clock::now(); }
    }
    void flush() {
        if (on && n > 1) {
            fprintf(stderr, "[yawhip trace]");
            for (int i = 1; i < n; ++i)
                fprintf(stderr, " %s +%.1f", name[i], std::chrono::duration<double, std::micro>(at[i] - at[i - 1]).count());
            fprintf(stderr, " | total %.1f us\n", std::chrono::duration<double, std::micro>(at[n - 1] - at[0]).count());
        }
        n = 0;
    }
};
extern thread_local Trace g_trace;  // (defined with fail, yawhip_api.hip)

constexpr int MWG = 64;      // threads per workgroup of the lean kernel (k_count_merged)
static_assert(MWG == 64, "the band kernels are single-wave workgroups: their lane tile is 64 * R objects");
constexpr int SEG_STRIPS_MIN_RUN = 16;  // mean objects per (patch, bin, strip) run of the lane side from which mode 3 is used
constexpr int SPLIT_JOBS = 1;  // internal status of count_enqueue: nothing was enqueued, the caller must split the job list
constexpr double UNIT_NORM_TOL = 1e-9;  // |a|^2 of a unit vector lies this close to 1 (yawhip_catalog::unit_norm)

extern thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...);  // (yawhip_api.hip) records the message of yawhip_last_error, returns code
// a failed HIP call of entry point `fn` as its error code
inline int hip_fail(const char *fn, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? YAWHIP_ERR_OOM : YAWHIP_ERR_HIP, "%s failed: %s", fn, hipGetErrorString(e));
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? YAWHIP_ERR_OOM : YAWHIP_ERR_HIP, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

struct CatView {
    const double *x, *y, *z, *w;  // w may be null
    const int64_t *off;           // [P*nb+1]
    int nb;
    const double *key;            // the column the segments are sorted by (x, y or z)
    int axis;                     // 0, 1, 2
};

constexpr int MAX_WIN = 3;  // windows (partner runs of c1) one work item can carry
struct alignas(16) Item {  // one unit of work for a workgroup: a lane tile of c2 and up to MAX_WIN windows of c1
    int64_t a0;    // first lane object (c2 side)
    int32_t na;    // lane objects (<= 256*R, <= 64*R on the SWEEP / BAND paths)
    int32_t slot;  // output slot: job * n_bins + bin, or the job itself on the strip path (bits 0..29);
                   // bits 30..31: orientation = which of the catalogues' three strip layouts a0 / b0 index
    int32_t pot;   // index among all potential items (slab index of weighted partial sums)
    int32_t nwin;  // windows in use (>= 1 for a kept item)
    int64_t b0[MAX_WIN];  // first streamed object of every window (c1 side)
    int32_t nb[MAX_WIN];  // streamed objects of every window
    int32_t pad_;
};
static_assert(sizeof(Item) == 64, "Item layout");

// One layout of one catalogue as the kernels see it. The count kernels and the strip builder receive a table of six:
// [o] = layout of c1 for orientation o, [3 + o] = layout of c2 (plain layouts: entry 0 / 3 only).
// Orientation o = the sort axis u of the layout (0 = x, 1 = y, 2 = z); strips are cut along v = (o + 2) % 3 and the
// third axis w = (o + 1) % 3 is the one the projection drops: a job uses the orientation whose w points towards its
// two patches, where the (u, v) projection of the sphere is least compressed.
// (pointers carry the global address space: loaded from a table the compiler could not tell, and would use flat loads)
typedef const __attribute__((address_space(1))) double *gf64p;
typedef const __attribute__((address_space(1))) int32_t *gi32p;
typedef const __attribute__((address_space(1))) int64_t *gi64p;
typedef const __attribute__((address_space(1))) float *gf32p;
// Lane image of a strip layout: the float32 images of an object's coordinates and its bin id as ONE 16-byte record, what a
// lane of the float32 band kernels fetches per object (k_make_q writes it beside the columns; 0 where the layout has no bin
// ids -- unbinned catalogues, per-segment layouts: their kernels ignore the bin). A lane loads its R records whether it
// has R objects or not, so the table ends with the records of a whole lane tile of the largest kind (64 lanes x 4 objects).
struct alignas(16) LaneObj {
    float x, y, z;
    int32_t bin;
};
static_assert(sizeof(LaneObj) == 16, "LaneObj is read with one 16-byte load");
constexpr int64_t LANE_IMAGE_PAD = 256;
typedef float lane_words __attribute__((ext_vector_type(4)));  // a record as the kernels load it: the bin id is the bit pattern of .w
typedef const __attribute__((address_space(1))) lane_words *glanep;
struct DevTab {
    gf64p x, y, z, w;          // columns; w may be null
    gi32p k;                   // bin id per object (merged cross-correlation layouts), else null
    gi64p off;                 // run offsets [V+1] (strip layouts) or segment offsets
    gi64p vbase, slo, tiles;   // strip layouts: first run of a group, its grid index, lane-tile prefix over runs
    const struct TileRec *tile_rec;  // strip layouts: first object, length, run and end keys of every lane tile
    const struct RunGrid *grid;      // strip layouts: per-run record and index along the sort axis (item builder)
    gf32p qx, qy, qz;          // strip layouts: float32 images of the columns (k_count_band32: the streamed side, LDS-DMA)
    glanep q4;                 // strip layouts: the same images with the bin id, one record per object (the lane side), else null
    gi32p idx;                // merged triple runs (streamed side): index of an entry in the layout's own order, else null
    gi32p pos3;                // lane side of a self count on merged triple runs: place of an object in its own strip's triple, else null
    int32_t axis;              // sort axis inside a run / segment
    int32_t pad_;
};
__device__ __forceinline__ gf64p tab_key(const DevTab &t) { return t.axis == 0 ? t.x : (t.axis == 1 ? t.y : t.z); }

// Tables of the strip item builder. Every thread of the builder walks a chain of dependent loads and the chain's length
// is the kernel's run time (0.06 of the 0.55 ms of a headline call), so what the host or the layout build can precompute
// travels as one record per job, per lane tile and per run instead of being looked up table by table.
struct alignas(16) TileRec {   // per lane tile of a layout (one table per tile size)
    int64_t a0;    // first object
    int32_t na;    // objects (<= tile)
    int32_t run;   // run the tile belongs to
    double klo, khi;  // sort keys of the tile's first and last object (k_tile_keys): what the builder's window starts from
};
static_assert(sizeof(TileRec) == 32, "TileRec is read as two 16-byte words");
struct JobRec {    // per job of a call
    int64_t t_lo;      // first lane tile of the job (absolute index into the lane side's tile table)
    int64_t k_off;     // strip of the streamed group facing lane run r2 under neighbour offset d: r2 + k_off + d
    int64_t vbase1;    // first run of the streamed group
    int32_t n_strips1; // runs of the streamed group
    int32_t o;         // orientation: which pair of layouts the job runs on
};
// Per-run index along the sort axis: the key range [first, last] of a run is cut into RUN_GRID cells by
// cell(key) = clamp(floor((key - first) * inv), 0, RUN_GRID - 1), and g[c] = number of entries whose cell is < c
// (g[0] = 0, g[RUN_GRID] = run length). cell() is monotone in the key and evaluated by the same instructions when the
// table is built and when it is queried, so for any w the first entry with key >= w and the first with key > w both lie in
// [g[cell(w)], g[cell(w) + 1]] -- exactly, whatever the rounding of the product: the bisection over a run of 900 entries
// (ten dependent loads) becomes one table look-up and four steps.
// In front of g[] stands what the item builder needs to know about the run before it looks at g[]: where the run begins, how
// long it is and the keys of its first and last entry, as the double the builder compares (a merged triple run's keys are
// float32 images, widened). One aligned read of the record replaces the loads of two offsets, two keys and inv from three
// tables, two of them dependent on the first. A zeroed record is an empty run.
constexpr int RUN_GRID = 64;
struct alignas(16) RunGrid {
    int64_t b0;                  // first entry of the run in its table
    double first, last;          // keys of its first and last entry (0 for an empty run)
    double inv;                  // RUN_GRID / (last - first), 0 for a run with one distinct key
    uint32_t n;                  // entries: 0 = empty run, nothing else of the record is looked at
    uint32_t g[RUN_GRID + 1];
};
static_assert(sizeof(RunGrid) == 304 && offsetof(RunGrid, n) == 32, "RunGrid: a 36-byte head in front of g[]");
// What a run and a tile record count for in yawhip_catalog_device_bytes: their sizes before the builder's heads were added
// (inv + g[RUN_GRID + 2]; a0, na, run). The reported figure is pinned by tests/test_gpu_ingest.py.
constexpr int64_t RUN_GRID_ACCOUNTED = 8 + 4 * (RUN_GRID + 2), TILE_REC_ACCOUNTED = 16;
__device__ __forceinline__ int run_cell(double key, double first, double inv) {
    const double f = (key - first) * inv;
    return f >= (double)RUN_GRID ? RUN_GRID - 1 : (f >= 1.0 ? (int)f : 0);
}

// the count call's buffers grow with a quarter to spare: calls of similar sizes keep them
template <typename T>
hipError_t reserve_call(DevBuf<T> &buf, size_t n) { return buf.reserve(n, n / 4 + 64); }

// Small per-call tables travel in ONE host-to-device copy from a pinned staging buffer, and the results (counters, counts,
// sums) come back in ONE copy into pinned memory: a dozen pageable copies of a few hundred bytes each cost more host
// time than the kernels of a small call take.
struct Arena {
    unsigned char *h = nullptr;  // pinned host image ...
    DevPtr<unsigned char> d;     // ... and device buffer of the same size
    size_t cap = 0;
    Arena() = default;
    Arena(Arena &&o) noexcept : h(std::exchange(o.h, nullptr)), d(std::move(o.d)), cap(std::exchange(o.cap, 0)) {}
    Arena &operator=(Arena &&o) noexcept {  // (h has no owner type: the two trade places, nothing is freed here)
        std::swap(h, o.h); std::swap(d, o.d); std::swap(cap, o.cap);
        return *this;
    }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        const size_t want = n + n / 4 + 4096;
        // (coherent: k_call_tail writes a result block and its completion word while the host polls for it)
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&h), want, hipHostMallocPortable | hipHostMallocCoherent);
        if (e == hipSuccess) e = d.alloc(want);
        if (e == hipSuccess) cap = want; else release();
        return e;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        d.release();
        h = nullptr;
        cap = 0;
    }
};
inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// Everything ONE count call in flight owns: its work items, partial sums, result block and timing events (the tables it
// reads are its plan's, HostPlan). A context keeps MAX_BATCH of these; the active one is the base-class part of the context
// (the count code says ctx->d_items ...), the others are parked -- yawhip_count_pairs_dense_batch activates one per
// request so that several counts of a measurement are on the stream at once (use_slot).
struct CallBufs {
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evc0 = nullptr, evc1 = nullptr, ev_done = nullptr;
    DevBuf<Item> d_items;
    unsigned long long *d_ctr = nullptr, *d_counts = nullptr;  // counters and results: windows into `out`, set by every count call
    double *d_sums = nullptr;
    DevBuf<double> d_partials;
    DevBuf<double> d_chunk_sums;
    DevBuf<unsigned char> d_kept;   // weighted runs: 1 for potential items the builder kept
    Arena out;   // results (device -> host)
    // The [counters][counts] part of out.d is zero whenever no call of the slot is in flight: k_call_tail zeroes it behind its
    // reads. `dirty` is set while that may not hold -- from the moment a call starts to enqueue until count_finish has seen it
    // complete, so also after a call that failed or was abandoned on the way, after a builder-only call (job_work) and after a
    // call whose tail left the counts in place (fetch_results = false) -- and the next call then fills the block itself.
    // zero_upto: the bytes from the start of out.d known to be zero while !dirty (a call with a larger result block than the
    // last one's has its counts where that one's sums were).
    bool dirty = true;
    size_t zero_upto = 0;
    uint64_t seq = 0;  // sequence number of the slot's calls: what k_call_tail writes into the pinned block when it is done
    Arena comb;  // yawhip_count_pairs_dense: recombination tables in, per-scale values out
    hipError_t make_events() {
        hipError_t e = hipSuccess;
        for (hipEvent_t *ev : {&ev0, &ev1, &evc0, &evc1, &ev_done})
            if (e == hipSuccess && !*ev) e = hipEventCreate(ev);
        return e;
    }
    void release_all() {
        d_items.release(); d_partials.release(); d_chunk_sums.release(); d_kept.release();
        out.release(); comb.release();
        for (hipEvent_t *ev : {&ev0, &ev1, &evc0, &evc1, &ev_done}) {
            if (*ev) (void)hipEventDestroy(*ev);
            *ev = nullptr;
        }
    }
};
constexpr int MAX_BATCH = 4;  // counts of one measurement on the stream at once (DD, DR, RD, RR)
constexpr size_t MAX_PLANS = 16;  // plans kept per context (least recently used one goes)

struct HostPlan;  // what a call derives from its inputs on the host, kept for the next call with the same inputs (yawhip_count.hip)

// What is to be counted, as every step of a count call passes it on: made once at the C entry point from its arguments, then
// handed down by reference. A step that counts a part of the job list (the halves of run_single, a device's share in
// yawhip_count_pairs) makes its record from the whole call's with with_jobs.
struct CountArgs {
    const yawhip_catalog *c1, *c2;
    int32_t n_jobs;
    const int32_t *jobs;  // [n_jobs][2] patch ids (c1, c2)
    int32_t n_bins, n_edges;
    const double *t;      // [n_bins][n_edges] thresholds
    int32_t kernel;       // YAWHIP_KERNEL_*
    CountArgs with_jobs(int32_t n, const int32_t *j) const {
        CountArgs a = *this;
        a.n_jobs = n;
        a.jobs = j;
        return a;
    }
};

// Everything a plan depends on: the catalogue pair (by upload id), the option set, sizes, kernel, the outputs asked for, job
// list and thresholds (compared exactly) -- and, for the job partition of a multi-device call, the device count. A key made
// from a call's arguments borrows their job list and thresholds; keep() gives it copies of its own before it is stored.
struct CallKey {
    uint64_t c1_uid = 0, c2_uid = 0, opt_gen = 0, hash = 0;
    int32_t n_jobs = 0, n_bins = 0, n_edges = 0, kernel = 0, n_dev = 0;
    bool want_counts = false, want_sums = false, for_work = false;
    const int32_t *jobs = nullptr;
    const double *t = nullptr;
    std::vector<int32_t> own_jobs;
    std::vector<double> own_t;

    CallKey() = default;
    CallKey(const yawhip_ctx *ctx, const CountArgs &a, bool want_counts, bool want_sums, bool for_work,
            int32_t n_dev = 0);  // (yawhip_count.hip)
    // (moves keep jobs / t valid: a vector's elements stay where they are; copies would not)
    CallKey(CallKey &&) = default;
    CallKey &operator=(CallKey &&) = default;
    CallKey(const CallKey &) = delete;
    CallKey &operator=(const CallKey &) = delete;

    void keep() {
        own_jobs.assign(jobs, jobs + 2 * (size_t)n_jobs);
        own_t.assign(t, t + (size_t)n_bins * n_edges);
        jobs = own_jobs.data();
        t = own_t.data();
    }
    bool operator==(const CallKey &o) const {
        return hash == o.hash && c1_uid == o.c1_uid && c2_uid == o.c2_uid && opt_gen == o.opt_gen && n_jobs == o.n_jobs &&
               n_bins == o.n_bins && n_edges == o.n_edges && kernel == o.kernel && n_dev == o.n_dev && want_counts == o.want_counts &&
               want_sums == o.want_sums && for_work == o.for_work &&
               memcmp(jobs, o.jobs, sizeof(int32_t) * 2 * (size_t)n_jobs) == 0 &&
               memcmp(t, o.t, sizeof(double) * (size_t)n_bins * n_edges) == 0;
    }
};

struct StripLayout {
    bool built = false;
    DevPtr<double> x, y, z, w;
    DevPtr<int32_t> k;                // bin id per object (patch-level layout of a binned catalogue)
    DevPtr<float> q;                  // [3][q_stride] float32 images of x, y, z (k_count_band32)
    int64_t q_stride = 0;
    DevPtr<LaneObj> q4;               // [n + LANE_IMAGE_PAD] the same images with the bin id (or 0), one record per object
    DevPtr<int64_t> off;              // [V+1] offsets of the runs
    std::vector<int64_t> h_off;       // same on the host
    std::vector<int64_t> h_vbase;     // [G+1] first run of every group
    std::vector<int64_t> h_slo;       // [G]   global strip index of a group's first run
    std::vector<int64_t> h_tiles[3];  // [V+1] prefix of lane tiles over the runs, for tiles of MWG * {1, 2, 4} objects
    DevPtr<int64_t> d_vbase, d_slo, d_tiles[3];
    DevPtr<TileRec> d_tile_rec[3];    // [tiles] first object, length, run and end keys of every lane tile
    DevPtr<RunGrid> d_grid;           // [V+1] per-run index along the sort axis (item builder)
    // merged triple runs (k_merge_triples), built when a float32 band kernel first streams this layout
    bool triples = false;
    DevPtr<float> q3;                 // [3][q3_stride] float32 images in merged order (3 n entries)
    int64_t q3_stride = 0;
    DevPtr<double> w3;                // weights in merged order
    DevPtr<int32_t> idx3;             // [3 n] entry -> index in the layout's own order
    DevPtr<int32_t> pos3;             // [n] object -> its place in the triple run centred on its own strip
    DevPtr<int64_t> off3;             // [V + 2 G + 1] offsets of the triple runs: group g has its strips + 2, first one = vbase[g] + 2 g
    DevPtr<RunGrid> d_grid3;          // [V + 2 G + 1]
    int64_t n_groups = 0;
    int64_t device_bytes = 0;
    double obj_run = 0.0;             // run length seen by the typical object (sum len^2 / sum len)
    double same_bin = 0.0;            // fraction of neighbours in the layout's order that share their bin (binned patch-level layouts)
    void release_triples() {
        q3.release(); w3.release(); idx3.release(); pos3.release(); off3.release(); d_grid3.release();
        triples = false;
    }
    void release() { *this = StripLayout{}; }  // (host tables and statistics go with the device memory: nothing reads them unbuilt)
};

}  // namespace yawhip_detail

struct yawhip_ctx : yawhip_detail::CallBufs {
    int device = 0;
    hipStream_t stream = nullptr;
    int tile_r = 0;          // 0 = auto
    int hist_copies_log2 = -1;  // band kernel: log2 of the copies of the LDS histogram (-1 = auto)
    int band_batch_log2 = -1;   // band kernel: log2 of the consecutive items a workgroup takes per visit (-1 = auto)
    int band_cap = 0;        // entries per LDS stage of the band kernel: 0 = auto, BCAP (192), BCAP_MID (288)
    int seg_strips = 1;      // binned x binned counts of dense catalogues use the per-segment strip layouts
    int seg_min_run = yawhip_detail::SEG_STRIPS_MIN_RUN;  // mean run length of the lane side from which binned x binned counts use it
    int debug_no_hits = 0;   // diagnostics only: pre-filter threshold above 1 -> no pair survives (timing of the fast path)
    int auto_orient = 1;     // every job runs on the strip layouts of the orientation that suits its patches (0: the catalogues' sort axis)
    int64_t slab_budget = 1ll << 30;  // bytes of per-item partial sums (weighted calls) above which a job list is cut in two
    int band_grid_div = 0;   // band kernel on strip items: workgroups = potential items / this (the kernel loops over the rest);
                             // 0 = auto (make_plan: 8, 16 for per-bin items, 4 on clustered catalogues)
    int flush_log2 = 17;     // band kernel: stages between flushes of the 32-bit LDS counters = 2^flush_log2
    int spin_wait = 1;       // wait for a call's results by polling the stream for the first 2 ms, then block (0: block at once)
    int item_segments = 1;   // strip builder -> float32 band kernels: the item list in eight segments, one per XCD (append_items)
    int half_bands = 1;      // self counts on merged triple runs, one object per lane: diagonal jobs take every unordered pair once (x 2)
    int triple_runs = 1;     // float32 band kernels stream merged triple runs (k_merge_triples) when the partner strips are c - 1, c, c + 1
    int band_fp32 = 1;       // band kernel on strip layouts of unit vectors: float32 classification + exact float64 for the
                             // guard bands (k_count_band32); 0: every entry in float64 (k_count_band)
    double strip_width = 0.005;  // strip grid of newly uploaded catalogues (strip_grid units, ~17 arcmin); 0 = no strips
    int strip_grid = 1;          // strip grid of newly uploaded catalogues: 1 = uniform in latitude (radians), 0 = linear in v (chord units)
    int band_trim = 1;           // strip builder and float32 band kernels trim u-windows and bands to the reachable caps (sep_angle)
    int default_kernel = YAWHIP_KERNEL_AUTO;
    int hist_chunk_log2 = 23;    // yawhip_redshift_histogram: objects per upload = 2^hist_chunk_log2
    int lds_limit = 160 * 1024;
    int n_cu = 256;
    yawhip_detail::DevBuf<unsigned long long> d_jobwork;
    yawhip_detail::DevBuf<double> d_full;          // yawhip_count_pairs_rows_device: the full result tensor of a sharded count
    yawhip_detail::DevBuf<int32_t> d_rowidx;
    // A context made by yawhip_ctx_create_multi owns one further context per additional device: catalogues are
    // replicated on all of them and yawhip_count_pairs splits its job list over them.
    std::vector<yawhip_ctx *> peers;
    struct Plan {  // job partition of the last multi-device call (a function of its inputs only)
        yawhip_detail::CallKey key;
        std::vector<std::vector<int32_t>> parts;  // job indices per device
    } plan;
    yawsort::Workspace sort_ws;  // upload-side sorts
    yawpix::Workspace pix_ws;    // yawhip_healpix_map, yawhip_healpix_pixels
    yawhip_detail::CallBufs parked[yawhip_detail::MAX_BATCH];  // the slots that are not active (the active one's entry is empty)
    int slot = 0;
    uint64_t opt_gen = 1;        // bumped by every accepted yawhip_ctx_set_option: plans and the partition are keyed on it
    uint64_t plan_clock = 0;     // least-recently-used stamp of the plans
    std::vector<yawhip_detail::HostPlan *> plans;
};

struct yawhip_catalog {
    yawhip_ctx *ctx = nullptr;
    uint64_t uid = 0;  // upload id, never reused (plans are keyed on it, not on the address)
    int64_t n = 0;
    int32_t n_patches = 0, nb = 1;
    yawhip_detail::DevPtr<double> x, y, z, w;  // w may be null
    yawhip_detail::DevPtr<int64_t> off;
    std::vector<int64_t> h_off;
    int64_t device_bytes = 0;
    bool unit_norm = true;  // every |a|^2 within UNIT_NORM_TOL of 1 (precondition of the FP32 pre-filter)
    int axis = 2;           // coordinate the segments are sorted by (0 = x, 1 = y, 2 = z)
    // strip layouts: the objects of every *group* cut into strips of a global grid along a second axis; inside a
    // (group, strip) run sorted along the sort axis. Partner runs of two catalogues are those whose grid indices
    // differ by at most sqrt(t_max) / spacing + 1.
    //   strips: group = patch, all redshift bins together, bin id per object (cross-correlation counts);
    //   seg:    group = (patch, bin) segment (binned x binned counts of dense catalogues; binned catalogues only).
    // One layout per orientation o = sort axis u (strips along (o + 2) % 3), built when a job first needs it (the one of
    // the catalogue's own sort axis at upload): see DevTab.
    yawhip_detail::StripLayout strips[3], seg[3];
    std::vector<yawhip_catalog *> replicas;  // copies on ctx->peers (multi-device contexts), same order
    bool has_strips = false;          // strip layouts can be built (unit vectors, n > 0)
    double strip_width = 0.0;         // grid spacing (strip_grid units); 0 = one run per patch
    int strip_grid = 0;               // 1: grid index floor((latitude + pi/2) / spacing), 0: floor((v + 1) / spacing) (k_strip_index)
    std::vector<double> h_box;        // [P][6] bounding box of every patch: min x, y, z, max x, y, z (empty patch: +4 / -4)
};

namespace yawhip_detail {

// Make slot i the active set of per-call buffers (its events are created on first use).
inline hipError_t use_slot(yawhip_ctx *ctx, int i) {
    if (i != ctx->slot) {
        std::swap(static_cast<CallBufs &>(*ctx), ctx->parked[ctx->slot]);  // park the active one
        std::swap(static_cast<CallBufs &>(*ctx), ctx->parked[i]);          // activate slot i
        ctx->slot = i;
    }
    return ctx->make_events();
}

inline const double *key_of(const double *x, const double *y, const double *z, int axis) { return axis == 0 ? x : (axis == 1 ? y : z); }
inline CatView view_of(const yawhip_catalog *c) {
    return CatView{c->x, c->y, c->z, c->w, c->off, c->nb, key_of(c->x, c->y, c->z, c->axis), c->axis};
}

// What count_finish needs to know about a call count_enqueue has put on a context's stream.
struct CallState {
    std::chrono::steady_clock::time_point wall0;
    bool pending = false;          // something was enqueued (false: nothing to count, outputs are zero)
    int64_t n_out = 0;
    size_t o_ctr = 0, o_counts = 0, o_sums = 0;
    bool want_counts = false, want_sums = false, band_ran = false, run_unweighted = false, run_weighted = false;
    bool segmented = false;        // the item list was kept in segments: the kept items are the sum of the segment counters
    int64_t cand = 0, abytes = 0, n_pot = 0;
    int launches = 0, kernel = 0, mode = 0, n_orient = 0, band_variant = 0, merged_triples = 0;
    int32_t variant[2] = {0, 0};   // count kernel of the unweighted, weighted launch (variant_code)
    uint64_t seq = 0;              // what k_call_tail writes into the slot's pinned block when the call is done
    bool word_wait = true;         // the completion word ends the wait (false: the caller put more behind the tail -- stream or event)
    bool stamps = false;           // kernel_ms / count_ms from the device clock stamps (false: no builder ran -- events)
    bool cleaned = false;          // the tail zeroes all of [counters][counts]: the slot is clean once the call is done
    size_t zero_after = 0;         // ... and this many bytes from the start of the block are zero then
};

// Row r of a call's result `in` (nullptr: zeros) into row at[r] of `out` (at == nullptr: row r), rows of `row` values;
// out == nullptr: not asked for.
template <typename T>
void place_rows(T *out, const T *in, int64_t n_rows, int64_t row, const int32_t *at = nullptr) {
    if (!out) return;
    if (!at) {  // contiguous: one piece
        row *= n_rows;
        n_rows = 1;
    }
    for (int64_t r = 0; r < n_rows; ++r) {
        T *dst = out + (size_t)(at ? at[r] : 0) * (size_t)row;
        if (in) memcpy(dst, in + (size_t)r * row, sizeof(T) * (size_t)row);
        else memset(dst, 0, sizeof(T) * (size_t)row);
    }
}

// ---- yawhip_count.hip: the count call
int check_call(const yawhip_ctx *ctx, const CountArgs &a);
int check_band_cap(int64_t value);
void drop_plans(yawhip_ctx *ctx, const yawhip_catalog *c);  // (defined with HostPlan)
int count_enqueue(yawhip_ctx *ctx, const CountArgs &a, bool want_counts, bool want_sums, int64_t *job_work, CallState &cs,
                  bool fetch_results = true);
int count_finish(yawhip_ctx *ctx, const CallState &cs, int64_t *fine_counts, double *fine_sums, yawhip_stats *stats,
                 const int32_t *row_index = nullptr, int64_t row_len = 0, bool wait_done = false);
void add_stats(yawhip_stats &total, const yawhip_stats &part, bool side_by_side);
int run_single(yawhip_ctx *ctx, const CountArgs &a, int64_t *fine_counts, double *fine_sums, yawhip_stats *stats,
               const std::function<void()> *meanwhile = nullptr);
// ---- yawhip_ingest.hip: the layouts a count call builds on first use
int build_strip_layout(yawhip_ctx *ctx, yawhip_catalog *c, int o, bool seg);
int build_triples(yawhip_ctx *ctx, yawhip_catalog *c, int o, bool seg);

}  // namespace yawhip_detail

#pragma GCC visibility pop
#endif
