// yawhip.hip -- MI355X (gfx950 / CDNA4) angular pair counting: the DEVICE code of the count call -- the item builders, the
// count kernels, the reductions and the tail -- and the launch layer that puts them on a stream. This unit decides nothing:
// the count call of yawhip_count.hip plans a call (kernel, layouts, tile and stage sizes, tables) and hands every launch one
// record, CountLaunch, whose selectors name the variant to run; csrc/yawhip_count_kernels.h declares that interface with the
// geometry and the counter-block layout the two units share. No entry point of include/yawhip.h lives here, and experiment
// flags and variant builds (build.KERNEL_UNIT, tools/build_variant.py) recompile this unit alone. The rest of the library:
//   yawhip_count.hip    the count call: plans, count_enqueue / count_finish / run_single, yawhip_count_pairs, yawhip_job_work;
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
#include <cstdint>
#include <type_traits>
#include <utility>

#include "yawhip_count_kernels.h"

using namespace yawhip_detail;

namespace {
constexpr int COUNT_FLUSH_MASK = (1 << 13) - 1;  // k_count: stages between flushes of the 32-bit LDS counters (see there)
constexpr int MERGED_FLUSH_MASK = (1 << 16) - 1; // k_count_merged: 256 lane objects x 64 streamed objects per stage
constexpr double PAD_COORD = 4.0;  // padded lanes sit >= 3 away from any unit vector: s >= 9 > max t = 4

struct alignas(16) Obj {  // one streamed object in LDS: two 16-byte broadcast reads
    double x, y, z, w;
};

struct alignas(16) ObjF {  // its float32 image for the pre-filter: one 16-byte broadcast read
    float x, y, z, pad;
};

// ------------------------------------------------------------------------------------------------
// Spherical caps: the u-range the partners of an object with key u can have, [u c - sqrt(1 - u^2) s, u c + sqrt(1 - u^2) s]
// with c, s = cos, sin of the largest separation angle (sep_angle, yawhip_count_kernels.h: the derivation is there).
// The bounds are culling bounds only: classification and the exact float64 path do not see them.
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
// A clock stamp of the call (CTR_T_*, yawhip_count_kernels.h), by the first thread of a kernel
__device__ __forceinline__ void stamp_start(unsigned long long *__restrict__ counters, int word) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[word] = wall_clock64();
}
// Append the kept items of a builder workgroup to the item list and add its evaluated-pair total: ONE atomic
// per workgroup on each of the two counters. (They are single hot addresses -- with an atomic per wave the
// builders spent three quarters of their time queueing on them.) Order of the list is irrelevant.
// seg_cap > 0: the list is kept in ITEM_SEGS segments of seg_cap records, workgroup b appends to segment b % ITEM_SEGS and
// counts in that segment's own counter (ITEM_SEG_CTR): eight addresses take the atomics of a launch side by side (on one
// address the 1200 appends of the headline queue for 10 of the builder's 43 us), and a segment -- every eighth builder
// workgroup's tiles -- is the same mix of dense and sparse items as the whole list: the float32 band kernels give XCD x
// segment x.
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
            s_base = total ? atomicAdd(&counters[CTR_KEPT], (unsigned long long)total) : 0ull;
        }
        if (wsum) atomicAdd(&counters[TILE_PAIR_CTR(blockIdx.x & (EVAL_SLOTS - 1))], wsum);  // statistics, spread like the other totals
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
        if (pot == 0) counters[CTR_KEPT] = (unsigned long long)n_pot;
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
    if (ticket >= counters[CTR_KEPT]) return;  // never taken when the host sized the grid from the builder's count
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

    const unsigned long long n_kept = counters[CTR_KEPT];
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
        if (lane == 0 && nev) atomicAdd(&counters[BAND_ENTRY_CTR(ticket & (EVAL_SLOTS - 1))], (unsigned long long)nev);
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
    const unsigned long long n_kept = counters[CTR_KEPT];
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
                                                                    counters + EXACT_EVAL_CTR(0) + CTR_SLOT_WORDS * (ticket & (EVAL_SLOTS - 1)));
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
        if (lane == 63 && nev) atomicAdd(&counters[BAND_ENTRY_CTR(ticket & (EVAL_SLOTS - 1))], (unsigned long long)nev);
    }
}

// Evaluated pairs per job (na * nb of the job's kept items): the cost the host balances over GPUs.
__global__ void k_item_work(const Item *__restrict__ items, const unsigned long long *__restrict__ counters,
                            int slots_per_job, unsigned long long *__restrict__ job_work) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= counters[CTR_KEPT]) return;
    const Item it = items[i];
    unsigned long long streamed = 0;
    for (int w = 0; w < it.nwin; ++w) streamed += (unsigned long long)it.nb[w];
    atomicAdd(&job_work[item_slot(it) / slots_per_job], (unsigned long long)it.na * streamed);
}

// Weighted sums: every kept item left a slab of `slab` float64 values at partials[pot]. They are added per output
// slot in a fixed two-level order -- chunks of REDUCE_CHUNK consecutive potential items, then the chunks of a slot in
// order -- so the result is bit-reproducible and the reduction is parallel over (chunk, value). Dropped potential
// items (kept[pot] == 0, their slab is never written) are skipped; kept == nullptr means every item was kept.
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

// yawhip_stats.count_variant*: the family and template arguments of a count kernel (code layout: include/yawhip.h)
enum VariantFamily : int32_t { VF_COUNT = 1, VF_MERGED, VF_MERGED_OCC8, VF_BAND, VF_BAND32, VF_BAND32_ONE, VF_BAND32_FINE };
constexpr int32_t variant_code(int32_t family, int R, int cap, bool weighted, int ne = 0, bool merged = false, bool uni = false,
                               bool priv = false, bool filter = false, bool nf1 = false) {
    return family | R << 4 | cap << 8 | (int32_t)weighted << 18 | ne << 19 | (int32_t)merged << 22 | (int32_t)uni << 23 |
           (int32_t)priv << 24 | (int32_t)filter << 25 | (int32_t)nf1 << 26;
}

}  // namespace

namespace yawhip_detail {  // the launch interface (declared in yawhip_count_kernels.h)

int band_lds_fixed(int cap) { return cap == BCAP_MID ? BandLds<BCAP_MID>::FIXED : BandLds<BCAP>::FIXED; }
size_t count_lds(bool weighted, bool priv, int n_edges) {
    return 2 * STAGE * (sizeof(Obj) + sizeof(ObjF)) + (size_t)((n_edges + 1) & ~1) * sizeof(double) +
           (size_t)(n_edges - 1) * (priv ? WG : 1) * (weighted ? 8 : 4);
}
size_t merged_stage_lds() { return 2 * MSTAGE * sizeof(ObjF); }
size_t merged_lds(bool weighted, int bins, int n_edges) {
    return merged_stage_lds() + (size_t)bins * n_edges * sizeof(double) + (size_t)bins * (n_edges - 1) * (weighted ? 8 * (MWG / 64) : 4) +
           (size_t)bins * sizeof(float) + (size_t)MWG * sizeof(unsigned int) + 16;
}

hipError_t launch_build_strips(const CountLaunch &L) {
    hipLaunchKernelGGL(k_build_items_strips, dim3(L.build_grid), dim3(L.build_wg), 0, L.stream, L.d_tabs,
                       reinterpret_cast<const JobRec *>(L.d_jobs), L.d_prefix, (int)L.n_build_jobs,
                       L.triple ? 0 : L.reach, (int)L.tile, L.rwin_max, L.cap_c, L.cap_s, L.swap ? 1 : 0, L.triple ? 1 : 0,
                       L.n_pot, L.d_items, L.d_ctr, L.d_kept, L.seg_cap);
    return hipGetLastError();
}
hipError_t launch_build_windows(const CountLaunch &L) {
    hipLaunchKernelGGL(k_build_items<true>, dim3(L.build_grid), dim3(L.build_wg), 0, L.stream, L.c1, L.c2,
                       L.d_jobs, L.d_prefix, (int)L.n_build_jobs, L.n_bins, (int)L.tile,
                       L.d_rwin, L.n_pot, L.d_items, L.d_ctr, L.d_kept);
    return hipGetLastError();
}
hipError_t launch_build_whole(const CountLaunch &L) {
    hipLaunchKernelGGL(k_build_items<false>, dim3(L.build_grid), dim3(L.build_wg), 0, L.stream, L.c1, L.c2,
                       L.d_jobs, L.d_prefix, (int)L.n_build_jobs, L.n_bins, (int)L.tile, L.d_rwin, L.n_pot,
                       L.d_items, L.d_ctr, nullptr);
    return hipGetLastError();
}
hipError_t launch_item_work(const CountLaunch &L, int slots_per_job, unsigned long long *job_work) {
    hipLaunchKernelGGL(k_item_work, dim3((unsigned)((L.n_pot + 255) / 256)), dim3(256), 0, L.stream, L.d_items,
                       L.d_ctr, slots_per_job, job_work);
    return hipGetLastError();
}

// two-level ordered reduction of the weighted slabs, per output slot; prefix = first potential item of every output slot,
// chunk prefix = first chunk of every output slot
hipError_t launch_reduce_chunks(const CountLaunch &L) {
    const int thr = 256;
    hipLaunchKernelGGL(k_reduce_chunks, dim3((unsigned)((L.n_chunks * L.slab + thr - 1) / thr)), dim3(thr), 0, L.stream,
                       L.d_partials, L.d_kept, L.d_prefix, L.d_cprefix,
                       (int)L.n_oslots, (int)L.slab, L.d_chunk_sums, L.d_ctr);
    return hipGetLastError();
}
hipError_t launch_reduce_slots(const CountLaunch &L) {
    const int thr = 256;
    hipLaunchKernelGGL(k_reduce_slots, dim3((unsigned)((L.n_oslots * L.slab + thr - 1) / thr)), dim3(thr), 0, L.stream,
                       L.d_chunk_sums, L.d_cprefix, (int)L.n_oslots, (int)L.slab, L.d_sums,
                       L.n_chunks > 0 ? nullptr : L.d_ctr);
    return hipGetLastError();
}
}  // namespace yawhip_detail

namespace {

// The count kernels. Their variants are picked from the selectors of the launch record (pick; each list runs from the last
// variant to the first: the compiler lays the kernels out in the reverse order, which keeps the code object as it was).
// The variants named in these lists are the ones compiled.
// Band kernels: grid from the number of POTENTIAL items (known on the host); the kernel reads the number the builder kept
// from the device counter, workgroups beyond it exit, workgroups loop if more were kept than the grid holds.
hipError_t launch_band32(const CountLaunch &L, bool wgt, int32_t *variant) {
    const std::pair<int, int> stage{L.R, L.cap};
    const std::pair<bool, bool> rows{L.merged, L.uni};
    const dim3 band_grid(L.band_grid), wave(64);
    return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
        return pick<Int<4>, Int<3>, Int<2>>(L.n_edges, [&](auto ne) {
            return pick<Rows<true, false>, Rows<true, true>, Rows<false, true>>(rows, [&](auto r) {
                return pick<Stage<4, B32_CAP_BIG>, Stage<2, B32_CAP_BIG>, Stage<2, B32_CAP>, Stage<1, B32_CAP>>(stage, [&](auto s) {
                    using S = decltype(s);
                    using M = decltype(r);
                    auto kern = L.one_chunk ? k_count_band32_one<S::R, S::CAP, w, ne, M::MERGED, M::UNI>
                                            : k_count_band32<S::R, S::CAP, w, ne, M::MERGED, M::UNI>;
                    *variant = variant_code(L.one_chunk ? VF_BAND32_ONE : VF_BAND32, S::R, S::CAP, w, ne, M::MERGED, M::UNI);
                    return launch(kern, band_grid, wave, L.lds, L.stream, L.d_tabs, L.d_items, L.n_bins, L.d_t,
                                  L.d_thr32, L.d_rwin, L.d_ucap, L.flush_mask, L.swap ? 1 : 0, L.d_counts,
                                  L.d_partials, L.d_ctr, L.seg_cap);
                });
            });
        });
    });
}
hipError_t launch_band64(const CountLaunch &L, bool wgt, int32_t *variant) {
    const std::pair<int, int> stage{L.R, L.cap};
    const std::pair<bool, bool> rows{L.merged, L.uni};
    const dim3 band_grid(L.band_grid), wave(64);
    return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
        return pick<Int<0>, Int<4>, Int<3>, Int<2>>(L.band_ne, [&](auto ne) {
            return pick<Rows<true, false>, Rows<true, true>, Rows<false, true>>(rows, [&](auto r) {
                return pick<Stage<4, BCAP_MID>, Stage<2, BCAP_MID>, Stage<2, BCAP>, Stage<1, BCAP>>(stage, [&](auto s) {
                    using S = decltype(s);
                    using M = decltype(r);
                    *variant = variant_code(VF_BAND, S::R, S::CAP, w, ne, M::MERGED, M::UNI);
                    return launch(k_count_band<S::R, S::CAP, w, ne, M::MERGED, M::UNI>, band_grid, wave, L.lds, L.stream,
                                  L.d_tabs, L.d_items, L.n_bins, L.n_edges, L.d_t, L.d_rwin, L.flush_mask,
                                  L.hp_shift, w ? 0 : L.batch_log2, L.d_counts, L.d_partials, L.d_ctr);
                });
            });
        });
    });
}
hipError_t launch_fine(const CountLaunch &L, bool wgt, int32_t *variant) {
    const std::pair<int, int> stage{L.R, L.cap};
    const std::pair<bool, bool> rows{L.merged, L.uni};
    const dim3 band_grid(L.band_grid), wave(64);
    return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
        return pick<Rows<true, false>, Rows<true, true>, Rows<false, false>, Rows<false, true>>(rows, [&](auto r) {
            return pick<Stage<4, BCAP_MID>, Stage<2, BCAP_MID>, Stage<2, BCAP>, Stage<1, BCAP>>(stage, [&](auto s) {
                using S = decltype(s);
                using M = decltype(r);
                *variant = variant_code(VF_BAND32_FINE, S::R, S::CAP, w, 0, M::MERGED, M::UNI);
                return launch(k_count_band32_fine<S::R, S::CAP, w, M::MERGED, M::UNI>, band_grid, wave, L.lds, L.stream,
                              L.d_tabs, L.d_items, L.n_bins, L.n_edges, L.d_t, L.d_thr32, L.d_rwin,
                              L.d_ucap, L.flush_mask, L.swap ? 1 : 0, L.d_counts, L.d_partials, L.d_ctr, L.seg_cap);
            });
        });
    });
}
// The lean kernel (k_count_merged / _occ8) and k_count, one workgroup per item: grids in pieces of at most 2^32 - 1
// work-items per launch dimension.
template <typename F>
hipError_t in_pieces(int64_t n_items, int wg, F &&launch_at) {
    const int64_t max_grid = (1ll << 31) / wg;
    for (int64_t base = 0; base < n_items; base += max_grid) {
        const hipError_t e = launch_at(dim3((unsigned)std::min(max_grid, n_items - base)), base);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t launch_lean(const CountLaunch &L, bool wgt, int32_t *variant) {
    return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
        return pick<Bool<false>, Bool<true>>(L.nf1, [&](auto nf1) {
            return pick<Bool<false>, Bool<true>>(L.merged, [&](auto m) {
                return pick<Int<4>, Int<2>, Int<1>>(L.R, [&](auto r) {
                    *variant = variant_code(r <= 2 ? VF_MERGED_OCC8 : VF_MERGED,  // (the choice of pick_count_merged)
                                            r, 0, w, 0, m, false, false, false, nf1);
                    return in_pieces(L.n_items, MWG, [&](dim3 g, int64_t base) {
                        return launch(pick_count_merged<r, w, nf1, m>(), g, dim3(MWG), L.lds, L.stream, L.d_tabs,
                                      L.d_items, L.n_bins, L.n_edges, L.d_t, L.d_dthr, L.d_rwin, base,
                                      L.d_counts, L.d_partials, L.d_ctr);
                    });
                });
            });
        });
    });
}
hipError_t launch_plain(const CountLaunch &L, bool wgt, int32_t *variant) {
    return pick<Bool<true>, Bool<false>>(wgt, [&](auto w) {
        return pick<Bool<false>, Bool<true>>(L.priv, [&](auto pv) {
            return pick<Bool<false>, Bool<true>>(L.filter, [&](auto f) {
                return pick<Int<4>, Int<2>, Int<1>>(L.R, [&](auto r) {
                    *variant = variant_code(VF_COUNT, r, 0, w, 0, false, false, pv, f);
                    return in_pieces(L.n_items, WG, [&](dim3 g, int64_t base) {
                        return launch(k_count<r, w, pv, f>, g, dim3(WG), L.lds, L.stream, L.c1, L.c2,
                                      L.d_items, L.n_bins, L.n_edges, L.d_t, L.d_dthr, base, L.d_counts,
                                      L.d_partials, L.d_ctr);
                    });
                });
            });
        });
    });
}

}  // namespace

namespace yawhip_detail {

hipError_t launch_count(const CountLaunch &L, bool weighted, int32_t *variant) {
    switch (L.family) {
    case CountFamily::BAND32: return launch_band32(L, weighted, variant);
    case CountFamily::BAND32_FINE: return launch_fine(L, weighted, variant);
    case CountFamily::BAND64: return launch_band64(L, weighted, variant);
    case CountFamily::LEAN: return launch_lean(L, weighted, variant);
    case CountFamily::PLAIN: return launch_plain(L, weighted, variant);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_counts_to_double(const CountLaunch &L, int64_t n_out) {
    const int thr = 256;
    hipLaunchKernelGGL(k_counts_to_double, dim3((unsigned)((n_out + thr - 1) / thr)), dim3(thr), 0, L.stream,
                       L.d_counts, L.d_sums, n_out, L.d_ctr);
    return hipGetLastError();
}
hipError_t launch_call_tail(hipStream_t stream, unsigned char *dev, unsigned char *host, unsigned n_copy, unsigned n_clean,
                            unsigned long long seq) {
    hipLaunchKernelGGL(k_call_tail, dim3(std::min((n_copy + TAIL_WG - 1) / TAIL_WG, TAIL_MAX_GRID)), dim3(TAIL_WG), 0, stream,
                       reinterpret_cast<uint4 *>(dev), reinterpret_cast<uint4 *>(host), n_copy, n_clean, seq);
    return hipGetLastError();
}

}  // namespace yawhip_detail
