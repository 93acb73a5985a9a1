// yawhip.hip -- MI355X (gfx950 / CDNA4) angular pair counting: the DEVICE code around the count kernels of a count call -- the
// item builders, the reductions and the tail -- the functions that launch it, and launch_count, which hands a launch to the
// unit of its kernel family. The kernel units decide nothing: the count call of yawhip_count.hip plans a call (kernel,
// layouts, tile and stage sizes, tables) and hands every launch one record, CountLaunch, whose selectors name the variant to
// run; csrc/yawhip_count_kernels.h declares that interface with the geometry and the counter-block layout. No entry point of
// include/yawhip.h lives in a kernel unit, and experiment flags and variant builds (build.KERNEL_UNITS,
// tools/build_variant.py) recompile the kernel units alone. They are one translation unit per kernel family -- the families
// share no kernel code, and a unit compiles in a fraction of the time all of them took together:
//   yawhip.hip                    this one: k_build_items(_strips), k_item_work, k_reduce_chunks / _slots, k_counts_to_double,
//                                 k_call_tail, their launchers, launch_count;
//   yawhip_kernel_plain.hip       k_count (EXACT / FILTER, non-unit input): 256-thread workgroups, 256*R lane objects in
//                                 registers, the c1 segment streamed through LDS; 8 FP64 ops + compare per pair, or a
//                                 conservative FP32 dot-product test first and exact FP64 for its survivors. Per-lane private
//                                 LDS histograms, fixed-order reduction;
//   yawhip_kernel_lean.hip        k_count_merged(_occ8) (SWEEP): single-wave workgroups, float32 only on chip (packed
//                                 v_pk_fma_f32), survivors queued per wave and evaluated 64 at a time in exact FP64; one item
//                                 of the cross-correlation path covers all redshift bins. AUTO uses it on layouts without strips;
//   yawhip_kernel_band64.hip      k_count_band: the band walk with every entry in FP64;
//   yawhip_kernel_band32.hip      k_count_band32 and k_count_band32_one, both from csrc/yawhip_band32.inc (BAND, what AUTO runs
//   yawhip_kernel_band32_one.hip  on strip layouts of unit vectors -- the headline): single-wave workgroups, the window of a
//                                 lane tile staged in LDS by LDS-DMA from float32 images of the columns, every lane walks
//                                 only the band |du| <= r of its objects, classifies every entry in float32 against guard
//                                 bands around the edges and decides the few inside a guard band with the exact FP64
//                                 predicate on the float64 columns (results identical to an all-float64 evaluation). The
//                                 streamed side is read from merged runs of three neighbouring strips (k_merge_triples,
//                                 yawhip_ingest.hip) where such a window fits the stage;
//   yawhip_kernel_fine.hip        k_count_band32_fine: the same for fine radial grids (separation weights);
//   yawhip_count_device.h         what more than one of these uses: device helpers, pick / launch.
// The rest of the library:
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
//   * a count kernel of one of the families above evaluates the items.
// Unweighted counts: uint32 LDS histograms -> 64-bit integer atomics. Weighted sums: per-item slabs (LDS float64
// atomics private to one wave) reduced in a fixed two-level order -> bit-reproducible run to run. No floating
// point atomics in global memory.
// Build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off (see yet_another_wizz_amd/build.py).

#include "yawhip_count_device.h"

namespace {
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
        const gf64p key1d = tab_key(c1);
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
        // (the tile's record brings the keys of its first and last object along: no look-up in the lane side's key column)
        const __attribute__((address_space(1))) TileRec *trp = (const __attribute__((address_space(1))) TileRec *)(c2.tile_rec + (jr.t_lo + tl));
        const struct { int64_t a0; int32_t na, run; double klo, khi; } tr = {trp->a0, trp->na, trp->run, trp->klo, trp->khi};
        const int64_t r2 = tr.run, a0 = tr.a0;
        const double kpad = triple ? 1.2e-7 : 0.0;  // float32 rounding of a streamed key (|u| <= 1: 2^-24)
        // (half bands: no lane of the tile looks at an entry in front of the tile's first object -- the window starts there)
        // cap_s > 0 (band_trim): the window is trimmed to the caps the tile's first and last objects can reach (sep_angle)
        double wlo = tr.klo - (it.pad_ ? 0.0 : rwin) - kpad, whi = tr.khi + rwin + kpad;
        if (cap_s > 0.0) {
            if (!it.pad_) wlo = cap_lo64(tr.klo, cap_c, cap_s) - kpad;
            whi = cap_hi64(tr.khi, cap_c, cap_s) + kpad;
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
            // The head of the run's record says where the run begins, whether it has entries and between which keys they
            // lie, in one round of loads (the offsets, the two keys behind them and inv were three rounds from three tables).
            // four partner runs in five lie entirely before or behind the tile's window (neighbouring patches share a
            // boundary only): the head settles those
            // (loads under their condition: the texture path is what this kernel is bound by, and it charges the lanes of a
            // load that are switched on; a wave whose tiles face no live run skips them altogether)
            const __attribute__((address_space(1))) RunGrid *rg = (const __attribute__((address_space(1))) RunGrid *)(c1.grid + r1);
            int64_t b0 = 0;
            uint32_t n1 = 0;
            double kfirst = 0.0, klast = 0.0, inv = 0.0;
            if (valid) { b0 = rg->b0; kfirst = rg->first; klast = rg->last; inv = rg->inv; n1 = rg->n; }
            const bool some = n1 > 0;
            const bool live = some && !(klast < wlo || kfirst > whi);
            // the run's index along the sort axis narrows both searches to one cell (RunGrid)
            uint32_t l0 = 0, l1 = 0, u0 = 0, u1 = 0;
            if (live) {
                const int cl = run_cell(wlo, kfirst, inv), cu = run_cell(whi, kfirst, inv);
                l0 = rg->g[cl]; l1 = rg->g[cl + 1]; u0 = rg->g[cu]; u1 = rg->g[cu + 1];
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

}  // namespace

namespace yawhip_detail {  // the launch interface (declared in yawhip_count_kernels.h)

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

// The count kernel of a call: each family's launcher picks the variant from the selectors of the launch record, in its own unit.
hipError_t launch_count(const CountLaunch &L, bool weighted, int32_t *variant) {
    switch (L.family) {
    case CountFamily::BAND32: return L.one_chunk ? launch_band32_one(L, weighted, variant) : launch_band32(L, weighted, variant);
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
