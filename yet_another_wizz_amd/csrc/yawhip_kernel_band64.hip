// yawhip_kernel_band64.hip -- k_count_band (BAND, every entry in float64): the band walk on float64 columns staged by LDS-DMA.
// One of the kernel units of the count call; yawhip.hip has the map.
#include "yawhip_count_device.h"

namespace {
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

}  // namespace

namespace yawhip_detail {

int band_lds_fixed(int cap) { return cap == BCAP_MID ? BandLds<BCAP_MID>::FIXED : BandLds<BCAP>::FIXED; }

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

}  // namespace yawhip_detail
