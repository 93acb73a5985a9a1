// k_count_band32 (float32 band kernel, DESIGN.md section 4) and its launcher, included once per number of chunks a round can
// stage -- by yawhip_kernel_band32.hip with YAW_B32_CH = 3 as k_count_band32 / launch_band32 (up to three windows, or pieces of
// one, in a round), by yawhip_kernel_band32_one.hip with YAW_B32_CH = 1 as k_count_band32_one / launch_band32_one, for calls whose
// items all have one window (merged triple runs, items of k_build_items): the bookkeeping of two more chunks costs scalar
// registers (spilled) and instructions per item, 0.283 against 0.274 ms at the headline. The chunk count is a macro of two
// inclusions rather than a template parameter because hipcc 7.2 emits no host stubs for this kernel as soon as a template
// parameter sizes its chunk arrays; and the two are two translation units because together they are 60 % of the library's
// device instructions. Not a translation unit of its own: the including unit names the kernel (YAW_B32_NAME), the launcher
// (YAW_B32_LAUNCH) and the chunks (YAW_B32_CH) and has included yawhip_count_device.h.
namespace {

// ------------------------------------------------------------------------------------------------
// Band kernel, float32 classification (BAND on strip layouts of unit vectors; DESIGN.md section 4).
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

template <int R, int CAP, bool WEIGHTED, int NE, bool MERGED, bool UNI>
__global__ __launch_bounds__(64, band32_min_waves(R, CAP, WEIGHTED, NE, UNI))
void YAW_B32_NAME(const DevTab *__restrict__ tabs, const Item *__restrict__ items, int n_bins,
                  const double *__restrict__ t, const float *__restrict__ thr32,
                  const double *__restrict__ rwin_k, const float *__restrict__ ucap,
                  unsigned flush_mask, int swap,
                  unsigned long long *__restrict__ out_counts,
                  double *__restrict__ partials,
                  unsigned long long *__restrict__ counters, unsigned long long seg_cap) {
    static_assert(NE >= 2 && NE <= 4, "edges per bin");
    constexpr int CH = YAW_B32_CH;  // chunks per round (see the head of this file)
    // One object per lane (sparse per-bin runs) in the one-chunk kernel: two ENTRIES per trip of the walk, see classify_entry.
    // (A chunk is then followed by two sentinel entries; with several chunks in a stage the second would be the next chunk's first.)
    constexpr bool PAIRS = R == 1 && CH == 1;
    constexpr int NS = PAIRS ? 2 : R;  // evaluations per trip
    static_assert(CH == 1 || CH == 3, "chunks per round");
    static_assert(CAP % 4 == 0, "stage capacity");
    using HistT = typename std::conditional<WEIGHTED, double, unsigned int>::type;
    constexpr int NC = NE == 2 ? 1 : NE;     // counters per lane object: hits of the annulus, or s <= t_e per edge
    constexpr int NF = NE - 1;               // fine bins per redshift bin
    constexpr int TW = thr32_width(NE);
    constexpr bool LANE_THR = MERGED && !UNI;  // every lane object has the edge row of its own bin
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_dyn[];
    const int nkb = MERGED ? n_bins : 1;
    const int nslots = nkb * NF;
    unsigned char *p = lds_dyn;
    // The plain one-annulus count with two objects per lane and one threshold row has its trip spelled out (classify_two_objects);
    // in the one-chunk kernel it also walks its bands DOWNWARDS, from entry hi - 1, so that one saturating subtraction is both
    // the advance and the clamp of the entry address: below the chunk lie LEAD sentinel entries, the first at LDS address 0.
    constexpr bool SLOT_TRIP = NE == 2 && !WEIGHTED && R == 2 && !LANE_THR;
    constexpr bool DOWN = SLOT_TRIP && CH == 1;
    constexpr int LEAD = DOWN ? 4 : 0;  // (four entries: the chunk keeps the 16-byte alignment the LDS-DMA needs; band32_lds has the 48 bytes)
    constexpr unsigned COLB = (CAP + 4 + LEAD) * 4;  // bytes of one staged float32 column
    float *const stage_lead = reinterpret_cast<float *>(p);
    float *stage = stage_lead + LEAD; p += (size_t)3 * COLB;  // columns x, y, z
    double *sw = reinterpret_cast<double *>(p); if (WEIGHTED) p += (size_t)(CAP + 4) * 8;
    HistT *hist = reinterpret_cast<HistT *>(p); p += (size_t)nslots * sizeof(HistT);
    p = reinterpret_cast<unsigned char *>(((size_t)p + 15) & ~(size_t)15);
    float *sthr = reinterpret_cast<float *>(p);  // [n_bins][TW] when LANE_THR
    const int lane = threadIdx.x;
    const unsigned a_stage = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(stage);
    const unsigned a_sw = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(sw);
    const unsigned a_hist = (unsigned)(size_t)(lds_byte *)reinterpret_cast<unsigned char *>(hist);

    const TicketMap tmap = ticket_map(counters, seg_cap);
    const unsigned long long n_kept = tmap.n_kept;
    for (int e = lane; e < nslots; e += 64) hist[e] = HistT(0);  // every flush leaves the histogram zeroed again
    if constexpr (DOWN) {
        if (a_stage != 4u * LEAD) __builtin_trap();  // (the dynamic LDS starts at address 0: nothing is declared in front of it)
        if (lane < LEAD) { stage_lead[lane] = PAD_COORD32; stage_lead[COLB / 4 + lane] = PAD_COORD32; stage_lead[2 * (COLB / 4) + lane] = PAD_COORD32; }
    }
    if (LANE_THR)
        for (int e = lane; e < n_bins * TW; e += 64) sthr[e] = thr32[e];
    unsigned round_no = 0;
    // statistics: the band entries the lanes walked, summed per lane over the workgroup's items and sent once -- only the sum
    // over the launch is read. (DPP: the shuffle form is six trips through the LDS crossbar. The halves of the lane sums are
    // reduced separately: 64 x 65535 fits a word.)
    unsigned int nev = 0;
    auto send_entries = [&](unsigned int lane_sum) {
        const unsigned int lo16 = wave_sum_lane63(lane_sum & 0xffffu), hi16 = wave_sum_lane63(lane_sum >> 16);
        const unsigned long long sum = (unsigned long long)lo16 + ((unsigned long long)hi16 << 16);
        if (lane == 63 && sum) atomicAdd(&counters[BAND_ENTRY_CTR(blockIdx.x & (EVAL_SLOTS - 1))], sum);
    };
    for (unsigned long long v = blockIdx.x;; v += gridDim.x) {
        if ((v >> 3) >= tmap.per_xcd) break;
        const unsigned long long ticket = tmap.ticket(v);
        if (ticket >= n_kept) continue;  // beyond the last block's end
        const Item it = items[ticket];
        const int o = item_orient(it), islot = item_slot(it);
        const DevTab cl = tabs[swap ? o : 3 + o], cs = tabs[swap ? 3 + o : o];  // lane side, streamed side
        const int kfix = MERGED ? 0 : islot % n_bins;
        // half width of the u-window in float32: sqrt(t_max) widened by the rounding of both keys and of the subtraction
        const float rwin = (float)(rwin_k[kfix] * 1.000001 + 4e-7);

        // The windows of an item are staged in ROUNDS: as many whole windows as fit the stage together (all three of a
        // typical item: one wait for the LDS-DMA instead of three, and the band searches of the windows run in lockstep);
        // a window longer than the stage goes through it alone, CAP - 4 entries at a time. A chunk = (first streamed
        // object, entries, first entry of the stage it occupies); every chunk is followed by its own sentinel entry.
        int win = 0;            // next window of the item
        int64_t win_off = 0;    // entries of it already staged
        int64_t cb[CH];
        int cn[CH], co[CH];
        int nch = 0;
        auto next_round = [&]() {
            nch = 0;
            int used = 0;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                cb[c] = 0; cn[c] = 0; co[c] = 0;
                if (win < it.nwin && nch == c) {
                    const int64_t wb = win == 0 ? it.b0[0] : (win == 1 ? it.b0[1] : it.b0[2]);
                    const int64_t rem = (int64_t)(win == 0 ? it.nb[0] : (win == 1 ? it.nb[1] : it.nb[2])) - win_off;
                    if (rem + 1 <= (int64_t)(CAP - used)) {           // the rest of the window and its sentinel fit
                        cb[c] = wb + win_off; cn[c] = (int)rem; co[c] = used;
                        used += ((int)rem + 1 + 3) & ~3;
                        ++win; win_off = 0; ++nch;
                    } else if (c == 0) {                               // alone in the stage, a piece at a time
                        cb[c] = wb + win_off; cn[c] = CAP - 4; co[c] = 0;
                        used = CAP;
                        win_off += CAP - 4; ++nch;
                    }
                }
            }
        };
        auto issue_round = [&]() {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (c < nch) {
                    // four entries of one column per lane and instruction (16 bytes; the last lane may run up to three entries
                    // past the chunk: into the next run of the catalogue, and into the chunk's padding in LDS)
                    const gf32p gx = cs.qx + cb[c], gy = cs.qy + cb[c], gz = cs.qz + cb[c];
                    const unsigned a_c = a_stage + ((unsigned)co[c] << 2);
#pragma unroll
                    for (int k = 0; k < (CAP + 255) / 256; ++k) {
                        const unsigned e = (unsigned)(k * 256 + 4 * lane);
                        if (e < (unsigned)cn[c]) {
                            __builtin_amdgcn_global_load_lds(gx + e, lds_ptr(a_c + k * 1024), 16, 0, 0);
                            __builtin_amdgcn_global_load_lds(gy + e, lds_ptr(a_c + COLB + k * 1024), 16, 0, 0);
                            __builtin_amdgcn_global_load_lds(gz + e, lds_ptr(a_c + 2 * COLB + k * 1024), 16, 0, 0);
                        }
                    }
                    if (WEIGHTED && cs.w) {
#pragma unroll
                        for (int k = 0; k < (CAP + 127) / 128; ++k) {
                            const unsigned e = (unsigned)(k * 128 + 2 * lane);
                            if (e < (unsigned)cn[c])
                                __builtin_amdgcn_global_load_lds(cs.w + cb[c] + e, lds_ptr(a_sw + ((unsigned)co[c] << 3) + k * 1024), 16, 0, 0);
                        }
                    }
                }
            }
        };
        __syncthreads();  // the previous item of this workgroup has left the LDS
        next_round();
        issue_round();
        // lane objects while the stage is in flight: R NEIGHBOURING objects of the u-sorted tile per lane
        f32x2 ax2[R / 2 > 0 ? R / 2 : 1], ay2[R / 2 > 0 ? R / 2 : 1], az2[R / 2 > 0 ? R / 2 : 1];  // packed pairs (R even)
        float ax[R], ay[R], az[R];
        int kb[R];
        double aw_own[R];  // weighted: the lane objects' own weights
        int lane_obj = lane;  // whose objects this lane counts for: its own, until the bands of a sparse item are shared out
        int n_own = (int)it.na - lane * R;
        n_own = n_own < 0 ? 0 : (n_own > R ? R : n_own);
        // One 16-byte record per object {x, y, z, bin} (DevTab::q4), fetched whether the lane has the object or not -- the table
        // ends with LANE_IMAGE_PAD records, a whole lane tile beyond the last object -- and padded in registers afterwards:
        // R loads in one round, no exec-masked blocks, instead of a dword load per object and column.
        lane_words rec[R];
        {
            const glanep lane_q = cl.q4 + it.a0 + lane * R;
#pragma unroll
            for (int r = 0; r < R; ++r) rec[r] = lane_q[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool have = r < n_own;
            const unsigned ic = have ? (unsigned)(lane * R + r) : 0u;
            ax[r] = have ? rec[r].x : PAD_COORD32;
            ay[r] = have ? rec[r].y : PAD_COORD32;
            az[r] = have ? rec[r].z : PAD_COORD32;
            kb[r] = MERGED ? (have ? __float_as_int(rec[r].w) : 0) : 0;
            // weighted: the object's own weight travels with its coordinates (one memory latency for both) instead of being
            // fetched at the flush, at the end of the item's chain of dependent latencies (config #4: DD 0.370 -> 0.349,
            // DR 1.67 -> 1.56, RR 3.20 -> 3.13 ms)
            if constexpr (WEIGHTED) aw_own[r] = (cl.w && have) ? (cl.w + it.a0)[ic] : 1.0;
        }
        // thresholds: per lane object (its bin's row from the LDS table) or one row for the wave
        float th[R][TW];
        {
            const float *row = LANE_THR ? nullptr : thr32 + (size_t)kfix * TW;  // uniform: scalar loads
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < TW; ++q) th[r][q] = LANE_THR ? sthr[kb[r] * TW + q] : row[q];
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
            // band_trim: the caps the lane's first and last objects can reach (sep_angle; lanes without an object walk nothing)
            const float cap_c = ucap[2 * kfix], cap_s = ucap[2 * kfix + 1];
            if (cap_s > 0.0f) {
                klo = cap_lo32(u_first, cap_c, cap_s);
                khi = cap_hi32(u_last, cap_c, cap_s);
            }
        }
        if constexpr (R >= 2) {
#pragma unroll
            for (int h = 0; h < R / 2; ++h) {
                ax2[h] = f32x2{ax[2 * h], ax[2 * h + 1]}; ay2[h] = f32x2{ay[2 * h], ay[2 * h + 1]}; az2[h] = f32x2{az[2 * h], az[2 * h + 1]};
            }
        }
        f32x2 nc2[R / 2 > 0 ? R / 2 : 1];  // one annulus: -c of the lane's objects, the addend of the first product
#pragma unroll
        for (int h = 0; h < R / 2; ++h) nc2[h] = f32x2{-th[2 * h][0], -th[2 * h + 1][0]};
        unsigned int cnt[R][NC];
        double acc[R][NC];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) { cnt[r][c] = 0u; acc[r][c] = 0.0; }
        // lane counters -> LDS histogram (cell = bin of the object x fine bin)
        // half bands (one object per lane, one chunk per round: the only variant that runs them): every pair was met once
        constexpr bool HALF = R == 1 && CH == 1;
        const double pair_mult = HALF && (it.pad_ & 1) ? 2.0 : 1.0;
        auto flush_lanes = [&]() {
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const unsigned cell = a_hist + (unsigned)((kb[r] * NF + f) * (int)sizeof(HistT));
                    if constexpr (WEIGHTED) {
                        const double vsum = NE == 2 ? acc[r][0] : acc[r][f + 1] - acc[r][f];
                        // float64 adds of ONE instruction that hit the same cell are serialised by the LDS in a fixed lane
                        // order; the histogram belongs to this wave alone -> reproducible sums
                        const double aw = aw_own[r];
                        if (vsum != 0.0)
                            (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) double *)(size_t)cell, HALF ? aw * vsum * pair_mult : aw * vsum,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        const unsigned int c = (NE == 2 ? cnt[r][0] : cnt[r][f + 1] - cnt[r][f]) << (HALF ? (it.pad_ & 1) : 0);
                        if (c)
                            (void)__hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned int *)(size_t)cell, c,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) { cnt[r][c] = 0u; acc[r][c] = 0.0; }
            }
        };
        auto flush_counts = [&]() {  // LDS histogram -> global result (unweighted)
            flush_lanes();
            __syncthreads();
            for (int idx = lane; idx < nslots; idx += 64) {
                const unsigned int c = (unsigned int)hist[idx];
                hist[idx] = HistT(0);
                if (c) atomicAdd(&out_counts[(int64_t)islot * nslots + idx], (unsigned long long)c);
            }
        };

        const bool single_window = it.nwin == 1 && it.nb[0] + 1 <= CAP;  // the item is this one chunk (its bands may be shared out, below)
        for (;; ++round_no) {
            // The round has landed: nothing but the issuing wave's own vmcnt orders an LDS read behind a pending LDS-DMA. The
            // wait is spelled out -- in a single-wave workgroup __syncthreads() is no barrier instruction, and on this loop's
            // back edge hipcc did not put a vmcnt wait in front of the LDS accesses by itself (counts came out wrong now and then).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (lane < nch) {  // a sentinel behind every chunk: beyond every edge of every lane object
                int at = co[0] + cn[0];
                if constexpr (CH > 1) at = lane == 0 ? at : (lane == 1 ? co[1] + cn[1] : co[CH - 1] + cn[CH - 1]);
                stage[at] = PAD_COORD32; stage[COLB / 4 + at] = PAD_COORD32; stage[2 * (COLB / 4) + at] = PAD_COORD32;
                if (WEIGHTED) sw[at] = 0.0;
                if constexpr (PAIRS) {  // (n <= CAP - 1: the stage has room for entry n + 1)
                    stage[at + 1] = PAD_COORD32; stage[COLB / 4 + at + 1] = PAD_COORD32; stage[2 * (COLB / 4) + at + 1] = PAD_COORD32;
                    if (WEIGHTED) sw[at + 1] = 0.0;
                }
            }
            if (WEIGHTED && !cs.w) {
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    if (c < nch)
                        for (int e = lane; e < cn[c]; e += 64) sw[co[c] + e] = 1.0;
            }
            __syncthreads();
            // bands of the lane inside the chunks: [lo, hi) = entries with klo <= key <= khi, by branch-free binary searches
            // on LDS byte addresses, all chunks in lockstep. q = address of entry base - 1 of a search that has narrowed its
            // answer to [base, base + len]: a step probes entry base + half - 1, half = len / 2 (wave-uniform), and keeps the
            // upper len - half entries where the probe passes. Every probe lies inside the chunk by construction -- no clamp
            // onto the sentinel --, and the step after the last halving reads entry base itself: an entry of the chunk or, at
            // base = n, the sentinel behind it, whose key 4.0 fails both comparisons (so an empty chunk gives lo = hi = 0).
            unsigned a_key[CH], ql[CH], qh[CH];
            int left[CH], left_max = 0;  // len of the chunk's two searches
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                a_key[c] = a_stage + COLB * (unsigned)cl.axis + ((unsigned)co[c] << 2);
                ql[c] = qh[c] = a_key[c] - 4u;
                left[c] = cn[c];
                left_max = cn[c] > left_max ? cn[c] : left_max;
            }
            for (; left_max > 1; left_max -= left_max >> 1) {  // (the longest chunk takes the most steps)
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    if (c < nch && (CH == 1 || left[c] > 1)) {
                        const unsigned half4 = (unsigned)(left[c] >> 1) << 2;
                        const unsigned pl = ql[c] + half4, ph = qh[c] + half4;
                        const float kl = *(const __attribute__((address_space(3))) float *)(size_t)pl;
                        const float kh = *(const __attribute__((address_space(3))) float *)(size_t)ph;
                        ql[c] = kl < klo ? pl : ql[c];    // entries [0, lo) have key <  klo
                        qh[c] = kh <= khi ? ph : qh[c];   // entries [0, hi) have key <= khi
                        left[c] -= left[c] >> 1;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
            if (c < nch) {
            const int n = cn[c];
            int lo = (int)((ql[c] + 4u - a_key[c]) >> 2), hi = (int)((qh[c] + 4u - a_key[c]) >> 2);
            lo += *(const __attribute__((address_space(3))) float *)(size_t)(ql[c] + 4u) < klo ? 1 : 0;
            hi += *(const __attribute__((address_space(3))) float *)(size_t)(qh[c] + 4u) <= khi ? 1 : 0;
            if (n_own == 0) lo = hi = n;  // lanes without an object walk the sentinel
            if constexpr (R == 1 && CH == 1) {
                // diagonal job of a self count: only the entries behind the lane object's own place in the triple run of its strip
                // (every unordered pair is then met from one side only and counts twice at the flush)
                if (it.pad_ & 1) {
                    const int own = n_own > 0 ? (int)((long long)(cl.pos3 + it.a0)[lane] - (long long)cb[c]) + 1 : n;
                    lo = own > lo ? own : lo;
                    lo = lo > hi ? hi : lo;
                }
            }
            int len = hi - lo;
            int top = hi - 1;  // the band's last entry (where a downward walk begins)
            unsigned stride = PAIRS ? 8u : 4u;  // bytes between the entries (pairs of entries) a lane evaluates (wave-uniform)
            nev += (unsigned int)(len * n_own);
            // Sparse items -- a lane tile at the border of its patch whose partner run reaches only a few of its objects, the
            // short last tile of a run: the walk takes as many trips as the longest band however few lanes have one (a seventh
            // of all trips at the headline belonged to windows with bands in at most 32 lanes). When the lanes with a band
            // span at most half the wave, their bands are SHARED OUT: 2, 4 or 8 lanes take the objects of one lane (register
            // shuffles) and every 2nd, 4th or 8th entry of its band each. Counters and bins travel with the objects, so this is done only where the
            // item consists of this one window (the lane counters are still zero and are flushed with the new owners).
            if (single_window) {
                const unsigned long long act = __builtin_amdgcn_ballot_w64(len > 0);
                const int first = act ? __builtin_ctzll(act) : 0, span = act ? 64 - __builtin_clzll(act) - first : 64;
                if (span <= 32) {
                    const int sh = span <= 8 ? 3 : (span <= 16 ? 2 : 1);
                    const bool idle = (lane >> sh) >= span;  // groups beyond the lanes that have a band: nothing to take
                    const int src = idle ? first : first + (lane >> sh);
                    const int part = lane & ((1 << sh) - 1);
                    if constexpr (R >= 2) {
#pragma unroll
                        for (int h = 0; h < R / 2; ++h) {
                            ax2[h] = f32x2{__shfl(ax2[h].x, src, 64), __shfl(ax2[h].y, src, 64)};
                            ay2[h] = f32x2{__shfl(ay2[h].x, src, 64), __shfl(ay2[h].y, src, 64)};
                            az2[h] = f32x2{__shfl(az2[h].x, src, 64), __shfl(az2[h].y, src, 64)};
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if constexpr (R < 2) { ax[r] = __shfl(ax[r], src, 64); ay[r] = __shfl(ay[r], src, 64); az[r] = __shfl(az[r], src, 64); }
                        if constexpr (MERGED) kb[r] = __shfl(kb[r], src, 64);
                        if constexpr (WEIGHTED) aw_own[r] = __shfl(aw_own[r], src, 64);
                        if constexpr (LANE_THR) {
#pragma unroll
                            for (int q = 0; q < TW; ++q) th[r][q] = sthr[kb[r] * TW + q];
                        }
                    }
                    if constexpr (LANE_THR && NE == 2) {
#pragma unroll
                        for (int h = 0; h < R / 2; ++h) nc2[h] = f32x2{-th[2 * h][0], -th[2 * h + 1][0]};
                    }
                    n_own = __shfl(n_own, src, 64);
                    lane_obj = src;
                    // lane `part` of a group takes the entries lo + part, lo + part + S, ... of the band: a lane that walks on
                    // past its share (the trip count is the wave's) meets the entries of no other lane of its group, and beyond
                    // the band entries that fail the predicate by themselves -- as on the ordinary walk
                    const int lo_s = __shfl(lo, src, 64), len_s = __shfl(len, src, 64);
                    if constexpr (PAIRS) {  // shares in units of pairs of entries; len = twice the pairs this lane takes
                        const int pairs_s = (len_s + 1) >> 1;
                        lo = idle ? n : lo_s + 2 * part;
                        len = !idle && pairs_s > part ? ((pairs_s - part + (1 << sh) - 1) >> sh) << 1 : 0;
                        stride = 8u << sh;
                    } else {
                        lo = idle ? n : lo_s + part;  // (idle lanes walk the sentinel)
                        top = lo_s + len_s - 1 - part;  // downwards: the entries hi - 1 - part, hi - 1 - part - S, ... (the same number)
                        len = !idle && len_s > part ? (len_s - part + (1 << sh) - 1) >> sh : 0;
                        stride = 4u << sh;
                    }
                }
            }
            const int steps = wave_max_nonneg(PAIRS ? (len + 1) >> 1 : len);  // the longest band of the wave: uniform trip count

            const unsigned a_chunk = a_stage + ((unsigned)co[c] << 2);
            unsigned cur = a_chunk + ((unsigned)lo << 2);
            const unsigned last = a_chunk + ((unsigned)n << 2);
            // One entry per evaluation step: three 4-byte reads from columns a fixed distance apart (lanes read nearly
            // consecutive words of a column). A trip past the end of the longest band meets entries beyond every band, or
            // the sentinel: they fail the predicate by themselves.
            // classify_entry is the whole trip of the walk loop: it leaves the undecided evaluations of the entry as wave masks
            // (any lane undecided: the return value is non-zero) and settle_entry, on the unlikely side of a branch, decides them.
            auto classify_entry = [&](const unsigned a16, unsigned long long (&unc_mask)[NS], float (&s32)[NS], double (&ewi)[NS]) {
                // PAIRS (one object per lane, one chunk per round): the trip evaluates TWO neighbouring entries for the lane's
                // object -- the packed float32 instructions that serve two objects per entry elsewhere serve two entries per
                // object here (evaluation i = entry a16 + 4 i of object 0); otherwise evaluation i = object i of the entry.
                struct { float x, y, z; } en, en1;
                en.x = *(const __attribute__((address_space(3))) float *)(size_t)a16;
                en.y = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + COLB);
                en.z = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + 2 * COLB);
                if constexpr (PAIRS) {
                    en1.x = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + 4u);
                    en1.y = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + 4u + COLB);
                    en1.z = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + 4u + 2 * COLB);
                }
                const unsigned a_w = ((a16 - a_stage) << 1) + a_sw;  // the entry's weight (one address for both entries of a pair)
                ewi[0] = WEIGHTED ? lds_f64(a_w) : 1.0;
                if constexpr (PAIRS) ewi[1] = WEIGHTED ? lds_f64(a_w + 8u) : 1.0;
                else {
#pragma unroll
                    for (int i = 1; i < NS; ++i) ewi[i] = ewi[0];
                }
                // One annulus: the centre c of the annulus is the addend of the first product, q = s32 - c comes out of the three
                // fused multiply-adds (no subtraction per evaluation; the host widens both classes by the rounding of the
                // intermediate sums, build_thr32). More edges: s32 itself.
                if constexpr (PAIRS) {
                    const f32x2 dx = ax[0] - f32x2{en.x, en1.x}, dy = ay[0] - f32x2{en.y, en1.y}, dz = az[0] - f32x2{en.z, en1.z};
                    f32x2 sq;
                    if constexpr (NE == 2) {
                        const f32x2 nc = f32x2{-th[0][0], -th[0][0]};
                        sq = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, __builtin_elementwise_fma(dx, dx, nc)));
                    } else sq = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
                    s32[0] = sq.x; s32[1] = sq.y;
                } else if constexpr (R >= 2) {
#pragma unroll
                    for (int h = 0; h < R / 2; ++h) {
                        const f32x2 dx = ax2[h] - en.x, dy = ay2[h] - en.y, dz = az2[h] - en.z;
                        f32x2 sq;
                        if constexpr (NE == 2) sq = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, __builtin_elementwise_fma(dx, dx, nc2[h])));
                        else sq = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
                        s32[2 * h] = sq.x; s32[2 * h + 1] = sq.y;
                    }
                } else {
                    const float dx = ax[0] - en.x, dy = ay[0] - en.y, dz = az[0] - en.z;
                    if constexpr (NE == 2) s32[0] = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, -th[0][0])));
                    else s32[0] = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                }
                // classes as wave masks: "certainly inside / below" feeds the lane counters (add with carry), "possibly" stays
                // on the scalar unit -- undecided = possibly & ~certainly costs no vector instruction
                unsigned long long any_mask = 0ull;
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const int r = PAIRS ? 0 : i;  // the object evaluation i belongs to
                    const double ew = ewi[i];
                    if constexpr (NE == 2) {
                        const float q = __builtin_fabsf(s32[i]);  // |s32 - c|
                        const bool in = q < th[r][1];
                        unc_mask[i] = __builtin_amdgcn_ballot_w64(q < th[r][2]) & ~__builtin_amdgcn_ballot_w64(in);
                        // weighted: acc += w of the entry where inside -- as an fma with the multiplier 1.0 / 0.0 (exact: the same
                        // rounding as the add; one select instead of two on the 64-bit operand)
                        if constexpr (WEIGHTED) acc[r][0] = __builtin_fma(in ? 1.0 : 0.0, ew, acc[r][0]);
                        else cnt[r][0] += in ? 1u : 0u;
                    } else {
                        unc_mask[i] = 0ull;
#pragma unroll
                        for (int e = 0; e < NE; ++e) {
                            const bool le = s32[i] < th[r][2 * e];  // certainly s <= t_e
                            unc_mask[i] |= __builtin_amdgcn_ballot_w64(s32[i] <= th[r][2 * e + 1]) & ~__builtin_amdgcn_ballot_w64(le);
                            if constexpr (WEIGHTED) acc[r][e] = __builtin_fma(le ? 1.0 : 0.0, ew, acc[r][e]);
                            else cnt[r][e] += le ? 1u : 0u;
                        }
                    }
                    any_mask |= unc_mask[i];
                }
                return any_mask;
            };
            // The trip of the plain one-annulus count with two objects per lane and one threshold row (the headline), with every
            // issue slot spelled out. A wave issues one instruction per turn whatever its class, and hipcc's trip spends 31 turns
            // on 17 instructions of arithmetic and reads: a result of a packed float32 instruction cannot be read by the very
            // next instruction and a compare's mask not by an add-with-carry within two, and hipcc fills those places with
            // s_nop. Here the address of the next trip (advance, clamp) stands where two of them stood, the four compares come
            // before the two adds, and the reads are waited for once (hipcc: three waits, the first of them for everything).
            // Same instructions on the same operands as classify_entry: the same float32 values, classes and masks.
            // Vector and scalar ALU only: the reads stay with the compiler (it places their one wait in front of the statement;
            // two dependent statements would get an s_nop between them from hipcc's hazard recogniser, hence one).
            // Walking downwards (DOWN) the two address instructions are one, "a16 = max(a16 - stride, 0)", and the other slot
            // takes the loop counter's decrement: 13 vector instructions, 25 in all.
            auto classify_two_objects = [&](unsigned &a16, unsigned &cur_, int &rem, unsigned long long (&unc_mask)[NS]) {
                // a16: the (clamped) address of this trip's entry on entry, of the next trip's on return; upwards cur_ is
                // advanced, downwards rem (the trips left) is counted down
                if constexpr (!SLOT_TRIP) return 0ull;
                else {
                f32x2 ex, ey, ez, q, dy, dz;  // an entry's coordinate is the low half of its operand (op_sel_hi: both halves read it)
                ex.x = *(const __attribute__((address_space(3))) float *)(size_t)a16;
                ey.x = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + COLB);
                ez.x = *(const __attribute__((address_space(3))) float *)(size_t)(a16 + 2 * COLB);
                // (q is pinned to v[0:1], a pair the compiler keeps for temporaries: the compares name its halves)
                unsigned long long in1, any_mask;
#define YAW_TRIP_SUMS_(slot)                                                                          \
    "v_pk_add_f32 v[0:1], %[ax], %[ex] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"                   \
    "v_pk_add_f32 %[dy], %[ay], %[ey] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"                    \
    "v_pk_fma_f32 v[0:1], v[0:1], v[0:1], %[nc]\n\t"                                                    \
    "v_pk_add_f32 %[dz], %[az], %[ez] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"                    \
    "v_pk_fma_f32 v[0:1], %[dy], %[dy], v[0:1]\n\t" slot "\n\t"                                        \
    "v_pk_fma_f32 v[0:1], %[dz], %[dz], v[0:1]\n\t"
#define YAW_TRIP_CLASSES_                                     \
    "v_cmp_lt_f32_e64 vcc, |v0|, %[hin]\n\t"                  \
    "v_cmp_lt_f32_e64 %[in1], |v1|, %[hin]\n\t"               \
    "v_cmp_lt_f32_e64 %[u0], |v0|, %[hout]\n\t"               \
    "v_cmp_lt_f32_e64 %[u1], |v1|, %[hout]\n\t"               \
    "s_andn2_b64 %[u0], %[u0], vcc\n\t"                       \
    "s_andn2_b64 %[u1], %[u1], %[in1]\n\t"                    \
    "v_addc_co_u32_e64 %[c0], vcc, 0, %[c0], vcc\n\t"         \
    "v_addc_co_u32_e64 %[c1], %[in1], 0, %[c1], %[in1]\n\t"   \
    "s_or_b64 %[any], %[u0], %[u1]"
                if constexpr (DOWN) {
                    asm volatile(YAW_TRIP_SUMS_("v_sub_u32_e64 %[a], %[a], %[stride] clamp") "s_add_i32 %[rem], %[rem], -1\n\t" YAW_TRIP_CLASSES_
                                 : [q] "=&{v[0:1]}"(q), [dy] "=&v"(dy), [dz] "=&v"(dz), [a] "+v"(a16), [rem] "+s"(rem),
                                   [in1] "=&s"(in1), [u0] "=&s"(unc_mask[0]), [u1] "=&s"(unc_mask[1]), [any] "=&s"(any_mask),
                                   [c0] "+v"(cnt[0][0]), [c1] "+v"(cnt[1][0])
                                 : [ax] "v"(ax2[0]), [ay] "v"(ay2[0]), [az] "v"(az2[0]), [ex] "v"(ex), [ey] "v"(ey), [ez] "v"(ez),
                                   [nc] "s"(nc2[0]), [stride] "s"(stride), [hin] "s"(th[0][1]), [hout] "s"(th[0][2])
                                 : "vcc", "scc");
                } else {
                    asm volatile(YAW_TRIP_SUMS_("v_add_u32 %[cur], %[stride], %[cur]") "v_min_u32 %[nxt], %[last], %[cur]\n\t" YAW_TRIP_CLASSES_
                                 : [q] "=&{v[0:1]}"(q), [dy] "=&v"(dy), [dz] "=&v"(dz), [cur] "+v"(cur_), [nxt] "=&v"(a16),
                                   [in1] "=&s"(in1), [u0] "=&s"(unc_mask[0]), [u1] "=&s"(unc_mask[1]), [any] "=&s"(any_mask),
                                   [c0] "+v"(cnt[0][0]), [c1] "+v"(cnt[1][0])
                                 : [ax] "v"(ax2[0]), [ay] "v"(ay2[0]), [az] "v"(az2[0]), [ex] "v"(ex), [ey] "v"(ey), [ez] "v"(ez),
                                   [nc] "s"(nc2[0]), [stride] "s"(stride), [last] "s"(last), [hin] "s"(th[0][1]), [hout] "s"(th[0][2])
                                 : "vcc", "scc");
                }
#undef YAW_TRIP_SUMS_
#undef YAW_TRIP_CLASSES_
                return any_mask;
                }
            };
            // inside a guard band: the exact float64 predicate on the float64 columns decides (rare). The entry's address, masks,
            // float32 distances and weights are what classify_entry left of the trip.
            auto settle_entry = [&](const unsigned a16, const unsigned long long (&unc_mask)[NS], const float (&s32)[NS], const double (&ewi)[NS]) {
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    const int r = PAIRS ? 0 : i;
                    const unsigned eidx = ((a16 - a_chunk) >> 2) + (PAIRS ? (unsigned)i : 0u);
                    const double ew = ewi[i];
                    if (((unc_mask[i] >> lane) & 1ull) && eidx < (unsigned)n && r < n_own) {
                        const ExactEval<NE> ev = band32_exact<NE>(cl.x, cl.y, cl.z, it.a0 + lane_obj * R + r, cs.x, cs.y, cs.z,
                                                                  cs.idx ? (int64_t)cs.idx[cb[c] + eidx] : cb[c] + (int64_t)eidx,
                                                                  t + (size_t)(MERGED ? kb[r] : kfix) * NE,
                                                                  counters + EXACT_EVAL_CTR(0) + CTR_SLOT_WORDS * (ticket & (EVAL_SLOTS - 1)));
                        const double sd = ev.s;
                        if constexpr (NE == 2) {
                            const bool in = sd > ev.th[0] && sd <= ev.th[1];
                            if constexpr (WEIGHTED) acc[r][0] += in ? ew : 0.0;
                            else cnt[r][0] += in ? 1u : 0u;
                        } else {
#pragma unroll
                            for (int e = 0; e < NE; ++e) {
                                const bool open = !(s32[i] < th[r][2 * e]) && s32[i] <= th[r][2 * e + 1];  // this edge was left undecided
                                const bool le = open && sd <= ev.th[e];
                                if constexpr (WEIGHTED) acc[r][e] += le ? ew : 0.0;
                                else cnt[r][e] += le ? 1u : 0u;
                            }
                        }
                    }
                }
            };
            // One entry per trip (1, 2 and 4 measured the same: 0.362 / 0.366 / 0.374 ms at the headline). The exact path is the
            // unlikely side of a branch inside the loop: the trip falls through to the latch. (Taken out of the loop -- an inner
            // loop left with the undecided entry, a resume loop around it -- hipcc 7.2 unifies the two exits through flag
            // registers: 42 instead of 31 instructions per trip. DESIGN.md section 8.)
            if constexpr (DOWN) {
                // from the band's last entry down to its first, then on into the entries below the band or the sentinels in front
                // of the chunk (lanes without a band: the sentinel at address 0 from the start)
                const unsigned start = len > 0 ? a_chunk + ((unsigned)top << 2) : 0u;
                unsigned a16 = start, unused = 0u;
                int rem = steps;
                while (rem != 0) {
                    unsigned long long unc_mask[NS];
                    if (__builtin_expect(classify_two_objects(a16, unused, rem, unc_mask) != 0ull, 0)) {
                        const float s32[NS] = {0.0f, 0.0f};  // (one annulus, no weights: the exact path reads neither)
                        const double ewi[NS] = {1.0, 1.0};
                        const unsigned back = (unsigned)(steps - rem - 1) * stride;  // the entry of this trip again
                        settle_entry(start > back ? start - back : 0u, unc_mask, s32, ewi);
                    }
                }
            } else if constexpr (SLOT_TRIP) {
                unsigned a16 = cur < last ? cur : last;  // the clamped address of a trip is made in a slot of the trip before
                int unused = 0;
                for (int s = 0; s < steps; ++s) {
                    unsigned long long unc_mask[NS];
                    if (__builtin_expect(classify_two_objects(a16, cur, unused, unc_mask) != 0ull, 0)) {
                        const float s32[NS] = {0.0f, 0.0f};  // (one annulus, no weights: the exact path reads neither)
                        const double ewi[NS] = {1.0, 1.0};
                        const unsigned at = cur - stride;    // the entry of this trip again
                        settle_entry(at < last ? at : last, unc_mask, s32, ewi);
                    }
                }
            } else {
                auto eval_entry = [&](const unsigned a16) {
                    unsigned long long unc_mask[NS];
                    float s32[NS];
                    double ewi[NS];
                    if (__builtin_expect(classify_entry(a16, unc_mask, s32, ewi) != 0ull, 0)) settle_entry(a16, unc_mask, s32, ewi);
                };
                for (int s = 0; s < steps; ++s) {
                    eval_entry(cur < last ? cur : last);
                    cur += stride;
                }
            }
            }
            }
            // a lane counter grows by at most one per trip, the LDS cell by 64 R per trip: flush before 2^32
            if (!WEIGHTED && (round_no & flush_mask) == flush_mask) flush_counts();
            if (win >= it.nwin) break;
            __syncthreads();  // every lane is done with this round's stage
            next_round();
            issue_round();
        }
        ++round_no;
        if constexpr (WEIGHTED) {
            flush_lanes();
            __syncthreads();
            for (int idx = lane; idx < nslots; idx += 64) {
                partials[(int64_t)it.pot * nslots + idx] = (double)hist[idx];
                hist[idx] = HistT(0);
            }
        } else {
            flush_counts();
        }
        // (a lane's sum stays below 2^32 as long as an item adds less than 2^31 to it -- the per-item sum over the wave it
        // replaces needed the whole wave's below 2^32)
        if (__builtin_amdgcn_ballot_w64((int)nev < 0)) { send_entries(nev); nev = 0; }
    }
    send_entries(nev);
}

}  // namespace

namespace yawhip_detail {

// The variants compiled are the ones named in these lists (pick); launch_count (yawhip.hip) calls this launcher or the other
// inclusion's by L.one_chunk.
hipError_t YAW_B32_LAUNCH(const CountLaunch &L, bool wgt, int32_t *variant) {
    const std::pair<int, int> stage{L.R, L.cap};
    const std::pair<bool, bool> rows{L.merged, L.uni};
    const dim3 band_grid(L.band_grid), wave(64);
    return pick<Bool<false>, Bool<true>>(wgt, [&](auto w) {
        return pick<Int<4>, Int<3>, Int<2>>(L.n_edges, [&](auto ne) {
            return pick<Rows<true, false>, Rows<true, true>, Rows<false, true>>(rows, [&](auto r) {
                return pick<Stage<4, B32_CAP_BIG>, Stage<2, B32_CAP_BIG>, Stage<2, B32_CAP>, Stage<1, B32_CAP>>(stage, [&](auto s) {
                    using S = decltype(s);
                    using M = decltype(r);
                    *variant = variant_code(YAW_B32_CH == 1 ? VF_BAND32_ONE : VF_BAND32, S::R, S::CAP, w, ne, M::MERGED, M::UNI);
                    return launch(YAW_B32_NAME<S::R, S::CAP, w, ne, M::MERGED, M::UNI>, band_grid, wave, L.lds, L.stream, L.d_tabs,
                                  L.d_items, L.n_bins, L.d_t, L.d_thr32, L.d_rwin, L.d_ucap, L.flush_mask, L.swap ? 1 : 0,
                                  L.d_counts, L.d_partials, L.d_ctr, L.seg_cap);
                });
            });
        });
    });
}

}  // namespace yawhip_detail
