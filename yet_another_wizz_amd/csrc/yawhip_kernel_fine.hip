// yawhip_kernel_fine.hip -- k_count_band32_fine: the float32 band kernel for fine radial grids (separation weights).
// One of the kernel units of the count call; yawhip.hip has the map.
#include "yawhip_count_device.h"

namespace {
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

}  // namespace

namespace yawhip_detail {

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

}  // namespace yawhip_detail
