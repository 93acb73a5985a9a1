// yawhip_kernel_lean.hip -- k_count_merged / k_count_merged_occ8 (SWEEP): the lean culling kernel, float32 only on chip, survivors
// evaluated 64 at a time in exact float64. One of the kernel units of the count call; yawhip.hip has the map.
#include "yawhip_count_device.h"

namespace {
constexpr int MERGED_FLUSH_MASK = (1 << 16) - 1; // k_count_merged: 256 lane objects x 64 streamed objects per stage

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

}  // namespace

namespace yawhip_detail {

size_t merged_stage_lds() { return 2 * MSTAGE * sizeof(ObjF); }
size_t merged_lds(bool weighted, int bins, int n_edges) {
    return merged_stage_lds() + (size_t)bins * n_edges * sizeof(double) + (size_t)bins * (n_edges - 1) * (weighted ? 8 * (MWG / 64) : 4) +
           (size_t)bins * sizeof(float) + (size_t)MWG * sizeof(unsigned int) + 16;
}

// One workgroup per item: grids in pieces (in_pieces).
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

}  // namespace yawhip_detail
