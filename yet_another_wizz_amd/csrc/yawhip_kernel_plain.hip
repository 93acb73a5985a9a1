// yawhip_kernel_plain.hip -- k_count (EXACT / FILTER, any input): 256-thread workgroups, the lane objects in registers, the c1
// segment streamed through LDS. One of the kernel units of the count call; yawhip.hip has the map.
#include "yawhip_count_device.h"

namespace {
constexpr int COUNT_FLUSH_MASK = (1 << 13) - 1;  // k_count: stages between flushes of the 32-bit LDS counters (see there)

struct alignas(16) Obj {  // one streamed object in LDS: two 16-byte broadcast reads
    double x, y, z, w;
};

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

}  // namespace

namespace yawhip_detail {

size_t count_lds(bool weighted, bool priv, int n_edges) {
    return 2 * STAGE * (sizeof(Obj) + sizeof(ObjF)) + (size_t)((n_edges + 1) & ~1) * sizeof(double) +
           (size_t)(n_edges - 1) * (priv ? WG : 1) * (weighted ? 8 : 4);
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

}  // namespace yawhip_detail
