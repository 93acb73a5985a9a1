// yawhip_kmeans.hip -- deterministic k-means over all objects of a catalogue with the columns resident on the device
// (yawhip_kmeans_*, include/yawhip.h; the host side and the numpy oracle: yet_another_wizz_amd/patches.py, DESIGN.md
// section 14). Every quantity summed over objects is an integer -- q_i = floor(m_i 2^29) of the k-means++ seeding, the
// per-cluster counts, the fixed-point coordinate sums a_i = rint(x_i 2^30) and the inertia floor(d 2^29) of a Lloyd round --
// so atomics, per-workgroup partials and any grid shape give the sums numpy gives, bit for bit and from run to run. No
// floating-point value is ever reduced. The squared distance is that of k_assign_patches (yawhip_ingest.hip): products
// and sums rounded one by one (the build contracts nothing), first minimum wins.
//
//   k_kmeans_seed  one object per thread; a workgroup walks SEG consecutive objects (a segment) per visit and takes
//                  segments grid-stride: m_i against the new centre, q_i, and ONE 64-bit sum per segment (wave shuffle,
//                  then LDS). The host keeps the segment sums of the last seed: their total is the draw's range.
//   k_kmeans_pick  the host finds the segment in which the prefix passes r (segments whose q are all zero cannot be it);
//                  one workgroup finds the object inside it: 16 consecutive q per thread, the thread sums in order, then
//                  the one thread whose range holds the crossing walks it.
//   k_kmeans_step  centres in LDS; one object per thread, grid-stride over a grid sized to the device; per-workgroup
//                  int64 partials [k][4] = (count, sum x, sum y, sum z) in LDS beside the centres (64-bit LDS adds),
//                  flushed once per workgroup with 64-bit global adds -- or, where they do not fit, every object adds to
//                  the global table directly. The inertia is summed per thread, per wave, then one global add per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "yawhip_internal.h"

using namespace yawhip_detail;

namespace {

constexpr int WG = 256;
constexpr int SEG_ROUNDS = 16;                      // objects per thread and segment
constexpr int64_t SEG = (int64_t)WG * SEG_ROUNDS;   // objects per segment (one 64-bit sum each)
constexpr int64_t N_MAX = (int64_t)1 << 31;
constexpr double Q_SCALE = 536870912.0;             // 2^29: d <= 4 -> q <= 2^31
constexpr double A_SCALE = 1073741824.0;            // 2^30: |x| <= 1 -> |a| <= 2^30
constexpr int PATH_NONE = 0, PATH_LDS = 1, PATH_GLOBAL = 2;

typedef unsigned long long u64;

__device__ __forceinline__ double dist2(double px, double py, double pz, double cx, double cy, double cz) {
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double zz = dz * dz;
    const double sxy = xx + yy;
    return sxy + zz;
}

// floor(d 2^29) of a squared distance 0 <= d <= 4 (the product is exact: a power of two)
__device__ __forceinline__ uint32_t quantise(double d) { return (uint32_t)(d * Q_SCALE); }

__device__ __forceinline__ u64 wave_sum(u64 v) {  // every lane of the wave calls it; lane 0 has the sum
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__global__ __launch_bounds__(WG) void k_kmeans_seed(int64_t n, int64_t n_seg, const double *__restrict__ x,
                                                    const double *__restrict__ y, const double *__restrict__ z, double cx,
                                                    double cy, double cz, int first, double *__restrict__ m,
                                                    uint32_t *__restrict__ q, u64 *__restrict__ segsum) {
    __shared__ u64 part[WG / 64];
    for (int64_t s = blockIdx.x; s < n_seg; s += gridDim.x) {
        u64 acc = 0;
        for (int j = 0; j < SEG_ROUNDS; ++j) {
            const int64_t i = s * SEG + (int64_t)j * WG + threadIdx.x;
            if (i < n) {
                double d = dist2(x[i], y[i], z[i], cx, cy, cz);
                if (!first) {
                    const double old = m[i];
                    d = old < d ? old : d;
                }
                m[i] = d;
                const uint32_t qi = quantise(d);
                q[i] = qi;
                acc += qi;
            }
        }
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 t = 0;
            for (int w = 0; w < WG / 64; ++w) t += part[w];
            segsum[s] = t;
        }
        __syncthreads();
    }
}

// One workgroup: the smallest i in [lo, hi) whose inclusive prefix sum of q over [lo, i] exceeds r (hi - lo <= SEG);
// -1 when the whole range sums to r or less.
__global__ __launch_bounds__(WG) void k_kmeans_pick(const uint32_t *__restrict__ q, int64_t lo, int64_t hi, u64 r,
                                                    int64_t *__restrict__ out) {
    __shared__ u64 part[WG];
    __shared__ u64 r_in;
    __shared__ int winner;
    const int64_t i0 = lo + (int64_t)threadIdx.x * SEG_ROUNDS;
    u64 own = 0;
    for (int j = 0; j < SEG_ROUNDS; ++j)
        if (i0 + j < hi) own += q[i0 + j];
    part[threadIdx.x] = own;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 run = 0;
        int t = 0;
        for (; t < WG; ++t) {
            if (run + part[t] > r) break;
            run += part[t];
        }
        winner = t < WG ? t : -1;
        r_in = r - run;
        if (t == WG) *out = -1;
    }
    __syncthreads();
    if ((int)threadIdx.x == winner) {
        u64 run = 0;
        for (int j = 0; j < SEG_ROUNDS; ++j) {  // (the crossing lies inside: i0 + j < hi holds up to it)
            run += q[i0 + j];
            if (run > r_in) {
                *out = i0 + j;
                break;
            }
        }
    }
}

// acc: [k][4] (count, sum x, sum y, sum z) then the inertia, all 64-bit two's complement, zeroed before the launch
template <bool WEIGHTED, bool LDS_ACC>
__global__ __launch_bounds__(WG) void k_kmeans_step(int64_t n, const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ z, const double *__restrict__ w, double wscale,
                                                    int k, const double *__restrict__ centres, u64 *__restrict__ acc,
                                                    int32_t *__restrict__ ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double *c = reinterpret_cast<double *>(lds_raw);   // [k][3]
    u64 *part = reinterpret_cast<u64 *>(c + 3 * k);    // [k][4], LDS_ACC only
    for (int e = threadIdx.x; e < 3 * k; e += WG) c[e] = centres[e];
    if constexpr (LDS_ACC)
        for (int e = threadIdx.x; e < 4 * k; e += WG) part[e] = 0;
    __syncthreads();
    u64 inertia = 0;
    for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * WG) {
        const double px = x[i], py = y[i], pz = z[i];
        double best = INFINITY;
        int best_j = 0;
        for (int j = 0; j < k; ++j) {
            const double d = dist2(px, py, pz, c[3 * j], c[3 * j + 1], c[3 * j + 2]);
            if (d < best) {
                best = d;
                best_j = j;
            }
        }
        if (ids) ids[i] = best_j;
        inertia += quantise(best);
        long long ax, ay, az;
        if constexpr (WEIGHTED) {
            const double wi = w[i];
            const double wx = wi * px;
            const double wy = wi * py;
            const double wz = wi * pz;
            ax = (long long)__builtin_rint(wx * wscale);
            ay = (long long)__builtin_rint(wy * wscale);
            az = (long long)__builtin_rint(wz * wscale);
        } else {
            ax = (long long)__builtin_rint(px * A_SCALE);
            ay = (long long)__builtin_rint(py * A_SCALE);
            az = (long long)__builtin_rint(pz * A_SCALE);
        }
        if constexpr (LDS_ACC) {
            u64 *dst = part + 4 * best_j;
            atomicAdd(dst, (u64)1);
            atomicAdd(dst + 1, (u64)ax);
            atomicAdd(dst + 2, (u64)ay);
            atomicAdd(dst + 3, (u64)az);
        } else {
            u64 *dst = acc + 4 * (size_t)best_j;
            atomicAdd(dst, (u64)1);
            atomicAdd(dst + 1, (u64)ax);
            atomicAdd(dst + 2, (u64)ay);
            atomicAdd(dst + 3, (u64)az);
        }
    }
    inertia = wave_sum(inertia);
    if ((threadIdx.x & 63) == 0 && inertia) atomicAdd(acc + 4 * (size_t)k, inertia);
    if constexpr (LDS_ACC) {
        __syncthreads();
        for (int e = threadIdx.x; e < 4 * k; e += WG) {
            const u64 v = part[e];
            if (v) atomicAdd(acc + e, v);
        }
    }
}

}  // namespace

#pragma GCC visibility push(hidden)  // (its destructor is not an export)
struct yawhip_kmeans {
    int device = 0;
    hipStream_t stream = nullptr;  // the context's
    int lds_limit = 0, n_cu = 0;
    int64_t n = 0, n_seg = 0;
    DevPtr<double> x, y, z, w;  // w may be null
    double wscale = 0.0;
    DevPtr<double> m;           // [n] squared distance to the nearest chosen centre
    DevPtr<uint32_t> q;         // [n] floor(m 2^29)
    DevPtr<u64> segsum;         // [n_seg]
    DevPtr<int64_t> pick_out;
    std::vector<u64> h_segsum;  // of the last seed
    u64 total = 0;
    bool seeded = false;
    DevBuf<u64> acc;            // [4 k + 1]
    DevBuf<double> centres;     // [3 k]
    DevPtr<int32_t> ids;        // [n], allocated when ids are first asked for
    std::vector<u64> h_acc;
    int last_path = PATH_NONE;
};
#pragma GCC visibility pop

namespace {

int max_k_step(const yawhip_kmeans *km) { return (int)std::min<size_t>((size_t)km->lds_limit / (3 * sizeof(double)), INT32_MAX / 8); }
int max_k_lds(const yawhip_kmeans *km) { return (int)std::min<size_t>((size_t)km->lds_limit / (7 * sizeof(double)), INT32_MAX / 8); }

template <bool WEIGHTED, bool LDS_ACC>
hipError_t launch_step(const yawhip_kmeans *km, unsigned grid, size_t lds, int k, int32_t *ids) {
    const void *fn = reinterpret_cast<const void *>(k_kmeans_step<WEIGHTED, LDS_ACC>);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_kmeans_step<WEIGHTED, LDS_ACC>), dim3(grid), dim3(WG), lds, km->stream, km->n, km->x, km->y, km->z, km->w,
                       km->wscale, k, km->centres.ptr, km->acc.ptr, ids);
    return hipGetLastError();
}

}  // namespace

extern "C" {

void yawhip_kmeans_close(yawhip_kmeans *km) {
    if (!km) return;
    (void)hipSetDevice(km->device);
    delete km;  // its device memory goes with it
}

int yawhip_kmeans_open(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w, double wscale,
                       yawhip_kmeans **out) {
    if (!ctx || !out) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_open: ctx or out is NULL");
    *out = nullptr;
    if (n < 1 || n > N_MAX || !x || !y || !z) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_open: n outside 1 .. 2^31 or NULL columns");
    if (w && !(std::isfinite(wscale) && wscale > 0.0))
        return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_open: wscale must be a positive finite number with weights");
    HIP_TRY(hipSetDevice(ctx->device));
    yawhip_kmeans *km = new (std::nothrow) yawhip_kmeans;
    if (!km) return fail(YAWHIP_ERR_OOM, "yawhip_kmeans_open: out of host memory");
    km->device = ctx->device;
    km->stream = ctx->stream;
    km->lds_limit = ctx->lds_limit;
    km->n_cu = ctx->n_cu;
    km->n = n;
    km->n_seg = (n + SEG - 1) / SEG;
    km->wscale = w ? wscale : 0.0;
    const size_t col = (size_t)n * sizeof(double);
    hipError_t e = km->x.alloc((size_t)n);
    if (e == hipSuccess) e = km->y.alloc((size_t)n);
    if (e == hipSuccess) e = km->z.alloc((size_t)n);
    if (e == hipSuccess && w) e = km->w.alloc((size_t)n);
    if (e == hipSuccess) e = km->m.alloc((size_t)n);
    if (e == hipSuccess) e = km->q.alloc((size_t)n);
    if (e == hipSuccess) e = km->segsum.alloc((size_t)km->n_seg);
    if (e == hipSuccess) e = km->pick_out.alloc(1);
    if (e == hipSuccess) e = hipMemcpyAsync(km->x, x, col, hipMemcpyHostToDevice, km->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(km->y, y, col, hipMemcpyHostToDevice, km->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(km->z, z, col, hipMemcpyHostToDevice, km->stream);
    if (e == hipSuccess && w) e = hipMemcpyAsync(km->w, w, col, hipMemcpyHostToDevice, km->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(km->stream);
    if (e != hipSuccess) {
        yawhip_kmeans_close(km);
        return hip_fail("yawhip_kmeans_open", e);
    }
    try {
        km->h_segsum.resize((size_t)km->n_seg);
    } catch (const std::bad_alloc &) {
        yawhip_kmeans_close(km);
        return fail(YAWHIP_ERR_OOM, "yawhip_kmeans_open: out of host memory");
    }
    *out = km;
    return YAWHIP_OK;
}

int yawhip_kmeans_seed(yawhip_kmeans *km, const double centre[3], int32_t first, uint64_t *total) {
    if (!km || !centre || !total) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_seed: NULL argument");
    if (!first && !km->seeded) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_seed: the first call of a seeding must have first = 1");
    HIP_TRY(hipSetDevice(km->device));
    km->seeded = false;
    const unsigned grid = (unsigned)std::min<int64_t>(km->n_seg, (int64_t)km->n_cu * 8);
    hipLaunchKernelGGL(k_kmeans_seed, dim3(grid), dim3(WG), 0, km->stream, km->n, km->n_seg, km->x, km->y, km->z, centre[0], centre[1],
                       centre[2], first ? 1 : 0, km->m, km->q, km->segsum);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(km->h_segsum.data(), km->segsum, (size_t)km->n_seg * sizeof(u64), hipMemcpyDeviceToHost, km->stream));
    HIP_TRY(hipStreamSynchronize(km->stream));
    u64 t = 0;
    for (u64 s : km->h_segsum) t += s;  // <= 2^31 objects x 2^31: below 2^63
    km->total = t;
    km->seeded = true;
    *total = t;
    return YAWHIP_OK;
}

int yawhip_kmeans_pick(yawhip_kmeans *km, uint64_t r, int64_t *index) {
    if (!km || !index) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_pick: NULL argument");
    if (!km->seeded) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_pick: no seed call before it");
    if (r >= km->total) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_pick: r (%llu) is not below the total (%llu)", (u64)r, km->total);
    int64_t s = 0;
    u64 before = 0;
    for (; s < km->n_seg; ++s) {  // the first segment whose inclusive prefix exceeds r
        if (before + km->h_segsum[(size_t)s] > r) break;
        before += km->h_segsum[(size_t)s];
    }
    if (s >= km->n_seg) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_pick: the segment sums do not reach r");
    HIP_TRY(hipSetDevice(km->device));
    const int64_t lo = s * SEG, hi = std::min(km->n, lo + SEG);
    hipLaunchKernelGGL(k_kmeans_pick, dim3(1), dim3(WG), 0, km->stream, km->q, lo, hi, (u64)(r - before), km->pick_out);
    HIP_TRY(hipGetLastError());
    int64_t got = -1;
    HIP_TRY(hipMemcpyAsync(&got, km->pick_out, sizeof(int64_t), hipMemcpyDeviceToHost, km->stream));
    HIP_TRY(hipStreamSynchronize(km->stream));
    if (got < lo || got >= hi) return fail(YAWHIP_ERR_HIP, "yawhip_kmeans_pick: no crossing inside segment %lld", (long long)s);
    *index = got;
    return YAWHIP_OK;
}

int yawhip_kmeans_step(yawhip_kmeans *km, int32_t k, const double *centres, int64_t *sums, int64_t *counts, uint64_t *inertia,
                       int32_t *ids) {
    if (!km || !centres || !sums || !counts || !inertia) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_step: NULL argument");
    if (k < 1) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_step: k must be positive");
    if (k > max_k_step(km)) return fail(YAWHIP_ERR_INVALID, "too many centres (%d) for the LDS table (at most %d)", k, max_k_step(km));
    HIP_TRY(hipSetDevice(km->device));
    const size_t n_acc = 4 * (size_t)k + 1;
    HIP_TRY(km->acc.reserve(n_acc));
    HIP_TRY(km->centres.reserve(3 * (size_t)k));
    if (ids && !km->ids) HIP_TRY(km->ids.alloc((size_t)km->n));
    try {
        km->h_acc.resize(n_acc);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "yawhip_kmeans_step: out of host memory");
    }
    HIP_TRY(hipMemsetAsync(km->acc.ptr, 0, n_acc * sizeof(u64), km->stream));
    HIP_TRY(hipMemcpyAsync(km->centres.ptr, centres, 3 * (size_t)k * sizeof(double), hipMemcpyHostToDevice, km->stream));
    // the partials share the LDS with the centres where both fit; the limit follows the device's LDS size
    const bool lds_acc = k <= max_k_lds(km);
    const size_t lds = (size_t)k * (lds_acc ? 7 : 3) * sizeof(double);
    // a grid sized to the device: as many workgroups per CU as their LDS admits, eight at the most
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)km->lds_limit / (int64_t)std::max<size_t>(lds, 1)));
    const unsigned grid = (unsigned)std::min<int64_t>((km->n + WG - 1) / WG, (int64_t)km->n_cu * per_cu);
    int32_t *d_ids = ids ? km->ids : nullptr;
    hipError_t e;
    if (km->w) e = lds_acc ? launch_step<true, true>(km, grid, lds, k, d_ids) : launch_step<true, false>(km, grid, lds, k, d_ids);
    else e = lds_acc ? launch_step<false, true>(km, grid, lds, k, d_ids) : launch_step<false, false>(km, grid, lds, k, d_ids);
    if (e != hipSuccess) return hip_fail("yawhip_kmeans_step", e);
    HIP_TRY(hipMemcpyAsync(km->h_acc.data(), km->acc.ptr, n_acc * sizeof(u64), hipMemcpyDeviceToHost, km->stream));
    if (ids) HIP_TRY(hipMemcpyAsync(ids, km->ids, (size_t)km->n * sizeof(int32_t), hipMemcpyDeviceToHost, km->stream));
    HIP_TRY(hipStreamSynchronize(km->stream));
    for (int32_t c = 0; c < k; ++c) {
        counts[c] = (int64_t)km->h_acc[4 * (size_t)c];
        for (int a = 0; a < 3; ++a) sums[3 * (size_t)c + a] = (int64_t)km->h_acc[4 * (size_t)c + 1 + a];
    }
    *inertia = km->h_acc[4 * (size_t)k];
    km->last_path = lds_acc ? PATH_LDS : PATH_GLOBAL;
    return YAWHIP_OK;
}

int yawhip_kmeans_query(const yawhip_kmeans *km, int32_t what, int64_t *value) {
    if (!km || !value) return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_query: NULL argument");
    switch (what) {
    case 0: *value = SEG; break;
    case 1: *value = km->last_path; break;
    case 2: *value = max_k_lds(km); break;
    case 3: *value = max_k_step(km); break;
    default: return fail(YAWHIP_ERR_INVALID, "yawhip_kmeans_query: unknown item %d", what);
    }
    return YAWHIP_OK;
}

}  // extern "C"
