// yawhip_ingest.hip -- how a catalogue gets onto the device and into the orders the count kernels read (yawhip_kernel_*.hip): nearest
// patch centres (yawhip_assign_patches), the upload in (patch, z-bin, u) order with its patch boxes and unit-norm check
// (yawhip_catalog_*), the strip layouts (build_strip_layout) and their merged triple runs (build_triples), with the kernels
// that build them. The sorts themselves are yawhip_sort.hip's. No count kernel is launched from here.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "yawhip_internal.h"

using namespace yawhip_detail;

namespace {

// Nearest patch centre of every object (replaces scipy.cluster.vq.vq in assign_patch_centers, catalog.py:229-249):
// squared distance accumulated x, y, z in that order with separately rounded products and sums, first minimum
// wins -- the arithmetic of scipy's small-dimension vq loop, so ids are identical including exact ties.
__global__ __launch_bounds__(256) void k_assign_patches(int64_t n, const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ z, int n_centers,
                                                       const double *__restrict__ centers, int32_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double *c = reinterpret_cast<double *>(lds_raw);  // [n_centers][3]
    for (int e = threadIdx.x; e < 3 * n_centers; e += blockDim.x) c[e] = centers[e];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double px = x[i], py = y[i], pz = z[i];
    double best = INFINITY;
    int best_j = -1;
    for (int j = 0; j < n_centers; ++j) {
        const double dx = px - c[3 * j], dy = py - c[3 * j + 1], dz = pz - c[3 * j + 2];
        const double xx = dx * dx;
        const double yy = dy * dy;
        const double zz = dz * dz;
        const double sxy = xx + yy;
        const double d = sxy + zz;
        if (d < best) {
            best = d;
            best_j = j;
        }
    }
    out[i] = best_j;
}

// ---- upload-side kernels: ordering of a catalogue on the device (the sorts themselves: yawhip_sort.hip) ----
__global__ void k_gather_columns(int64_t n, const uint32_t *__restrict__ perm, const double *__restrict__ sx,
                                 const double *__restrict__ sy, const double *__restrict__ sz, const double *__restrict__ sw,
                                 double *__restrict__ dx, double *__restrict__ dy, double *__restrict__ dz, double *__restrict__ dw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = perm[i];
    dx[i] = sx[src];
    dy[i] = sy[src];
    dz[i] = sz[src];
    if (sw) dw[i] = sw[src];
}

// The gather of yawhip_catalog_upload_scalar: ONE permutation fills two catalogues -- the plain one (d*: weights sw, none
// without) and its twin (k*: the same coordinates, weights kappa * w, kappa without sw). The product is one float64 multiply
// rounded on its own (no sum follows it, and the build contracts nothing): the value numpy's kappa * w has on the host.
__global__ void k_gather_columns_scalar(int64_t n, const uint32_t *__restrict__ perm, const double *__restrict__ sx,
                                        const double *__restrict__ sy, const double *__restrict__ sz, const double *__restrict__ sw,
                                        const double *__restrict__ sk, double *__restrict__ dx, double *__restrict__ dy,
                                        double *__restrict__ dz, double *__restrict__ dw, double *__restrict__ kx,
                                        double *__restrict__ ky, double *__restrict__ kz, double *__restrict__ kw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = perm[i];
    const double vx = sx[src], vy = sy[src], vz = sz[src], kappa = sk[src];
    dx[i] = vx;
    dy[i] = vy;
    dz[i] = vz;
    kx[i] = vx;
    ky[i] = vy;
    kz[i] = vz;
    if (sw) {
        const double wv = sw[src];
        dw[i] = wv;
        kw[i] = kappa * wv;
    } else {
        kw[i] = kappa;
    }
}

// Sum of the weight column over every (patch, bin) segment of a resident catalogue, one workgroup per segment: thread t adds
// the objects lo + t, lo + t + 256, ... in that order, then the 256 partial sums are folded in halves through the LDS. The
// order is a function of the segment alone: the same catalogue gives the same bits every time; no atomics.
__global__ __launch_bounds__(256) void k_segment_weight_sums(const double *__restrict__ w, const int64_t *__restrict__ off,
                                                            double *__restrict__ out) {
    __shared__ double part[256];
    const int64_t lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) acc += w[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// largest s in [0, n_seg) with off[s] <= i (off[0] = 0 <= i < off[n_seg])
__device__ __forceinline__ int segment_of(const int64_t *__restrict__ off, int n_seg, int64_t i) {
    int lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// bin id of every object of the strip layout = its (patch, bin) segment in the input order, modulo B
__global__ void k_gather_bins(int64_t n, const uint32_t *__restrict__ perm, const int64_t *__restrict__ off, int64_t n_seg,
                              int n_bins, int32_t *__restrict__ bins) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bins[i] = segment_of(off, (int)n_seg, (int64_t)perm[i]) % n_bins;
}

// float32 images of a strip layout's columns, rounded to nearest: [3][stride] -- and the same values once more as one
// 16-byte record per object, {x, y, z, bin id} (0 where the layout has no bin ids), for the lane side of the float32 band
// kernels: a lane fetches an object with one load instead of four. The LANE_IMAGE_PAD records behind the last object are zero.
__global__ void k_make_q(int64_t n, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                         const int32_t *__restrict__ bins, int64_t stride, float *__restrict__ q, LaneObj *__restrict__ q4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + LANE_IMAGE_PAD) return;
    if (i >= n) {
        q4[i] = LaneObj{0.0f, 0.0f, 0.0f, 0};
        return;
    }
    const float fx = (float)x[i], fy = (float)y[i], fz = (float)z[i];
    q[i] = fx;
    q[stride + i] = fy;
    q[2 * stride + i] = fz;
    q4[i] = LaneObj{fx, fy, fz, bins ? bins[i] : 0};
}

// How often two neighbours of the (strip, u)-sorted order share their redshift bin: ~1/B when redshift and position are
// unrelated, towards 1 when they are not -- then the lanes of a wave keep hitting the same histogram cells.
__global__ void k_same_bin_neighbours(int64_t n, const int32_t *__restrict__ bins, unsigned long long *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool same = i + 1 < n && bins[i] == bins[i + 1];
    const unsigned long long m = __builtin_amdgcn_ballot_w64(same);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, (unsigned long long)__popcll(m));
}

// grid index of every object (0 without strips) and the occupied range per patch: floor((v + 1) / width) (lat = 0), or
// floor((latitude + pi/2) / width) with the latitude atan2(v, hypot(u, w)) of the object's direction (lat = 1, sep_angle)
__global__ void k_strip_index(int64_t n, const double *__restrict__ v, const double *__restrict__ u, const double *__restrict__ w,
                              double width, int lat, const int64_t *__restrict__ poff, int n_patches, int32_t *__restrict__ gidx,
                              int32_t *__restrict__ lohi) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = i < n;
    int32_t g = 0;
    int p = -1;
    if (ok) {
        const double vi = v[i];
        if (width > 0.0)
            g = lat ? (int32_t)floor((atan2(vi, hypot(u[i], w[i])) + 1.5707963267948966) / width) : (int32_t)floor((vi + 1.0) / width);
        gidx[i] = g;
        p = segment_of(poff, n_patches, i);
    }
    // Objects of a patch are contiguous, so nearly every wave sits inside one patch: reduce there and issue one
    // atomic pair per wave (one pair per object on 2P addresses cost 97 ms for 10 M objects).
    const int p0 = __builtin_amdgcn_readfirstlane(p);
    if (__builtin_amdgcn_ballot_w64(p != p0) == 0ull) {
        if (p0 < 0) return;  // whole wave past the end
        int32_t lo = g, hi = g;
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, __shfl_xor(lo, off, 64));
            hi = max(hi, __shfl_xor(hi, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&lohi[2 * p0], lo);
            atomicMax(&lohi[2 * p0 + 1], hi);
        }
    } else if (ok) {  // a wave across a patch boundary (or the ragged end)
        atomicMin(&lohi[2 * p], g);
        atomicMax(&lohi[2 * p + 1], g);
    }
}

// run id of the object that is i-th in `order` (objects of a patch are contiguous in the input)
__global__ void k_run_of(int64_t n, const uint32_t *__restrict__ order, const int32_t *__restrict__ gidx,
                         const int64_t *__restrict__ poff, int n_patches, const int64_t *__restrict__ vbase,
                         const int64_t *__restrict__ slo, uint32_t *__restrict__ run) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = order[i];
    const int p = segment_of(poff, n_patches, (int64_t)src);
    run[i] = (uint32_t)(vbase[p] + (int64_t)gidx[src] - slo[p]);
}

// moff[r] = first position of the (sorted) run column that holds a run >= r; moff[n_runs] = n
__global__ void k_run_offsets(const uint32_t *__restrict__ run_sorted, int64_t n, int64_t n_runs, int64_t *__restrict__ moff) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_runs) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)run_sorted[mid] < r) lo = mid + 1; else hi = mid;
    }
    moff[r] = lo;
}

// monotone map double -> uint64 (atomicMin / atomicMax on the images order like the doubles)
__host__ __device__ inline unsigned long long sortable_of(double d) {
    unsigned long long b;
    memcpy(&b, &d, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double double_of(unsigned long long s) {
    const unsigned long long b = (s >> 63) ? (s & 0x7fffffffffffffffull) : ~s;
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}

// Bounding box of every patch ([P][6]: min x, y, z, max x, y, z as sortable images) and, in box[6 P], the number of
// waves that saw an object off the unit sphere. One atomic set per wave inside a patch (see k_strip_index).
__global__ void k_patch_boxes(int64_t n, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                              const int64_t *__restrict__ poff, int n_patches, unsigned long long *__restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = i < n;
    double v[3] = {0.0, 0.0, 0.0};
    int p = -1;
    bool off_sphere = false;
    if (ok) {
        v[0] = x[i]; v[1] = y[i]; v[2] = z[i];
        p = segment_of(poff, n_patches, i);
        const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        off_sphere = !(n2 > 1.0 - UNIT_NORM_TOL && n2 < 1.0 + UNIT_NORM_TOL);
    }
    if (__builtin_amdgcn_ballot_w64(off_sphere) != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&box[(size_t)6 * n_patches], 1ull);
    const int p0 = __builtin_amdgcn_readfirstlane(p);
    if (__builtin_amdgcn_ballot_w64(p != p0) == 0ull) {
        if (p0 < 0) return;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            unsigned long long lo = sortable_of(v[a]), hi = lo;
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&box[(size_t)6 * p0 + a], lo);
                atomicMax(&box[(size_t)6 * p0 + 3 + a], hi);
            }
        }
    } else if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(&box[(size_t)6 * p + a], sortable_of(v[a]));
            atomicMax(&box[(size_t)6 * p + 3 + a], sortable_of(v[a]));
        }
    }
}

// one thread per (run, cell boundary): g[c] by bisection with the predicate cell(key) < c
template <typename KeyT>
__global__ __launch_bounds__(256) void k_run_grid(int64_t n_runs, const int64_t *__restrict__ off, const KeyT *__restrict__ key,
                                                  RunGrid *__restrict__ grid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = i / (RUN_GRID + 1);
    const int c = (int)(i - r * (RUN_GRID + 1));
    if (r >= n_runs) return;
    const int64_t b0 = off[r], b1 = off[r + 1];
    double inv = 0.0, first = 0.0, last = 0.0;
    if (b1 > b0) {
        first = (double)key[b0];
        last = (double)key[b1 - 1];
        const double span = last - first;
        inv = span > 0.0 ? (double)RUN_GRID / span : 0.0;
        if (!(inv < 1e300)) inv = 0.0;  // a denormal span: one cell
    }
    int64_t l = b0, h = b1;
    while (l < h) {
        const int64_t m = (l + h) >> 1;
        if (run_cell((double)key[m], first, inv) < c) l = m + 1; else h = m;
    }
    grid[r].g[c] = (uint32_t)(l - b0);
    if (c == 0) {  // the head of the record: what the item builder reads of the run before g[] (an empty run: n = 0)
        grid[r].b0 = b0; grid[r].first = first; grid[r].last = last; grid[r].inv = inv;
        grid[r].n = (uint32_t)(b1 - b0);
    }
}

// keys of the first and last object of every lane tile, into its record (the rest of the record comes from the host)
__global__ __launch_bounds__(256) void k_tile_keys(int64_t n_tiles, const double *__restrict__ key, TileRec *__restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tiles) return;
    const int64_t a0 = rec[i].a0;
    rec[i].klo = key[a0];
    rec[i].khi = key[a0 + rec[i].na - 1];
}

// Merged triple runs of a strip layout (streamed side of the float32 band kernels). With a grid as wide as the largest
// separation the partners of a lane tile in strip c are the strips c - 1, c, c + 1 of the other patch: three windows, three
// band searches and three walks per item, each walk as long as the longest of 64 short bands. The triple run T(group, c)
// holds the objects of those three strips MERGED along u (float32 images, weights, and the index of every entry in the
// layout's own order for the exact re-evaluation): one window, one search, one walk whose trip count is the longest of 64
// bands three times as long -- relatively more even. Every object is a member of three triples: 36 bytes of float32 images
// per object more (+ 4 for the index, + 24 with weights). c runs over [first strip - 1, last strip + 1] of the group.
// One thread per entry: its place in each of its three triples is its rank among the members (ties: lower run first) -- the
// order (key, run, position in the run) is the SAME total order of objects in every triple two objects share, which is what
// lets a self count take every unordered pair once: a lane object walks only the entries BEHIND its own place in the triple
// of its strip (pos3), and the pair (a, b) is then met from exactly one side (k_count_band32_one, half bands).
__global__ __launch_bounds__(256) void k_merge_triples(int64_t n, int64_t n_runs, const int64_t *__restrict__ off,
                                                       const int32_t *__restrict__ run_group, const int64_t *__restrict__ vbase,
                                                       const int64_t *__restrict__ off3, const double *__restrict__ key,
                                                       const float *__restrict__ q, int64_t q_stride, const double *__restrict__ w,
                                                       float *__restrict__ q3, int64_t q3_stride, double *__restrict__ w3,
                                                       int32_t *__restrict__ idx3, int32_t *__restrict__ pos3) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t lo = 0, hi = n_runs;  // run of the entry: the largest r with off[r] <= i
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    const int64_t r = lo;
    const int64_t g = run_group[r], g_lo = vbase[g], g_hi = vbase[g + 1];
    const double ki = key[i];
    const float fx = q[i], fy = q[q_stride + i], fz = q[2 * q_stride + i];
    const double wi = w ? w[i] : 0.0;
    // entries of the group's runs r - 2 .. r + 2 in front of this one
    int64_t before[5];
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
        const int64_t m = r + d;
        int64_t cnt = 0;
        if (d == 0) {
            cnt = i - off[r];
        } else if (m >= g_lo && m < g_hi) {
            int64_t l = off[m], h = off[m + 1];
            const int64_t base = l;
            if (d < 0) { while (l < h) { const int64_t mid = (l + h) >> 1; if (key[mid] <= ki) l = mid + 1; else h = mid; } }
            else       { while (l < h) { const int64_t mid = (l + h) >> 1; if (key[mid] < ki) l = mid + 1; else h = mid; } }
            cnt = l - base;
        }
        before[d + 2] = cnt;
    }
#pragma unroll
    for (int d = -1; d <= 1; ++d) {  // triple centred on run r + d: members r + d - 1, r + d, r + d + 1
        const int64_t t = r + d + 1 + 2 * g;
        const int64_t dst = off3[t] + before[d + 1] + before[d + 2] + before[d + 3];
        q3[dst] = fx; q3[q3_stride + dst] = fy; q3[2 * q3_stride + dst] = fz;
        idx3[dst] = (int32_t)i;
        if (w3) w3[dst] = wi;
        if (d == 0) pos3[i] = (int32_t)dst;  // where the object stands in the triple of its OWN strip (half bands of self counts)
    }
}

}  // namespace

namespace yawhip_detail {

// Build one strip layout of a catalogue from its resident (patch, bin, u) copy: orientation o = sort axis inside a run,
// strips of the global grid along (o + 2) % 3; seg = groups are the (patch, bin) segments instead of the patches.
int build_strip_layout(yawhip_ctx *ctx, yawhip_catalog *c, int o, bool seg) {
    StripLayout &L = seg ? c->seg[o] : c->strips[o];
    if (L.built) return YAWHIP_OK;
    const int64_t n = c->n, nseg = (int64_t)c->n_patches * c->nb;
    const int n_groups = seg ? (int)nseg : c->n_patches;
    const bool want_bins = !seg && c->nb > 1;
    const double width = c->strip_width;
    const int saxis = (o + 2) % 3;  // z -> y, y -> x, x -> z
    std::vector<int64_t> h_poff((size_t)n_groups + 1);
    for (int g = 0; g <= n_groups; ++g) h_poff[(size_t)g] = seg ? c->h_off[(size_t)g] : c->h_off[(size_t)g * c->nb];
    const size_t col = (size_t)std::max<int64_t>(n, 1) * sizeof(double) + 16;  // + 16: the band kernel's 16-byte loads may touch the bytes behind the last element
    DevPtr<uint32_t> perm, perm2, run, run_sorted;  // sort scratch: freed on the way out
    DevPtr<int32_t> gidx, lohi;
    DevPtr<int64_t> poff;
    auto bail = [&](hipError_t err, const char *what) {
        L.release();
        return fail(err == hipErrorOutOfMemory ? YAWHIP_ERR_OOM : YAWHIP_ERR_HIP, "strip layout (%s) failed: %s", what,
                    hipGetErrorString(err));
    };
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int32_t> h_lohi((size_t)2 * n_groups);
    for (int g = 0; g < n_groups; ++g) { h_lohi[(size_t)2 * g] = INT32_MAX; h_lohi[(size_t)2 * g + 1] = INT32_MIN; }
    const size_t n1 = (size_t)std::max<int64_t>(n, 1);
    hipError_t e = poff.alloc((size_t)(n_groups + 1));
    if (e == hipSuccess) e = lohi.alloc((size_t)2 * n_groups);
    if (e == hipSuccess) e = gidx.alloc(n1);
    if (e == hipSuccess) e = perm.alloc(n1);
    if (e == hipSuccess) e = perm2.alloc(n1);
    if (e == hipSuccess) e = run.alloc(n1);
    if (e == hipSuccess) e = run_sorted.alloc(n1);
    if (e == hipSuccess)
        e = hipMemcpyAsync(poff, h_poff.data(), (size_t)(n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(lohi, h_lohi.data(), (size_t)2 * n_groups * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return bail(e, "strip tables");
    const unsigned ngrid = (unsigned)((n1 + 255) / 256);
    // grid index of every object, first / last occupied strip of every group
    hipLaunchKernelGGL(k_strip_index, dim3(ngrid), dim3(256), 0, ctx->stream, n, key_of(c->x, c->y, c->z, saxis),
                       key_of(c->x, c->y, c->z, (saxis + 1) % 3), key_of(c->x, c->y, c->z, (saxis + 2) % 3), width, c->strip_grid && !seg ? 1 : 0, poff,
                       n_groups, gidx, lohi);
    e = hipMemcpyAsync(h_lohi.data(), lohi, (size_t)2 * n_groups * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(e, "strip index");
    std::vector<int64_t> vbase((size_t)n_groups + 1, 0), slo((size_t)n_groups, 0);
    for (int g = 0; g < n_groups; ++g) {
        const bool any = h_poff[(size_t)g + 1] > h_poff[(size_t)g];
        slo[(size_t)g] = any ? h_lohi[(size_t)2 * g] : 0;
        vbase[(size_t)g + 1] = vbase[(size_t)g] + (any ? (int64_t)h_lohi[(size_t)2 * g + 1] - h_lohi[(size_t)2 * g] + 1 : 0);
    }
    const int64_t n_runs = vbase[(size_t)n_groups];
    if (n_runs >= (1ll << 31)) return bail(hipErrorInvalidValue, "too many strip runs");
    int run_bits = 1;
    while ((1ll << run_bits) < n_runs) ++run_bits;
    e = L.d_vbase.alloc((size_t)(n_groups + 1));
    if (e == hipSuccess) e = L.d_slo.alloc((size_t)std::max(n_groups, 1));
    if (e == hipSuccess)
        e = hipMemcpyAsync(L.d_vbase, vbase.data(), (size_t)(n_groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(L.d_slo, slo.data(), (size_t)n_groups * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    // order along the sort axis inside every group, then group by run (unique keys (run, rank): no reliance on
    // the stability of the sort)
    if (e == hipSuccess) e = yawsort::sort_segments(ctx->sort_ws, ctx->stream, n, key_of(c->x, c->y, c->z, o), poff, n_groups, perm);
    if (e != hipSuccess) return bail(e, "group sort");
    hipLaunchKernelGGL(k_run_of, dim3(ngrid), dim3(256), 0, ctx->stream, n, perm, gidx, poff, n_groups, L.d_vbase, L.d_slo, run);
    e = yawsort::sort_runs(ctx->sort_ws, ctx->stream, n, run, perm, run_bits, perm2, run_sorted);
    if (e != hipSuccess) return bail(e, "run sort");
    e = L.x.alloc(n1, 16);
    if (e == hipSuccess) e = L.y.alloc(n1, 16);
    if (e == hipSuccess) e = L.z.alloc(n1, 16);
    if (e == hipSuccess && c->w) e = L.w.alloc(n1, 16);
    if (e == hipSuccess && want_bins) e = L.k.alloc(n1, 16);
    L.q_stride = (int64_t)((n1 + 3) & ~(size_t)3) + 8;  // a 16-byte load of the band kernel may run up to 12 bytes past a column
    if (e == hipSuccess) e = L.q.alloc((size_t)3 * L.q_stride);
    if (e == hipSuccess) e = L.q4.alloc((size_t)(n + LANE_IMAGE_PAD));
    if (e == hipSuccess) e = L.off.alloc((size_t)(n_runs + 1));
    if (e == hipSuccess) e = L.d_grid.alloc((size_t)(n_runs + 1));
    if (e == hipSuccess) e = hipMemsetAsync(L.d_grid, 0, (size_t)(n_runs + 1) * sizeof(RunGrid), ctx->stream);  // [V]: read for groups without runs
    if (e != hipSuccess) return bail(e, "strip layout");
    hipLaunchKernelGGL(k_gather_columns, dim3(ngrid), dim3(256), 0, ctx->stream, n, perm2, c->x, c->y, c->z, c->w, L.x, L.y, L.z, L.w);
    if (want_bins)
        hipLaunchKernelGGL(k_gather_bins, dim3(ngrid), dim3(256), 0, ctx->stream, n, perm2, c->off, nseg, c->nb, L.k);
    hipLaunchKernelGGL(k_make_q, dim3((unsigned)((n + LANE_IMAGE_PAD + 255) / 256)), dim3(256), 0, ctx->stream, n, L.x, L.y, L.z,
                       want_bins ? (const int32_t *)L.k : nullptr, L.q_stride, L.q, L.q4);
    hipLaunchKernelGGL(k_run_offsets, dim3((unsigned)((n_runs + 1 + 255) / 256)), dim3(256), 0, ctx->stream, run_sorted, n, n_runs,
                       L.off);
    if (n_runs > 0)
        hipLaunchKernelGGL(k_run_grid<double>, dim3((unsigned)((n_runs * (RUN_GRID + 1) + 255) / 256)), dim3(256), 0, ctx->stream, n_runs,
                           L.off, o == 0 ? L.x : (o == 1 ? L.y : L.z), L.d_grid);
    std::vector<int64_t> voff((size_t)n_runs + 1);
    e = hipMemcpyAsync(voff.data(), L.off, (size_t)(n_runs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    unsigned long long h_same = 0;
    if (want_bins && n > 1) {  // `run` (sorted away by now) serves as the 8-byte result cell
        unsigned long long *d_same = reinterpret_cast<unsigned long long *>(static_cast<uint32_t *>(run));
        if (e == hipSuccess) e = hipMemsetAsync(d_same, 0, sizeof(unsigned long long), ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_same_bin_neighbours, dim3(ngrid), dim3(256), 0, ctx->stream, n, L.k, d_same);
            e = hipMemcpyAsync(&h_same, d_same, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(e, "run offsets");
    L.same_bin = n > 1 ? (double)h_same / (double)(n - 1) : 0.0;
    for (int64_t r = 0; r < n_runs; ++r)
        if (voff[(size_t)r + 1] - voff[(size_t)r] >= (1ll << 32)) return bail(hipErrorInvalidValue, "a strip run of 2^32 objects or more");
    // small per-run tables the item builder walks on the device
    for (int ri = 0; ri < 3; ++ri) {
        const int64_t tile = (int64_t)MWG << ri;
        L.h_tiles[ri].assign((size_t)n_runs + 1, 0);
        for (int64_t r = 0; r < n_runs; ++r)
            L.h_tiles[ri][(size_t)r + 1] = L.h_tiles[ri][(size_t)r] + (voff[(size_t)r + 1] - voff[(size_t)r] + tile - 1) / tile;
        {  // record of every tile: the item builder decodes a potential item with one load instead of a search over the
           // prefix and a look-up of the run's offsets
            const int64_t n_tiles = L.h_tiles[ri][(size_t)n_runs];
            std::vector<TileRec> tile_rec((size_t)std::max<int64_t>(n_tiles, 1), TileRec{0, 0, 0, 0.0, 0.0});
            for (int64_t r = 0; r < n_runs; ++r)
                for (int64_t tl = L.h_tiles[ri][(size_t)r]; tl < L.h_tiles[ri][(size_t)r + 1]; ++tl) {
                    const int64_t a0 = voff[(size_t)r] + (tl - L.h_tiles[ri][(size_t)r]) * tile;
                    tile_rec[(size_t)tl] = TileRec{a0, (int32_t)std::min<int64_t>(tile, voff[(size_t)r + 1] - a0), (int32_t)r, 0.0, 0.0};
                }
            if (e == hipSuccess) e = L.d_tile_rec[ri].alloc(tile_rec.size());
            if (e == hipSuccess)
                e = hipMemcpy(L.d_tile_rec[ri], tile_rec.data(), tile_rec.size() * sizeof(TileRec), hipMemcpyHostToDevice);
            if (e == hipSuccess && n_tiles > 0) {  // the end keys live on the device (every tile has an object: a0 + na - 1 >= a0)
                hipLaunchKernelGGL(k_tile_keys, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, ctx->stream, n_tiles,
                                   o == 0 ? L.x : (o == 1 ? L.y : L.z), L.d_tile_rec[ri]);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess) e = L.d_tiles[ri].alloc((size_t)(n_runs + 1));
        if (e == hipSuccess)
            e = hipMemcpyAsync(L.d_tiles[ri], L.h_tiles[ri].data(), (size_t)(n_runs + 1) * sizeof(int64_t),
                               hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(e, "tile tables");
    {  // run length as the typical OBJECT sees it (sum of squares / sum): equals the mean for uniform data, far above it
       // for clustered data, where most objects live in a few dense runs
        double sq = 0.0;
        for (int64_t r = 0; r < n_runs; ++r) {
            const double len = (double)(voff[(size_t)r + 1] - voff[(size_t)r]);
            sq += len * len;
        }
        L.obj_run = n > 0 ? sq / (double)n : 0.0;
    }
    L.h_off = std::move(voff);
    L.h_vbase = std::move(vbase);
    L.h_slo = std::move(slo);
    L.n_groups = n_groups;
    // (the figure is pinned byte for byte by tests/test_gpu_ingest.py: the run and tile records count with RUN_GRID_ACCOUNTED and
    // TILE_REC_ACCOUNTED bytes, their size without the item builder's heads -- 32 bytes per run and 16 per lane tile that
    // yawhip_catalog_device_bytes does not report: about half a byte per object, under 1 % of the catalogue's bytes; and, in
    // the same way, not the lane records q4: 16 bytes per object and LANE_IMAGE_PAD records per layout)
    L.device_bytes = (int64_t)col * (c->w ? 4 : 3) + (want_bins ? n * (int64_t)sizeof(int32_t) : 0) + 3 * L.q_stride * (int64_t)sizeof(float) +
                     (4 * (n_runs + 1) + 2 * (int64_t)n_groups + 1) * (int64_t)sizeof(int64_t) + (n_runs + 1) * RUN_GRID_ACCOUNTED +
                     (L.h_tiles[0][(size_t)n_runs] + L.h_tiles[1][(size_t)n_runs] + L.h_tiles[2][(size_t)n_runs]) * TILE_REC_ACCOUNTED;
    c->device_bytes += L.device_bytes;
    L.built = true;
    return YAWHIP_OK;
}

// Merged triple runs of a built strip layout (see k_merge_triples); built once, on first use as the streamed side of a
// float32 band kernel with partner strips c - 1, c, c + 1.
int build_triples(yawhip_ctx *ctx, yawhip_catalog *c, int o, bool seg) {
    StripLayout &L = seg ? c->seg[o] : c->strips[o];
    if (!L.built) return fail(YAWHIP_ERR_INVALID, "build_triples: layout not built");
    if (L.triples) return YAWHIP_OK;
    const int64_t n = c->n, G = L.n_groups, V = L.h_vbase[(size_t)G], V3 = V + 2 * G;
    if (3 * n >= (1ll << 31)) return fail(YAWHIP_ERR_INVALID, "build_triples: catalogue too large for 32-bit entry indices");
    std::vector<int64_t> off3((size_t)V3 + 1, 0);
    std::vector<int32_t> run_group((size_t)std::max<int64_t>(V, 1), 0);
    for (int64_t g = 0; g < G; ++g) {
        const int64_t lo = L.h_vbase[(size_t)g], hi = L.h_vbase[(size_t)g + 1];
        for (int64_t r = lo; r < hi; ++r) run_group[(size_t)r] = (int32_t)g;
        for (int64_t c_rel = 0; c_rel < hi - lo + 2; ++c_rel) {
            const int64_t t = lo + 2 * g + c_rel, rc = lo + c_rel - 1;
            int64_t len = 0;
            for (int64_t m = rc - 1; m <= rc + 1; ++m)
                if (m >= lo && m < hi) len += L.h_off[(size_t)m + 1] - L.h_off[(size_t)m];
            off3[(size_t)t + 1] = len;
        }
    }
    for (int64_t t = 0; t < V3; ++t) off3[(size_t)t + 1] += off3[(size_t)t];
    if (off3[(size_t)V3] != 3 * n) return fail(YAWHIP_ERR_HIP, "build_triples: %lld entries for %lld objects", (long long)off3[(size_t)V3], (long long)n);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n3 = (size_t)std::max<int64_t>(3 * n, 1);
    L.q3_stride = (int64_t)((n3 + 3) & ~(size_t)3) + 8;  // as q_stride: a 16-byte load may run up to 12 bytes past a column
    DevPtr<int32_t> d_run_group;
    hipError_t e = L.q3.alloc((size_t)3 * L.q3_stride);
    if (e == hipSuccess) e = L.idx3.alloc(n3);
    if (e == hipSuccess) e = L.pos3.alloc((size_t)std::max<int64_t>(n, 1));
    if (e == hipSuccess && c->w) e = L.w3.alloc(n3, 16);
    if (e == hipSuccess) e = L.off3.alloc((size_t)(V3 + 1));
    if (e == hipSuccess) e = L.d_grid3.alloc((size_t)(V3 + 1));
    if (e == hipSuccess) e = d_run_group.alloc(run_group.size());
    if (e == hipSuccess) e = hipMemsetAsync(L.q3, 0, (size_t)3 * L.q3_stride * sizeof(float), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(L.d_grid3, 0, (size_t)(V3 + 1) * sizeof(RunGrid), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(L.off3, off3.data(), (size_t)(V3 + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_run_group, run_group.data(), run_group.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n > 0) {
        hipLaunchKernelGGL(k_merge_triples, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, V, L.off, d_run_group,
                           L.d_vbase, L.off3, o == 0 ? L.x : (o == 1 ? L.y : L.z), L.q, L.q_stride, L.w, L.q3, L.q3_stride, L.w3, L.idx3, L.pos3);
        hipLaunchKernelGGL(k_run_grid<float>, dim3((unsigned)((V3 * (RUN_GRID + 1) + 255) / 256)), dim3(256), 0, ctx->stream, V3, L.off3,
                           L.q3 + (size_t)o * L.q3_stride, L.d_grid3);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    d_run_group.release();
    if (e != hipSuccess) {
        L.release_triples();
        return fail(e == hipErrorOutOfMemory ? YAWHIP_ERR_OOM : YAWHIP_ERR_HIP, "merged triple runs failed: %s", hipGetErrorString(e));
    }
    const int64_t bytes = 3 * L.q3_stride * (int64_t)sizeof(float) + (int64_t)n3 * (4 + (c->w ? 8 : 0)) + n * 4 + (V3 + 1) * ((int64_t)sizeof(int64_t) + RUN_GRID_ACCOUNTED);
    L.device_bytes += bytes;
    c->device_bytes += bytes;
    L.triples = true;
    return YAWHIP_OK;
}

}  // namespace yawhip_detail

extern "C" {

int yawhip_catalog_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                          const double *w, int32_t n_patches, int32_t n_bins_or_1, const int64_t *offsets,
                          yawhip_catalog **out) {
    return yawhip_catalog_upload_axis(ctx, n, x, y, z, w, n_patches, n_bins_or_1, offsets, 2, out);
}

int yawhip_catalog_sort_axis(const yawhip_catalog *cat, int32_t *axis) {
    if (!cat || !axis) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_sort_axis: NULL argument");
    *axis = cat->axis;
    return YAWHIP_OK;
}

// The upload behind yawhip_catalog_upload_axis (kappa == NULL: one catalogue, *out) and yawhip_catalog_upload_scalar (kappa
// given: the plain catalogue *out and its twin *out_k with weights kappa * w, both from ONE copy of the coordinates and ONE
// segment sort; the twin is a catalogue like any other from there on -- own uid, own layouts, own replicas).
static int upload_catalogs(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                           const double *kappa, int32_t n_patches, int32_t n_bins_or_1, const int64_t *offsets,
                           int32_t sort_axis, yawhip_catalog **out, yawhip_catalog **out_k) {
    if (!out) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_upload: out is NULL");
    if (sort_axis < 0 || sort_axis > 2) return fail(YAWHIP_ERR_INVALID, "sort_axis must be 0 (x), 1 (y) or 2 (z)");
    *out = nullptr;
    if (out_k) *out_k = nullptr;
    if (!ctx) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_upload: ctx is NULL");
    if (n < 0 || n_patches <= 0 || n_bins_or_1 <= 0 || !offsets || (n > 0 && (!x || !y || !z)))
        return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_upload: bad sizes or NULL columns");
    const int64_t nseg = (int64_t)n_patches * n_bins_or_1;
    if (n >= (1ll << 32)) return fail(YAWHIP_ERR_INVALID, "at most 2^32 - 1 objects per catalogue");
    if (offsets[0] != 0 || offsets[nseg] != n) return fail(YAWHIP_ERR_INVALID, "offsets must start at 0 and end at n");
    for (int64_t i = 0; i < nseg; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(YAWHIP_ERR_INVALID, "offsets must be non-decreasing");
    HIP_TRY(hipSetDevice(ctx->device));
    yawhip_catalog *c = new (std::nothrow) yawhip_catalog();
    static std::atomic<uint64_t> next_uid{1};
    if (c) c->uid = next_uid.fetch_add(1);
    if (!c) return fail(YAWHIP_ERR_OOM, "host allocation failed");
    yawhip_catalog *ck = nullptr;  // the twin (kappa given)
    if (kappa) {
        ck = new (std::nothrow) yawhip_catalog();
        if (!ck) {
            delete c;
            return fail(YAWHIP_ERR_OOM, "host allocation failed");
        }
        ck->uid = next_uid.fetch_add(1);
    }
    for (yawhip_catalog *t : {c, ck}) {
        if (!t) continue;
        t->ctx = ctx;
        t->n = n;
        t->n_patches = n_patches;
        t->nb = n_bins_or_1;
        t->axis = sort_axis;
        t->h_off.assign(offsets, offsets + nseg + 1);
    }
    // Library-private order: the columns go to the device as they are and are ordered there (rocPRIM radix sorts,
    // yawhip_sort.hip): ascending along the sort axis inside every (patch, bin) segment. The strip layouts are derived
    // from this resident copy (build_strip_layout), the one of the catalogue's own sort axis right away.
    const size_t n1 = (size_t)std::max<int64_t>(n, 1);
    const size_t col = n1 * sizeof(double) + 16;  // + 16: see build_strip_layout
    DevPtr<double> rx, ry, rz, rw, rk;  // raw columns (temporary)
    DevPtr<uint32_t> perm;
    DevPtr<int64_t> poff;
    DevPtr<unsigned long long> box;  // [P][6] sortable images of min / max per axis, [6 P]: violations of the unit norm
    auto bail = [&](hipError_t err, const char *what) {
        yawhip_catalog_free(c);
        yawhip_catalog_free(ck);
        return fail(err == hipErrorOutOfMemory ? YAWHIP_ERR_OOM : YAWHIP_ERR_HIP, "catalog upload (%s) failed: %s", what,
                    hipGetErrorString(err));
    };
    std::vector<int64_t> h_poff((size_t)n_patches + 1);
    for (int p = 0; p <= n_patches; ++p) h_poff[(size_t)p] = offsets[(int64_t)p * n_bins_or_1];
    std::vector<unsigned long long> h_box((size_t)6 * n_patches + 1);
    for (int p = 0; p < n_patches; ++p)
        for (int a = 0; a < 3; ++a) {
            h_box[(size_t)6 * p + a] = sortable_of(4.0);       // running minimum
            h_box[(size_t)6 * p + 3 + a] = sortable_of(-4.0);  // running maximum
        }
    h_box[(size_t)6 * n_patches] = 0ull;
    hipError_t e = c->x.alloc(n1, 16);
    if (e == hipSuccess) e = c->y.alloc(n1, 16);
    if (e == hipSuccess) e = c->z.alloc(n1, 16);
    if (e == hipSuccess && w) e = c->w.alloc(n1, 16);
    if (e == hipSuccess) e = c->off.alloc((size_t)(nseg + 1));
    if (ck) {  // the twin's columns: coordinates, the product (always weighted), its own copy of the offsets
        for (DevPtr<double> *q : {&ck->x, &ck->y, &ck->z, &ck->w, &rk})
            if (e == hipSuccess) e = q->alloc(n1, 16);
        if (e == hipSuccess) e = ck->off.alloc((size_t)(nseg + 1));
    }
    if (e == hipSuccess) e = rx.alloc(n1, 16);
    if (e == hipSuccess) e = ry.alloc(n1, 16);
    if (e == hipSuccess) e = rz.alloc(n1, 16);
    if (e == hipSuccess && w) e = rw.alloc(n1, 16);
    if (e == hipSuccess) e = perm.alloc(n1);
    if (e == hipSuccess) e = poff.alloc((size_t)(n_patches + 1));
    if (e == hipSuccess) e = box.alloc(h_box.size());
    if (e == hipSuccess && n > 0) {
        e = hipMemcpyAsync(rx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ry, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(rz, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && w) e = hipMemcpyAsync(rw, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && ck) e = hipMemcpyAsync(rk, kappa, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess && ck)
        e = hipMemcpyAsync(ck->off, offsets, (size_t)(nseg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->off, offsets, (size_t)(nseg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(poff, h_poff.data(), (size_t)(n_patches + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(box, h_box.data(), h_box.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return bail(e, "columns");
    const unsigned ngrid = (unsigned)((std::max<int64_t>(n, 1) + 255) / 256);
    if (n > 0) {
        // bounding box of every patch (the orientation of a job follows from the boxes of its two patches) and the
        // unit-norm check of the pre-filter, both on the device
        hipLaunchKernelGGL(k_patch_boxes, dim3(ngrid), dim3(256), 0, ctx->stream, n, rx, ry, rz, poff, n_patches, box);
        e = yawsort::sort_segments(ctx->sort_ws, ctx->stream, n, key_of(rx, ry, rz, sort_axis), c->off, nseg, perm);
        if (e != hipSuccess) return bail(e, "segment sort");
        if (ck)
            hipLaunchKernelGGL(k_gather_columns_scalar, dim3(ngrid), dim3(256), 0, ctx->stream, n, perm, rx, ry, rz, rw, rk, c->x,
                               c->y, c->z, c->w, ck->x, ck->y, ck->z, ck->w);
        else
            hipLaunchKernelGGL(k_gather_columns, dim3(ngrid), dim3(256), 0, ctx->stream, n, perm, rx, ry, rz, rw, c->x, c->y, c->z, c->w);
        if ((e = hipGetLastError()) != hipSuccess) return bail(e, "gather");
        e = hipMemcpyAsync(h_box.data(), box, h_box.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return bail(e, "patch boxes");
    }
    e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(e, "finish");
    // the temporaries go before the layouts are built, not at the end: they are half of an upload's peak memory
    rx.release(); ry.release(); rz.release(); rw.release(); rk.release(); perm.release(); poff.release(); box.release();
    for (yawhip_catalog *t : {c, ck}) {
        if (!t) continue;
        t->unit_norm = h_box[(size_t)6 * n_patches] == 0ull;
        t->h_box.resize((size_t)6 * n_patches);
        for (size_t i = 0; i < t->h_box.size(); ++i) t->h_box[i] = double_of(h_box[i]);
        t->device_bytes = (int64_t)col * (t->w ? 4 : 3) + (nseg + 1) * (int64_t)sizeof(int64_t);
        t->strip_width = ctx->strip_width;
        t->strip_grid = ctx->strip_grid;
        t->has_strips = t->unit_norm && n > 0;
    }
    for (yawhip_catalog *t : {c, ck}) {  // layouts are built per catalogue (the twin's carry its own weight column)
        if (!t || !t->has_strips) continue;
        const int rc = build_strip_layout(ctx, t, sort_axis, false);
        if (rc != YAWHIP_OK) {
            yawhip_catalog_free(c);
            yawhip_catalog_free(ck);
            return rc;
        }
    }
    if (ctx->sort_ws.cap > ((size_t)1 << 25)) ctx->sort_ws.release();  // ~30 bytes per object: keep only small workspaces
    for (yawhip_ctx *peer : ctx->peers) {  // multi-device context: the same catalogue(s) on every further device
        yawhip_catalog *rep = nullptr, *rep_k = nullptr;
        const int rc = upload_catalogs(peer, n, x, y, z, w, kappa, n_patches, n_bins_or_1, offsets, sort_axis, &rep,
                                       ck ? &rep_k : nullptr);
        if (rc != YAWHIP_OK) {
            yawhip_catalog_free(c);
            yawhip_catalog_free(ck);
            return rc;
        }
        c->replicas.push_back(rep);
        if (ck) ck->replicas.push_back(rep_k);
    }
    if (ck) *out_k = ck;
    *out = c;
    return YAWHIP_OK;
}

int yawhip_catalog_upload_axis(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                               const double *w, int32_t n_patches, int32_t n_bins_or_1, const int64_t *offsets,
                               int32_t sort_axis, yawhip_catalog **out) {
    return upload_catalogs(ctx, n, x, y, z, w, nullptr, n_patches, n_bins_or_1, offsets, sort_axis, out, nullptr);
}

int yawhip_catalog_upload_scalar(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                                 const double *w, const double *kappa, int32_t n_patches, int32_t n_bins_or_1,
                                 const int64_t *offsets, int32_t sort_axis, yawhip_catalog **out_n, yawhip_catalog **out_k) {
    if (!out_n || !out_k) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_upload_scalar: out_n / out_k is NULL");
    *out_n = *out_k = nullptr;  // before every check: on any failure neither is returned
    if (n > 0 && !kappa) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_upload_scalar: kappa is NULL");
    static const double none = 0.0;  // (n == 0: nothing is read through it)
    return upload_catalogs(ctx, n, x, y, z, w, kappa ? kappa : &none, n_patches, n_bins_or_1, offsets, sort_axis, out_n, out_k);
}

int yawhip_catalog_segment_sums(const yawhip_catalog *cat, double *sums) {
    if (!cat || !sums) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_segment_sums: NULL argument");
    const int64_t nseg = (int64_t)cat->n_patches * cat->nb;
    if (!cat->w) {  // unweighted: the number of objects (exact)
        for (int64_t s = 0; s < nseg; ++s) sums[s] = (double)(cat->h_off[(size_t)s + 1] - cat->h_off[(size_t)s]);
        return YAWHIP_OK;
    }
    yawhip_ctx *ctx = cat->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    DevPtr<double> d_out;
    hipError_t e = d_out.alloc((size_t)nseg);
    if (e != hipSuccess) return fail(YAWHIP_ERR_OOM, "segment sums: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_segment_weight_sums, dim3((unsigned)nseg), dim3(256), 0, ctx->stream, cat->w, cat->off, d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(sums, d_out, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(YAWHIP_ERR_HIP, "segment sums failed: %s", hipGetErrorString(e));
    return YAWHIP_OK;
}

int yawhip_catalog_free(yawhip_catalog *c) {
    if (!c) return YAWHIP_OK;
    for (yawhip_catalog *rep : c->replicas) (void)yawhip_catalog_free(rep);
    c->replicas.clear();
    if (c->ctx) (void)hipSetDevice(c->ctx->device);
    if (c->ctx) {  // its plans hold pointers into its layouts (nothing of them is in flight: calls are blocking)
        if (c->ctx->stream) (void)hipStreamSynchronize(c->ctx->stream);
        drop_plans(c->ctx, c);
    }
    delete c;  // its columns and layouts go with it
    return YAWHIP_OK;
}

// Test hook (tests/test_gpu_lane_image.py; not part of the ABI of include/yawhip.h): builds the strip layout of orientation o
// (seg: the per-segment one) if it is not built yet, reads its lane records back and compares them word for word with the
// float32 columns and the bin ids they restate. *n_checked = objects compared, *n_differing = records that differ in any of
// their four words, plus the records of the padding that are not zero.
int yawhip_debug_lane_image(yawhip_ctx *ctx, yawhip_catalog *cat, int32_t o, int32_t seg, int64_t *n_checked, int64_t *n_differing) {
    if (!ctx || !cat || !n_checked || !n_differing || o < 0 || o > 2) return fail(YAWHIP_ERR_INVALID, "yawhip_debug_lane_image: bad argument");
    if (cat->strip_width <= 0.0 || (seg && cat->nb <= 1)) return fail(YAWHIP_ERR_INVALID, "yawhip_debug_lane_image: no such layout");
    if (const int rc = build_strip_layout(ctx, cat, o, seg != 0)) return rc;
    const StripLayout &L = seg ? cat->seg[o] : cat->strips[o];
    const int64_t n = cat->n;
    std::vector<LaneObj> rec((size_t)(n + LANE_IMAGE_PAD));
    std::vector<float> q((size_t)3 * L.q_stride);
    std::vector<int32_t> bins((size_t)n, 0);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(rec.data(), L.q4, rec.size() * sizeof(LaneObj), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q.data(), L.q, q.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (L.k && n > 0) HIP_TRY(hipMemcpy(bins.data(), L.k, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t bad = 0;
    for (int64_t i = 0; i < n + LANE_IMAGE_PAD; ++i) {
        const LaneObj want = i < n ? LaneObj{q[(size_t)i], q[(size_t)(L.q_stride + i)], q[(size_t)(2 * L.q_stride + i)], bins[(size_t)i]}
                                   : LaneObj{0.0f, 0.0f, 0.0f, 0};
        bad += memcmp(&rec[(size_t)i], &want, sizeof(LaneObj)) != 0;
    }
    *n_checked = n;
    *n_differing = bad;
    return YAWHIP_OK;
}

int yawhip_catalog_device_bytes(const yawhip_catalog *cat, int64_t *bytes) {
    if (!cat || !bytes) return fail(YAWHIP_ERR_INVALID, "yawhip_catalog_device_bytes: NULL argument");
    *bytes = cat->device_bytes;
    return YAWHIP_OK;
}

int yawhip_assign_patches(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, int32_t n_centers,
                          const double *centers_xyz, int32_t *patch_out) {
    if (!ctx) return fail(YAWHIP_ERR_INVALID, "yawhip_assign_patches: ctx is NULL");
    if (n < 0 || n_centers <= 0 || !centers_xyz || (n > 0 && (!x || !y || !z || !patch_out)))
        return fail(YAWHIP_ERR_INVALID, "yawhip_assign_patches: bad sizes or NULL arrays");
    if ((size_t)n_centers * 3 * sizeof(double) > (size_t)ctx->lds_limit)
        return fail(YAWHIP_ERR_INVALID, "too many centres (%d) for the LDS table", n_centers);
    if (n == 0) return YAWHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DevPtr<double> dx, dc;
    DevPtr<int32_t> dout;
    hipError_t e = dx.alloc((size_t)3 * n);
    if (e == hipSuccess) e = dc.alloc((size_t)3 * n_centers);
    if (e == hipSuccess) e = dout.alloc((size_t)n);
    if (e == hipSuccess) e = hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dx + n, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dx + 2 * n, z, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(dc, centers_xyz, (size_t)3 * n_centers * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const size_t lds = (size_t)3 * n_centers * sizeof(double);
        if (lds > 64 * 1024)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_assign_patches), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_assign_patches, dim3((unsigned)((n + 255) / 256)), dim3(256), lds, ctx->stream, n, dx, dx + n, dx + 2 * n,
                               n_centers, dc, dout);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(patch_out, dout, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail("yawhip_assign_patches", e);
    return YAWHIP_OK;
}

}  // extern "C"
