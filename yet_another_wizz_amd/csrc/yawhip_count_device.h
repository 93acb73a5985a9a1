// What more than one kernel unit of the count call uses (yawhip.hip maps the units): small device helpers, and the host-side
// templates that pick a compiled variant and launch it. Everything sits in an unnamed namespace: every unit that includes
// this gets its own copy, band32_exact (noinline) included. Included by the kernel units only; what one family alone uses
// lives in that family's unit.
#ifndef YAWHIP_COUNT_DEVICE_H
#define YAWHIP_COUNT_DEVICE_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "yawhip_count_kernels.h"

using namespace yawhip_detail;

namespace {
constexpr double PAD_COORD = 4.0;  // padded lanes sit >= 3 away from any unit vector: s >= 9 > max t = 4

struct alignas(16) ObjF {  // float32 image of a streamed object in LDS, for the pre-filter: one 16-byte broadcast read
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
// relative to 1 - u^2 and a square root within 2 ulp (together 2e-7 relative, times s), the product and the final fma (6e-8
// each), the margin's own subtraction (6e-8): at most 1.8e-7 + 3.2e-7 s; the partner's float32 image adds 3.1e-8. The margin
// CAP32_MARGIN = 8e-7 covers s <= 1 (3e-4 of the band half width r at the headline's r = 2.9e-3).
// The square root is the hardware's (v_sqrt_f32, within 1 ulp: inside the 2 ulp budgeted above, so the margin stands), not
// the correctly rounded sqrtf, which costs some twenty vector instructions per bound and item for a culling bound. Its
// argument is 0 or at least 2^-24 wherever the formula branch is taken: never a denormal.
constexpr float CAP32_SHIFT = 1e-7f, CAP32_CLIP = 1.2e-7f, CAP32_MARGIN = 8e-7f;
// (The clipped bound is made where it is used: with the two bounds this short, hipcc keeps both constants in vector registers
// of their own through the whole kernel, the walk loop included -- one register more in nearly every variant, a wave per
// SIMD less in five of them. The empty asm statement is not moved out of the item loop; it costs one v_mov per bound.)
__device__ __forceinline__ float cap32_clipped(float bound) {
    asm volatile("" : "+v"(bound));
    return bound;
}
__device__ __forceinline__ float cap_lo32(float u, float c, float s) {
    const float ul = fmaxf(u - CAP32_SHIFT, -1.0f), clipped = cap32_clipped(-1.0f - CAP32_MARGIN);
    return ul <= -c + CAP32_CLIP ? clipped : fmaf(ul, c, -__builtin_amdgcn_sqrtf(fmaxf(fmaf(-ul, ul, 1.0f), 0.0f)) * s) - CAP32_MARGIN;
}
__device__ __forceinline__ float cap_hi32(float u, float c, float s) {
    const float uh = fminf(u + CAP32_SHIFT, 1.0f), clipped = cap32_clipped(1.0f + CAP32_MARGIN);
    return uh >= c - CAP32_CLIP ? clipped : fmaf(uh, c, __builtin_amdgcn_sqrtf(fmaxf(fmaf(-uh, uh, 1.0f), 0.0f)) * s) + CAP32_MARGIN;
}

constexpr int SLOT_MASK = 0x3fffffff;
__host__ __device__ inline int item_slot(const Item &it) { return it.slot & SLOT_MASK; }
__host__ __device__ inline int item_orient(const Item &it) { return (int)((unsigned)it.slot >> 30); }

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// A clock stamp of the call (CTR_T_*, yawhip_count_kernels.h), by the first thread of a kernel
__device__ __forceinline__ void stamp_start(unsigned long long *__restrict__ counters, int word) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[word] = wall_clock64();
}

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

// ------------------------------------------------------------------------------------------------
// Host side: the launchers of the families are built from these.
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

// Band kernels: grid from the number of POTENTIAL items (known on the host); the kernel reads the number the builder kept
// from the device counter, workgroups beyond it exit, workgroups loop if more were kept than the grid holds. Their selectors:
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

}  // namespace

#endif
