// yawhip_random.hip -- uniform random catalogues (BoxRandoms, reference src/yaw/randoms.py) drawn on the device from
// the very stream numpy's Generator reads, so that the values are the reference's bit for bit.
//
// numpy's PCG64 is a 128-bit LCG  s <- s * M + inc (mod 2^128)  with the output rotr64(hi ^ lo, hi >> 58) of the new
// state. d steps are the affine map  s <- A_d s + C_d,  A_d = M^d, C_d = inc (M^d - 1) / (M - 1), so any position of
// the stream is reached in log2(d) steps from a table of the maps of 2^j steps (made on the host, 2 KiB).
// One chunk of BoxRandoms.__call__(k) reads, in order:
//   * 2k 64-bit outputs: x = x_min + x_range * ((out >> 11) * 2^-53), then y the same way (Generator.uniform);
//   * with attached data, k bounded integers from the 32-bit stream (Generator.integers(0, n_data), n_data <= 2^32):
//     a pending high half of the state first, then the low and the high half of every further output; a candidate v
//     is accepted iff (v * n_data mod 2^32) >= (2^32 - n_data) mod n_data and then gives (v * n_data) >> 32 (numpy's
//     Lemire step). The k-th accepted candidate fixes where the stream ends and whether a half is left pending.
// Kernels (workgroups of 256 threads, each handles ROUNDS outputs 256 apart, so stores are coalesced):
//   * k_random_uniform writes x and y;
//   * k_random_count counts the accepted candidates of every workgroup's tile of a window of outputs, k_random_scan
//     turns the counts into workgroup offsets, k_random_compact writes the accepted values in stream order (wave64
//     ballot + mbcnt inside a wave, a scan over the waves and rounds of the workgroup, the workgroup offset) and
//     gathers weights[idx] / redshifts[idx] from device copies of the data. A window too short for the chunk is
//     followed by the next one, from the output after its end.
// The host follows the state from chunk to chunk with the same affine maps (unsigned __int128).
//
// HealPixRandoms (yawhip_random_healpix) reads the stream in the same shape -- 2k 64-bit outputs, then the k indices -- and
// differs in what it makes of the outputs: output i picks a pixel of the mask, u = (out >> 11) * 2^-53 searched in the
// cumulative probabilities of the unmasked pixels (numpy's searchsorted(cdf, u, "right")), output k + i picks one of the
// 4^(29 - order) order-29 pixels inside it, sub = out >> (64 - 2 (29 - order)). k_random_healpix does both and writes the
// centre of that order-29 nested pixel as x = phi, y = z = sin(dec): integer ring arithmetic of HEALPix' pix2loc, then
// the few float64 operations of the host route (randoms.py: pix2loc_nest) in its order, every one rounded on its own.
// The index pass and the state bookkeeping are the ones above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "yawhip_devmem.h"
#include "yawhip_healpix_math.h"
#include "yawhip_random.h"

namespace yawrand {

using yawhip_detail::DevPtr;

namespace {

constexpr int WG = 256;
constexpr int WG_LOG2 = 8;
constexpr int WAVES = WG / 64;
constexpr int ROUNDS = 16;                           // outputs per thread
constexpr int64_t TILE = (int64_t)WG * ROUNDS;       // outputs per workgroup
constexpr int64_t WINDOW_MAX = (int64_t)1 << 22;     // outputs per window of the bounded-integer pass
constexpr int64_t WINDOW_TILES = WINDOW_MAX / TILE;  // workgroups of a full window
constexpr int SCAN_WG = 1024;
static_assert(WG == 1 << WG_LOG2 && ROUNDS * WAVES == 64, "k_random_compact scans its ROUNDS x WAVES totals with one wave");

struct U128 {
    uint64_t hi, lo;
};
struct Affine {  // s -> a s + c (mod 2^128)
    U128 a, c;
};

__device__ __forceinline__ U128 mul(U128 x, U128 y) {
    return {__umul64hi(x.lo, y.lo) + x.lo * y.hi + x.hi * y.lo, x.lo * y.lo};
}

__device__ __forceinline__ U128 apply(const Affine &f, U128 s) {
    const U128 p = mul(f.a, s);
    const uint64_t lo = p.lo + f.c.lo;
    return {p.hi + f.c.hi + (lo < p.lo ? 1u : 0u), lo};
}

__device__ __forceinline__ uint64_t output(U128 s) {
    const uint64_t x = s.hi ^ s.lo;
    const unsigned r = (unsigned)(s.hi >> 58);
    return (x >> r) | (x << ((64u - r) & 63u));
}

// the state d steps after s
__device__ __forceinline__ U128 jump(const Affine *__restrict__ pow2, U128 s, uint64_t d) {
    for (int j = 0; d != 0; ++j, d >>= 1)
        if (d & 1) s = apply(pow2[j], s);
    return s;
}

__device__ __forceinline__ unsigned lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Outputs 0 .. 2n-1 after the state s0: the first n are x, the others y.
__global__ __launch_bounds__(WG) void k_random_uniform(U128 s0, const Affine *__restrict__ pow2, int64_t n, double x_min,
                                                       double x_range, double y_min, double y_range, double *__restrict__ x,
                                                       double *__restrict__ y) {
    const int64_t first = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (first >= 2 * n) return;
    const Affine stride = pow2[WG_LOG2];
    U128 s = jump(pow2, s0, (uint64_t)first + 1);
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = first + (int64_t)r * WG;
        if (i >= 2 * n) break;
        const double u = (double)(output(s) >> 11) * 0x1.0p-53;  // exact: an integer below 2^53 times a power of two
        if (i < n)
            x[i] = x_min + x_range * u;
        else
            y[i - n] = y_min + y_range * u;
        s = apply(stride, s);
    }
}

// ---- HealPixRandoms ----
constexpr int HP_ORDER = 29;                                // every point is the centre of a nested pixel of this order
constexpr double HP_FACT2 = 4.0 / 3458764513820540928.0;    // 4 / npix, npix = 12 * 4^29
constexpr double HP_FACT1 = 1073741824.0 * HP_FACT2;        // 2 nside * fact2

struct HealpixMap {
    int shift;           // 2 (29 - order): bits of the sub-pixel number
    int64_t n_unmasked;
    const int64_t *__restrict__ ipix;  // unmasked pixels of the map, nested, ascending
    const double *__restrict__ cdf;    // their cumulative probabilities, cdf[n_unmasked - 1] == 1
};

// Points 0 .. n-1 of a chunk after the state s0: output i picks the mask pixel, output n + i the sub-pixel.
__global__ __launch_bounds__(WG) void k_random_healpix(U128 s0, const Affine *__restrict__ pow2, int64_t n, HealpixMap map,
                                                       double *__restrict__ x, double *__restrict__ y, int64_t *__restrict__ pix) {
    const int64_t first = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (first >= n) return;
    const Affine stride = pow2[WG_LOG2];
    U128 sa = jump(pow2, s0, (uint64_t)first + 1);
    U128 sb = jump(pow2, s0, (uint64_t)(n + first) + 1);
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t i = first + (int64_t)r * WG;
        if (i >= n) break;
        const double u = (double)(output(sa) >> 11) * 0x1.0p-53;
        const uint64_t sub = output(sb) >> (64 - map.shift);
        int64_t lo = 0, hi = map.n_unmasked;  // the slot is the number of cdf values <= u
        while (lo < hi) {
            const int64_t m = (lo + hi) >> 1;
            if (map.cdf[m] <= u) lo = m + 1; else hi = m;
        }
        lo = lo < map.n_unmasked ? lo : map.n_unmasked - 1;  // u < 1 == cdf[n_unmasked - 1]: never taken, keeps the load inside
        const uint64_t p = ((uint64_t)map.ipix[lo] << map.shift) | sub;
        double phi, z;
        yawpix::pixel_centre(HP_ORDER, yawpix::ring_position_nest(HP_ORDER, (int64_t)p), HP_FACT1, HP_FACT2, phi, z);
        x[i] = phi;
        y[i] = z;
        if (pix) pix[i] = (int64_t)p;
        sa = apply(stride, sa);
        sb = apply(stride, sb);
    }
}

// The 2 ROUNDS candidates of this thread: low and high half of outputs o = tile + r * WG + threadIdx.x (< n_out).
struct Candidates {
    uint32_t v[2 * ROUNDS];
    int64_t o0, n_out;
    __device__ Candidates(U128 s0, const Affine *__restrict__ pow2, int64_t n_out_) : n_out(n_out_) {
        o0 = (int64_t)blockIdx.x * TILE + threadIdx.x;
        const Affine stride = pow2[WG_LOG2];
        U128 s = o0 < n_out ? jump(pow2, s0, (uint64_t)o0 + 1) : s0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const uint64_t out = output(s);
            v[2 * r] = (uint32_t)out;
            v[2 * r + 1] = (uint32_t)(out >> 32);
            if (r + 1 < ROUNDS) s = apply(stride, s);
        }
    }
    __device__ bool live(int r) const { return o0 + (int64_t)r * WG < n_out; }
};

__device__ __forceinline__ bool accepted(uint32_t v, uint64_t n_data, uint32_t threshold) {
    return (uint32_t)((uint64_t)v * n_data) >= threshold;
}

__global__ __launch_bounds__(WG) void k_random_count(U128 s0, const Affine *__restrict__ pow2, int64_t n_out, uint64_t n_data,
                                                     uint32_t threshold, int32_t *__restrict__ counts) {
    __shared__ int32_t wave_count[WAVES];
    const Candidates c(s0, pow2, n_out);
    int32_t mine = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        if (c.live(r)) mine += (int)accepted(c.v[2 * r], n_data, threshold) + (int)accepted(c.v[2 * r + 1], n_data, threshold);
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t total = 0;
        for (int w = 0; w < WAVES; ++w) total += wave_count[w];
        counts[blockIdx.x] = total;
    }
}

// offs[b] = counts[0] + ... + counts[b - 1]; *total = sum of all. One workgroup.
__global__ __launch_bounds__(SCAN_WG) void k_random_scan(const int32_t *__restrict__ counts, int64_t nb, int64_t *__restrict__ offs,
                                                         int64_t *__restrict__ total) {
    __shared__ long long wave_sum[SCAN_WG / 64];
    __shared__ long long carry;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += SCAN_WG) {
        const int64_t i = base + threadIdx.x;
        const long long v = i < nb ? counts[i] : 0;
        long long s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        if (lane == 63) wave_sum[w] = s;
        __syncthreads();
        long long before = carry;
        for (int k = 0; k < w; ++k) before += wave_sum[k];
        if (i < nb) offs[i] = before + s - v;
        __syncthreads();
        if (threadIdx.x == SCAN_WG - 1) carry = before + s;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

struct Sink {  // where an accepted value at position p < need goes
    int64_t need;
    const double *__restrict__ dw;
    const double *__restrict__ dz;
    double *__restrict__ w;
    double *__restrict__ z;
    int64_t *__restrict__ idx;
    __device__ __forceinline__ void put(int64_t p, uint32_t value) const {
        if (p >= need) return;
        if (idx) idx[p] = value;
        if (dw) w[p] = dw[value];
        if (dz) z[p] = dz[value];
    }
};

// Accepted candidates of the window in stream order, from position out_base on (first >= 0: the accepted pending half of
// the chunk, written at position 0 by the first thread). *last = candidate number (2 o + half) of position need - 1.
__global__ __launch_bounds__(WG) void k_random_compact(U128 s0, const Affine *__restrict__ pow2, int64_t n_out, uint64_t n_data,
                                                       uint32_t threshold, const int64_t *__restrict__ offs, int64_t out_base,
                                                       int64_t first, Sink sink, int64_t *__restrict__ last) {
    __shared__ int32_t round_wave[ROUNDS * WAVES];  // accepted per (round, wave), then their exclusive scan
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (first >= 0 && blockIdx.x == 0 && threadIdx.x == 0) sink.put(0, (uint32_t)first);
    const Candidates c(s0, pow2, n_out);
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const bool live = c.live(r);
        const uint64_t lo = __ballot(live && accepted(c.v[2 * r], n_data, threshold));
        const uint64_t hi = __ballot(live && accepted(c.v[2 * r + 1], n_data, threshold));
        if (lane == 0) round_wave[r * WAVES + w] = __popcll(lo) + __popcll(hi);
    }
    __syncthreads();
    if (w == 0) {  // the 64 (round, wave) totals in stream order: one per lane
        const int v = round_wave[lane];
        int s = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(s, d);
            if (lane >= d) s += t;
        }
        round_wave[lane] = s - v;
    }
    __syncthreads();
    const int64_t base = out_base + offs[blockIdx.x];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const bool live = c.live(r);
        const bool ok_lo = live && accepted(c.v[2 * r], n_data, threshold);
        const bool ok_hi = live && accepted(c.v[2 * r + 1], n_data, threshold);
        const uint64_t lo = __ballot(ok_lo), hi = __ballot(ok_hi);
        const int64_t p = base + round_wave[r * WAVES + w] + lanes_below(lo) + lanes_below(hi);
        const int64_t o = c.o0 + (int64_t)r * WG;
        if (ok_lo) {
            sink.put(p, (uint32_t)(((uint64_t)c.v[2 * r] * n_data) >> 32));
            if (p == sink.need - 1) *last = 2 * o;
        }
        if (ok_hi) {
            const int64_t q = p + (ok_lo ? 1 : 0);
            sink.put(q, (uint32_t)(((uint64_t)c.v[2 * r + 1] * n_data) >> 32));
            if (q == sink.need - 1) *last = 2 * o + 1;
        }
    }
}

// ---- host: the stream in unsigned __int128 ----
using u128 = unsigned __int128;
constexpr u128 PCG_MULT = ((u128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull;

struct HostMap {
    u128 a, c;
    u128 operator()(u128 s) const { return a * s + c; }
};

HostMap steps(u128 inc, uint64_t d) {  // the map of d steps
    u128 am = 1, ac = 0, cm = PCG_MULT, cc = inc;
    while (d) {
        if (d & 1) {
            am *= cm;
            ac = ac * cm + cc;
        }
        cc = (cm + 1) * cc;
        cm *= cm;
        d >>= 1;
    }
    return {am, ac};
}

uint64_t host_output(u128 s) {
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    const uint64_t x = hi ^ lo;
    const unsigned r = (unsigned)(hi >> 58);
    return (x >> r) | (x << ((64u - r) & 63u));
}

U128 dev(u128 s) { return {(uint64_t)(s >> 64), (uint64_t)s}; }

#define TRY(expr)                          \
    do {                                   \
        hipError_t e_ = (expr);            \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

// The chunks of one draw. `coords` is what tells the generators apart: coords.launch(stream, s0, pow2, k, x, y) writes the
// k coordinate pairs of a chunk from the 2k outputs after the state s0, coords.fetch(stream, off, k) copies what it
// made besides x and y to the host; what coords needs on the device is already there.
template <class Coords>
hipError_t draw_chunks(hipStream_t stream, const Draw &d, DrawEnd &end, const Coords &coords) {
    const u128 inc = ((u128)d.inc_hi << 64) | d.inc_lo;
    u128 state = ((u128)d.state_hi << 64) | d.state_lo;
    bool pending = d.has_uint32 != 0;
    uint32_t half = d.uinteger;
    const int64_t chunk_max = std::min(d.n, d.chunksize);
    const bool bounded = d.n_data > 1;                     // n_data == 1 returns zeros and reads nothing
    const bool gather = d.n_data >= 1 && (d.data_w || d.data_z || d.idx_out);
    const uint32_t threshold = bounded ? (uint32_t)((((uint64_t)1 << 32) - (uint64_t)d.n_data) % (uint64_t)d.n_data) : 0;
    const double accept_rate = 1.0 - threshold / 4294967296.0;

    DevPtr<Affine> pow2;  // (a count of zero allocates nothing and leaves the pointer null)
    DevPtr<double> x, y, w, z, dw, dz;
    DevPtr<int64_t> idx, offs, scalars;
    DevPtr<int32_t> counts;
    TRY(pow2.alloc(64));
    TRY(x.alloc(chunk_max));
    TRY(y.alloc(chunk_max));
    if (bounded) {
        if (d.data_w) TRY(w.alloc(chunk_max));
        if (d.data_z) TRY(z.alloc(chunk_max));
        if (d.idx_out) TRY(idx.alloc(chunk_max));
        if (d.data_w) TRY(dw.alloc(d.n_data));
        if (d.data_z) TRY(dz.alloc(d.n_data));
        TRY(counts.alloc(WINDOW_TILES));
        TRY(offs.alloc(WINDOW_TILES));
        TRY(scalars.alloc(2));
        if (d.data_w) TRY(hipMemcpyAsync(dw, d.data_w, d.n_data * sizeof(double), hipMemcpyHostToDevice, stream));
        if (d.data_z) TRY(hipMemcpyAsync(dz, d.data_z, d.n_data * sizeof(double), hipMemcpyHostToDevice, stream));
    }
    Affine table[64];
    for (int j = 0; j < 64; ++j) {
        const HostMap m = steps(inc, (uint64_t)1 << j);
        table[j] = {dev(m.a), dev(m.c)};
    }
    TRY(hipMemcpyAsync(pow2, table, sizeof table, hipMemcpyHostToDevice, stream));
    const Sink sink_proto{0, dw, dz, w, z, idx};

    for (int64_t off = 0; off < d.n; off += chunk_max) {
        const int64_t k = std::min(chunk_max, d.n - off);
        TRY(coords.launch(stream, dev(state), pow2, k, x, y));
        state = steps(inc, 2 * (uint64_t)k)(state);
        if (bounded) {
            Sink sink = sink_proto;
            sink.need = k;
            int64_t got = 0, first = -1;
            if (pending) {  // the pending half is the chunk's first candidate
                pending = false;
                const uint64_t m = (uint64_t)half * (uint64_t)d.n_data;
                if ((uint32_t)m >= threshold) {
                    first = (int64_t)(m >> 32);
                    got = 1;
                }
            }
            bool launched = false;
            while (got < k || (first >= 0 && !launched)) {
                const int64_t rest = k - got;
                int64_t n_out = 0;
                if (rest > 0) {
                    const double want = rest / accept_rate + 8.0 * std::sqrt((double)rest) + 64.0;  // candidates
                    n_out = std::min<int64_t>(WINDOW_MAX, (int64_t)std::ceil(want / 2.0));
                }
                const unsigned nb = (unsigned)std::max<int64_t>(1, (n_out + TILE - 1) / TILE);
                const U128 s0 = dev(state);
                if (n_out > 0) {
                    hipLaunchKernelGGL(k_random_count, dim3(nb), dim3(WG), 0, stream, s0, pow2, n_out, (uint64_t)d.n_data, threshold, counts);
                    TRY(hipGetLastError());
                    hipLaunchKernelGGL(k_random_scan, dim3(1), dim3(SCAN_WG), 0, stream, counts, (int64_t)nb, offs, scalars);
                    TRY(hipGetLastError());
                } else {
                    TRY(hipMemsetAsync(offs, 0, sizeof(int64_t), stream));
                    TRY(hipMemsetAsync(scalars, 0, sizeof(int64_t), stream));
                }
                TRY(hipMemsetAsync(scalars + 1, 0xff, sizeof(int64_t), stream));  // last = -1
                hipLaunchKernelGGL(k_random_compact, dim3(nb), dim3(WG), 0, stream, s0, pow2, n_out, (uint64_t)d.n_data, threshold, offs,
                                   got, launched ? (int64_t)-1 : first, sink, scalars + 1);
                TRY(hipGetLastError());
                launched = true;
                if (n_out == 0) break;  // only the pending half was needed
                int64_t host_scalars[2];
                TRY(hipMemcpyAsync(host_scalars, scalars, sizeof host_scalars, hipMemcpyDeviceToHost, stream));
                TRY(hipStreamSynchronize(stream));
                if (got + host_scalars[0] >= k) {  // the window holds the chunk's last value: the stream ends at its candidate
                    const int64_t cand = host_scalars[1];
                    state = steps(inc, (uint64_t)(cand / 2 + 1))(state);
                    pending = (cand & 1) == 0;  // the low half was the last one read: the high half waits
                    got = k;
                } else {
                    got += host_scalars[0];
                    state = steps(inc, (uint64_t)n_out)(state);
                }
                half = (uint32_t)(host_output(state) >> 32);  // numpy keeps the high half of the last output, pending or read
            }
        }
        TRY(hipMemcpyAsync(d.x_out + off, x, k * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRY(hipMemcpyAsync(d.y_out + off, y, k * sizeof(double), hipMemcpyDeviceToHost, stream));
        TRY(coords.fetch(stream, off, k));
        if (bounded) {
            if (d.w_out) TRY(hipMemcpyAsync(d.w_out + off, w, k * sizeof(double), hipMemcpyDeviceToHost, stream));
            if (d.z_out) TRY(hipMemcpyAsync(d.z_out + off, z, k * sizeof(double), hipMemcpyDeviceToHost, stream));
            if (d.idx_out) TRY(hipMemcpyAsync(d.idx_out + off, idx, k * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        }
        TRY(hipStreamSynchronize(stream));
        if (gather && !bounded) {  // n_data == 1: every index is 0 and no draw is made
            if (d.w_out) std::fill(d.w_out + off, d.w_out + off + k, d.data_w[0]);
            if (d.z_out) std::fill(d.z_out + off, d.z_out + off + k, d.data_z[0]);
            if (d.idx_out) std::fill(d.idx_out + off, d.idx_out + off + k, (int64_t)0);
        }
    }
    end.state_hi = (uint64_t)(state >> 64);
    end.state_lo = (uint64_t)state;
    end.has_uint32 = pending ? 1 : 0;
    end.uinteger = half;
    return hipSuccess;
}

struct BoxCoords {
    const BoxDraw &d;
    hipError_t launch(hipStream_t stream, U128 s0, const Affine *pow2, int64_t k, double *x, double *y) const {
        hipLaunchKernelGGL(k_random_uniform, dim3((unsigned)((2 * k + TILE - 1) / TILE)), dim3(WG), 0, stream, s0, pow2, k, d.x_min,
                           d.x_range, d.y_min, d.y_range, x, y);
        return hipGetLastError();
    }
    hipError_t fetch(hipStream_t, int64_t, int64_t) const { return hipSuccess; }
};

struct HealpixCoords {
    HealpixMap map;
    int64_t *pix, *pix_out;  // device chunk and host output of the drawn order-29 pixels, both null if not asked for
    hipError_t launch(hipStream_t stream, U128 s0, const Affine *pow2, int64_t k, double *x, double *y) const {
        hipLaunchKernelGGL(k_random_healpix, dim3((unsigned)((k + TILE - 1) / TILE)), dim3(WG), 0, stream, s0, pow2, k, map, x, y, pix);
        return hipGetLastError();
    }
    hipError_t fetch(hipStream_t stream, int64_t off, int64_t k) const {
        return pix_out ? hipMemcpyAsync(pix_out + off, pix, k * sizeof(int64_t), hipMemcpyDeviceToHost, stream) : hipSuccess;
    }
};

}  // namespace

hipError_t draw_box(hipStream_t stream, const BoxDraw &d, DrawEnd &end) {
    return draw_chunks(stream, d, end, BoxCoords{d});
}

hipError_t draw_healpix(hipStream_t stream, const HealpixDraw &d, DrawEnd &end) {
    HealpixCoords c{{2 * (HP_ORDER - d.order), d.n_unmasked, nullptr, nullptr}, nullptr, d.pix_out};
    DevPtr<int64_t> ipix, pix;  // the map goes up once, before the chunks
    DevPtr<double> cdf;
    TRY(ipix.alloc(d.n_unmasked));
    TRY(cdf.alloc(d.n_unmasked));
    TRY(hipMemcpyAsync(ipix, d.ipix_unmasked, d.n_unmasked * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    TRY(hipMemcpyAsync(cdf, d.cdf, d.n_unmasked * sizeof(double), hipMemcpyHostToDevice, stream));
    if (d.pix_out) TRY(pix.alloc(std::min(d.n, d.chunksize)));
    c.map.ipix = ipix, c.map.cdf = cdf, c.pix = pix;
    const hipError_t e = draw_chunks(stream, d, end, c);
    if (e != hipSuccess) (void)hipStreamSynchronize(stream);  // the uploads read this call's host memory
    return e;
}

}  // namespace yawrand
