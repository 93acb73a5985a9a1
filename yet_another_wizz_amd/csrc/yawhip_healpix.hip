// yawhip_healpix.hip -- HEALPix pixels of a catalogue and its map (healpix.ang2pix / healpix.healpix_map,
// Catalog.healpix_map, HealPixRandoms.from_catalog): what the reference leaves to healpy's ang2pix and np.bincount.
//
// The pixel of (phi, z = sin dec) is HEALPix' loc2pix (Gorski et al. 2005, section 4.1) in the steps of healpix.py: every
// float64 step is one IEEE operation in the written order (fmod, +, -, *, /, sqrt, floor; no FMA, no transcendental), so
// the device repeats the host route bit for bit. The arithmetic is the nested one; a ring-scheme number is that pixel's
// (face, ix, iy) put through the ring arithmetic of randoms.nest2ring (jr, nr, kshift, jp) -- one path, two numberings.
//
// Objects are uploaded in passes of `chunksize`. Per pass:
//   * k_pixels: one object per thread -> its pixel (-1 for a non-finite input or |z| > 1), stored to the pass's pixel
//     column (when the caller wants pixels), counted into the map with a 64-bit integer atomic (maps without weights: exact,
//     whatever the order) or written as a 32-bit sort key (weighted maps; an invalid point gets the key npix).
//   * weighted maps: rocPRIM's stable radix sort of (pixel, weight) over the 2 order + 4 key bits, then k_sum_runs: the
//     thread at the head of a run of equal pixels starts from the map's value and adds the run's weights in order. Passes
//     are in object order and the sort keeps object order inside a pixel, so the map is numpy's sequential
//     np.bincount(pix, w) bit for bit, run to run. A run is summed by one thread: a low-order weighted map of a huge
//     catalogue is slow (order 0: twelve threads), and still exact.
// The counters become float64 in place at the end (k_counts_to_f64) and the map goes to the host in one copy.
//
// yawhip_healpix_pixels goes the other way (healpix.map_pixels, Catalog.from_healpix_map): a full-sky scalar map, with an
// optional weight map, becomes the columns of a catalogue. The maps are uploaded once; nested pixel numbers are walked in
// passes of `chunksize`. Per pass:
//   * k_select_count: one nested pixel q per thread -> its index in the map (q, or the ring arithmetic above), the
//     selection rule of healpix.py (finite, not UNSEEN; weight finite and > 0), wave ballot + popcount, one count per
//     workgroup.
//   * rocPRIM's exclusive scan of the workgroup counts (one more entry holds the pass's total, read by the host).
//   * k_select_write: the same predicate again; a selected pixel's place is the workgroup's base + the counts of the waves
//     before its own + the ballot bits below its lane, so the output keeps ascending q. It stores the map's own pixel
//     number, the centre (phi, z) in the float64 steps of randoms.pix2loc_nest, the value and the weight.
// No atomics and no floating-point sums; every pixel and element index is 64-bit (an order-13 map is 6.4 GB). The selected
// part of the pass is then copied to the host outputs at the running offset -- after the host has checked that it fits.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "yawhip_healpix.h"
#include "yawhip_healpix_math.h"

namespace yawpix {

using yawhip_detail::grid_for;

namespace {

constexpr int WG = 256;
constexpr double TWOTHIRD = 2.0 / 3.0;

__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// Pixel of `order` that holds (phi, z); -1 for a non-finite phi or z, or |z| > 1. The float64 steps of healpix.py.
__device__ __forceinline__ int64_t loc2pix(int order, int nested, double phi, double z) {
    const double za = fabs(z);
    if (!(fabs(phi) < __builtin_huge_val()) || !(za <= 1.0)) return -1;  // a NaN fails either comparison
    const int64_t nside = (int64_t)1 << order;
    const double fn = (double)nside;
    double r = fmod(phi, TWOPI);  // exact
    if (r < 0.0) r = r + TWOPI;
    if (r >= TWOPI) r = 0.0;      // -1e-20 + 2 pi rounds to 2 pi
    const double tt = r / HALFPI;  // [0, 4)
    int64_t face, ix, iy;
    if (za <= TWOTHIRD) {  // belt
        const double t1 = fn * (0.5 + tt);
        const double t2 = fn * z * 0.75;
        // 0.5 + tt can round to 4.5 and t2 to +-0.5 nside: an edge line index 5 nside names the corner pixel one below it
        const int64_t jp = imin((int64_t)floor(t1 - t2), 5 * nside - 1);  // ascending edge line
        const int64_t jm = imin((int64_t)floor(t1 + t2), 5 * nside - 1);  // descending edge line
        const int64_t ifp = jp >> order, ifm = jm >> order;              // 0 .. 4
        face = ifp == ifm ? (ifp | 4) : (ifp < ifm ? ifp : ifm + 8);
        ix = jm & (nside - 1);
        iy = nside - (jp & (nside - 1)) - 1;
    } else {  // caps
        const int64_t ntt = imin(3, (int64_t)tt);
        const double tp = tt - (double)ntt;
        const double tmp = fn * sqrt(3.0 * (1.0 - za));
        const int64_t jp = imin((int64_t)(tp * tmp), nside - 1);
        const int64_t jm = imin((int64_t)((1.0 - tp) * tmp), nside - 1);
        if (z > 0.0) {
            face = ntt, ix = nside - jm - 1, iy = nside - jp - 1;
        } else {
            face = ntt + 8, ix = jp, iy = jm;
        }
    }
    if (!nested) return ring_number(order, ring_position(order, face, ix, iy));
    return face * nside * nside + spread_bits(ix) + 2 * spread_bits(iy);
}

// Objects 0 .. n-1 of a pass. pix, counts and keys may each be null; nothing is stored outside [0, npix) of counts.
__global__ __launch_bounds__(WG) void k_pixels(int64_t n, const double *__restrict__ phi, const double *__restrict__ z, int order, int nested,
                                               int64_t npix, int64_t *__restrict__ pix, unsigned long long *__restrict__ counts,
                                               uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    int64_t p = loc2pix(order, nested, phi[i], z[i]);
    if (p < 0 || p >= npix) p = -1;
    if (pix) pix[i] = p;
    if (counts && p >= 0) atomicAdd(&counts[p], 1ull);
    if (keys) keys[i] = p >= 0 ? (uint32_t)p : (uint32_t)npix;  // npix < 2^(2 order + 4): invalid points sort behind every pixel
}

// keys ascending, w in the same order: the thread at the head of a run of one pixel adds the run to the map, in order.
__global__ __launch_bounds__(WG) void k_sum_runs(int64_t n, const uint32_t *__restrict__ keys, const double *__restrict__ w, uint32_t npix,
                                                 double *__restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k >= npix || (i > 0 && keys[i - 1] == k)) return;
    double s = map[k];
    for (int64_t j = i; j < n && keys[j] == k; ++j) s += w[j];
    map[k] = s;
}

__global__ __launch_bounds__(WG) void k_counts_to_f64(int64_t npix, double *map) {
    const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long c = reinterpret_cast<const unsigned long long *>(map)[i];
    map[i] = (double)c;
}

// ---- yawhip_healpix_pixels ----
constexpr double UNSEEN = -1.6375e30;  // healpy's sentinel of a pixel without data
constexpr int WAVES = WG / 64;

// The maps on the device and the nested pixels [q0, q_end) of one pass.
struct PixelPass {
    const double *__restrict__ values;
    const double *__restrict__ weights;  // may be null
    int order, nested;
    int64_t q0, q_end;
};

// The selection rule on entry `src` of the maps; v and wt are the values read (wt only with a weight map).
__device__ __forceinline__ bool pixel_selected(const PixelPass &m, int64_t src, double &v, double &wt) {
    v = m.values[src];
    if (!(fabs(v) < __builtin_huge_val()) || v == UNSEEN) return false;  // a NaN fails the comparison
    if (!m.weights) return true;
    wt = m.weights[src];
    return wt > 0.0 && wt < __builtin_huge_val();
}

// counts[workgroup] = selected pixels among the workgroup's WG nested pixels.
__global__ __launch_bounds__(WG) void k_select_count(PixelPass m, int64_t *__restrict__ counts) {
    __shared__ int s_cnt[WAVES];
    const int64_t q = m.q0 + (int64_t)blockIdx.x * WG + threadIdx.x;
    bool keep = false;
    if (q < m.q_end) {
        const int64_t src = m.nested ? q : ring_number(m.order, ring_position_nest(m.order, q));
        double v, wt;
        keep = pixel_selected(m, src, v, wt);
    }
    const unsigned long long mask = __ballot(keep);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < WAVES; ++w) total += s_cnt[w];
        counts[blockIdx.x] = total;
    }
}

// base[workgroup] = selected pixels of the pass before the workgroup's. Nothing is stored at or beyond `cap`.
__global__ __launch_bounds__(WG) void k_select_write(PixelPass m, double fact1, double fact2, const int64_t *__restrict__ base, int64_t cap,
                                                     int64_t *__restrict__ ipix, double *__restrict__ phi, double *__restrict__ z,
                                                     double *__restrict__ kappa, double *__restrict__ w) {
    __shared__ int s_cnt[WAVES];
    const int64_t q = m.q0 + (int64_t)blockIdx.x * WG + threadIdx.x;
    bool keep = false;
    int64_t src = 0;
    double v = 0.0, wt = 0.0;
    RingPos r{};
    if (q < m.q_end) {
        r = ring_position_nest(m.order, q);
        src = m.nested ? q : ring_number(m.order, r);
        keep = pixel_selected(m, src, v, wt);
    }
    const unsigned long long mask = __ballot(keep);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    if (!keep) return;
    int64_t at = base[blockIdx.x] + __popcll(mask & (((unsigned long long)1 << lane) - 1));
    for (int k = 0; k < wave; ++k) at += s_cnt[k];
    if (at >= cap) return;  // (cannot happen: the counts come from the same predicate on the same maps)
    ipix[at] = src;
    pixel_centre(m.order, r, fact1, fact2, phi[at], z[at]);
    kappa[at] = v;
    if (w) w[at] = wt;
}

hipError_t reserve(Workspace &ws, size_t chunk, bool sort_bufs, size_t npix) {
    hipError_t e = hipSuccess;
    if (chunk > ws.chunk_cap || (sort_bufs && !ws.sort_bufs)) {
        const size_t want = std::max(chunk, ws.chunk_cap);
        ws.chunk_cap = 0, ws.sort_bufs = false;
        const size_t want1 = std::max<size_t>(want, 1);  // (an empty pass still has its buffers)
        e = ws.cols.alloc(3 * want1);
        if (e == hipSuccess) e = ws.pix.alloc(want1);
        if (e == hipSuccess && sort_bufs) e = ws.keys.alloc(2 * want1);
        if (e == hipSuccess && sort_bufs) e = ws.w_sorted.alloc(want1);
        if (e != hipSuccess) return e;
        ws.chunk_cap = want, ws.sort_bufs = sort_bufs;
    }
    return ws.map.reserve(npix);
}

hipError_t reserve_tmp(Workspace &ws, size_t bytes) { return ws.tmp.reserve(bytes, bytes / 8 + 4096); }

// Buffers of yawhip_healpix_pixels: the uploaded maps (`src_count` values) and the outputs of a pass of `chunk` pixels.
hipError_t reserve_pixels(Workspace &ws, size_t src_count, size_t chunk) {
    hipError_t e = ws.src.reserve(src_count);
    if (e != hipSuccess) return e;
    if (chunk > ws.sel_cap) {
        ws.sel_cap = 0;
        e = ws.sel.alloc(4 * chunk);
        if (e == hipSuccess) e = ws.sel_pix.alloc(chunk);
        if (e == hipSuccess) e = ws.wg_counts.alloc(2 * (chunk / WG + 2));
        if (e != hipSuccess) return e;
        ws.sel_cap = chunk;
    }
    return e;
}

}  // namespace

size_t Workspace::bytes() const {
    return chunk_cap * (3 * sizeof(double) + sizeof(int64_t) + (sort_bufs ? 2 * sizeof(uint32_t) + sizeof(double) : 0)) + tmp.cap +
           map.cap * sizeof(double) + src.cap * sizeof(double) +
           (sel_cap ? sel_cap * (4 * sizeof(double) + sizeof(int64_t)) + 2 * (sel_cap / WG + 2) * sizeof(int64_t) : 0);
}

hipError_t healpix_map(Workspace &ws, hipStream_t stream, const MapCall &c) {
    const int64_t npix = (int64_t)12 << (2 * c.order);
    const bool weighted = c.map_out && c.w;
    const int64_t chunk = std::min(c.chunksize, c.n);
    hipError_t e = reserve(ws, (size_t)chunk, weighted, c.map_out ? (size_t)npix : 0);
    if (e != hipSuccess) return e;
    double *d_phi = ws.cols, *d_z = ws.cols + ws.chunk_cap, *d_w = ws.cols + 2 * ws.chunk_cap;
    uint32_t *keys_in = ws.keys, *keys_out = ws.keys + ws.chunk_cap;
    double *map = ws.map.ptr, *w_sorted = ws.w_sorted;  // (plain pointers: rocPRIM deduces its iterator types from the arguments)
    const unsigned end_bit = (unsigned)(2 * c.order + 4);
    if (c.map_out) e = hipMemsetAsync(map, 0, (size_t)npix * sizeof(double), stream);
    for (int64_t c0 = 0; c0 < c.n && e == hipSuccess; c0 += chunk) {
        const int64_t k = std::min(chunk, c.n - c0);
        e = hipMemcpyAsync(d_phi, c.phi + c0, (size_t)k * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_z, c.z + c0, (size_t)k * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && weighted) e = hipMemcpyAsync(d_w, c.w + c0, (size_t)k * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_pixels, dim3(grid_for(k)), dim3(WG), 0, stream, k, d_phi, d_z, (int)c.order, (int)c.nested, npix,
                           c.pix_out ? ws.pix : nullptr,
                           c.map_out && !weighted ? reinterpret_cast<unsigned long long *>(map) : nullptr,
                           weighted ? keys_in : nullptr);
        e = hipGetLastError();
        if (e == hipSuccess && weighted) {
            size_t bytes = 0;
            e = rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, d_w, w_sorted, (size_t)k, 0, end_bit, stream);
            if (e == hipSuccess) e = reserve_tmp(ws, bytes);
            if (e != hipSuccess) break;
            bytes = ws.tmp.cap;
            e = rocprim::radix_sort_pairs(ws.tmp.ptr, bytes, keys_in, keys_out, d_w, w_sorted, (size_t)k, 0, end_bit, stream);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(k_sum_runs, dim3(grid_for(k)), dim3(WG), 0, stream, k, keys_out, w_sorted, (uint32_t)npix, map);
            e = hipGetLastError();
        }
        if (e == hipSuccess && c.pix_out)
            e = hipMemcpyAsync(c.pix_out + c0, ws.pix, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess && c.map_out) {
        if (!weighted) {
            hipLaunchKernelGGL(k_counts_to_f64, dim3(grid_for(npix)), dim3(WG), 0, stream, npix, map);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(c.map_out, map, (size_t)npix * sizeof(double), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // nothing of this call is left in flight
    else (void)hipStreamSynchronize(stream);
    return e;
}

hipError_t healpix_pixels(Workspace &ws, hipStream_t stream, const PixelsCall &c, int64_t &selected, bool &overflow) {
    selected = 0, overflow = false;
    const int64_t npix = (int64_t)12 << (2 * c.order);
    const int64_t chunk = std::min(c.chunksize, npix);
    hipError_t e = reserve_pixels(ws, (size_t)npix * (c.weights ? 2 : 1), (size_t)chunk);
    if (e != hipSuccess) return e;
    double *d_values = ws.src.ptr, *d_weights = c.weights ? ws.src.ptr + npix : nullptr;
    double *d_phi = ws.sel, *d_z = ws.sel + ws.sel_cap, *d_kappa = ws.sel + 2 * ws.sel_cap, *d_w = c.weights ? ws.sel + 3 * ws.sel_cap : nullptr;
    int64_t *counts = ws.wg_counts, *base = ws.wg_counts + (ws.sel_cap / WG + 2);
    const double fact2 = 4.0 / (double)npix;                              // as randoms.pix2loc_nest
    const double fact1 = (double)((int64_t)2 << c.order) * fact2;
    e = hipMemcpyAsync(d_values, c.values, (size_t)npix * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && c.weights) e = hipMemcpyAsync(d_weights, c.weights, (size_t)npix * sizeof(double), hipMemcpyHostToDevice, stream);
    for (int64_t q0 = 0; q0 < npix && e == hipSuccess; q0 += chunk) {
        const int64_t k = std::min(chunk, npix - q0);
        const unsigned nb = grid_for(k);
        const PixelPass pass{d_values, d_weights, (int)c.order, (int)c.nested, q0, q0 + k};
        e = hipMemsetAsync(counts + nb, 0, sizeof(int64_t), stream);  // the entry whose scan is the pass's total
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_select_count, dim3(nb), dim3(WG), 0, stream, pass, counts);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        size_t bytes = 0;
        e = rocprim::exclusive_scan(nullptr, bytes, counts, base, (int64_t)0, (size_t)nb + 1, rocprim::plus<int64_t>(), stream);
        if (e == hipSuccess) e = reserve_tmp(ws, bytes);
        if (e != hipSuccess) break;
        bytes = ws.tmp.cap;
        e = rocprim::exclusive_scan(ws.tmp.ptr, bytes, counts, base, (int64_t)0, (size_t)nb + 1, rocprim::plus<int64_t>(), stream);
        int64_t total = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&total, base + nb, sizeof(int64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess || total == 0) continue;
        if (total < 0 || total > k || total > c.capacity - selected) {  // nothing of this pass is written
            overflow = true;
            break;
        }
        hipLaunchKernelGGL(k_select_write, dim3(nb), dim3(WG), 0, stream, pass, fact1, fact2, base, k, ws.sel_pix, d_phi, d_z, d_kappa, d_w);
        e = hipGetLastError();
        const size_t n8 = (size_t)total * sizeof(double);
        if (e == hipSuccess) e = hipMemcpyAsync(c.ipix_out + selected, ws.sel_pix, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c.phi_out + selected, d_phi, n8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c.z_out + selected, d_z, n8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(c.kappa_out + selected, d_kappa, n8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && d_w) e = hipMemcpyAsync(c.w_out + selected, d_w, n8, hipMemcpyDeviceToHost, stream);
        selected += total;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // nothing of this call is left in flight
    else (void)hipStreamSynchronize(stream);
    return e;
}

}  // namespace yawpix
