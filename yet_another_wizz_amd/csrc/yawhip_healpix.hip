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
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "yawhip_healpix.h"

namespace yawpix {

namespace {

constexpr int WG = 256;
constexpr double TWOPI = 0x1.921fb54442d18p+2;   // numpy's 2 pi
constexpr double HALFPI = 0x1.921fb54442d18p+0;  // numpy's pi / 2
constexpr double TWOTHIRD = 2.0 / 3.0;

__device__ __forceinline__ int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }

// bits 0 .. 13 of v moved to the even positions 0, 2, .. 26
__device__ __forceinline__ int64_t spread_bits(int64_t v) {
    uint64_t x = (uint64_t)v;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return (int64_t)x;
}

// Ring-scheme number of the pixel (face, ix, iy) of `order`: the integer steps of randoms._ring_position / nest2ring.
__device__ __forceinline__ int64_t ring_number(int order, int64_t face, int64_t ix, int64_t iy) {
    const int64_t nside = (int64_t)1 << order;
    const int64_t jrll = 2 + (face >> 2);                                          // 2 2 2 2 3 3 3 3 4 4 4 4
    const int64_t jpll = (int64_t)((0x753164207531ull >> (4 * (face & 15))) & 7);  // 1 3 5 7 0 2 4 6 1 3 5 7
    const int64_t jr = (jrll << order) - ix - iy - 1;                              // ring, 1 .. 4 nside - 1 from the north
    const bool north = jr < nside, south = jr > 3 * nside;
    const int64_t nr = north ? jr : (south ? 4 * nside - jr : nside);
    const int64_t kshift = (north || south) ? 0 : ((jr - nside) & 1);
    int64_t jp = (jpll * nr + ix - iy + 1 + kshift) / 2;  // the sum is even
    if (jp > 4 * nside) jp -= 4 * nside;
    if (jp < 1) jp += 4 * nside;
    if (north) return 2 * jr * (jr - 1) + jp - 1;
    if (south) return 12 * nside * nside - 2 * nr * (nr + 1) + jp - 1;
    return 2 * nside * (nside - 1) + (jr - nside) * (4 * nside) + jp - 1;
}

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
    if (!nested) return ring_number(order, face, ix, iy);
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

inline unsigned grid_for(int64_t n) { return (unsigned)((n + WG - 1) / WG); }

template <typename T>
hipError_t regrow(T *&p, size_t count) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T));
}

hipError_t reserve(Workspace &ws, size_t chunk, bool sort_bufs, size_t npix) {
    hipError_t e = hipSuccess;
    if (chunk > ws.chunk_cap || (sort_bufs && !ws.sort_bufs)) {
        const size_t want = std::max(chunk, ws.chunk_cap);
        ws.chunk_cap = 0, ws.sort_bufs = false;
        e = regrow(ws.cols, 3 * want);
        if (e == hipSuccess) e = regrow(ws.pix, want);
        if (e == hipSuccess && sort_bufs) e = regrow(ws.keys, 2 * want);
        if (e == hipSuccess && sort_bufs) e = regrow(ws.w_sorted, want);
        if (e != hipSuccess) return e;
        ws.chunk_cap = want, ws.sort_bufs = sort_bufs;
    }
    if (npix > ws.map_cap) {
        ws.map_cap = 0;
        e = regrow(ws.map, npix);
        if (e == hipSuccess) ws.map_cap = npix;
    }
    return e;
}

hipError_t reserve_tmp(Workspace &ws, size_t bytes) {
    if (bytes <= ws.tmp_bytes) return hipSuccess;
    if (ws.tmp) (void)hipFree(ws.tmp);
    ws.tmp = nullptr;
    ws.tmp_bytes = 0;
    const size_t want = bytes + bytes / 8 + 4096;
    const hipError_t e = hipMalloc(&ws.tmp, want);
    if (e == hipSuccess) ws.tmp_bytes = want;
    return e;
}

}  // namespace

size_t Workspace::bytes() const {
    return chunk_cap * (3 * sizeof(double) + sizeof(int64_t) + (sort_bufs ? 2 * sizeof(uint32_t) + sizeof(double) : 0)) + tmp_bytes +
           map_cap * sizeof(double);
}

void Workspace::release() {
    if (cols) (void)hipFree(cols);
    if (pix) (void)hipFree(pix);
    if (keys) (void)hipFree(keys);
    if (w_sorted) (void)hipFree(w_sorted);
    if (tmp) (void)hipFree(tmp);
    if (map) (void)hipFree(map);
    *this = Workspace{};
}

hipError_t healpix_map(Workspace &ws, hipStream_t stream, const MapCall &c) {
    const int64_t npix = (int64_t)12 << (2 * c.order);
    const bool weighted = c.map_out && c.w;
    const int64_t chunk = std::min(c.chunksize, c.n);
    hipError_t e = reserve(ws, (size_t)chunk, weighted, c.map_out ? (size_t)npix : 0);
    if (e != hipSuccess) return e;
    double *d_phi = ws.cols, *d_z = ws.cols + ws.chunk_cap, *d_w = ws.cols + 2 * ws.chunk_cap;
    uint32_t *keys_in = ws.keys, *keys_out = ws.keys + ws.chunk_cap;
    const unsigned end_bit = (unsigned)(2 * c.order + 4);
    if (c.map_out) e = hipMemsetAsync(ws.map, 0, (size_t)npix * sizeof(double), stream);
    for (int64_t c0 = 0; c0 < c.n && e == hipSuccess; c0 += chunk) {
        const int64_t k = std::min(chunk, c.n - c0);
        e = hipMemcpyAsync(d_phi, c.phi + c0, (size_t)k * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_z, c.z + c0, (size_t)k * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && weighted) e = hipMemcpyAsync(d_w, c.w + c0, (size_t)k * sizeof(double), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_pixels, dim3(grid_for(k)), dim3(WG), 0, stream, k, d_phi, d_z, (int)c.order, (int)c.nested, npix,
                           c.pix_out ? ws.pix : nullptr,
                           c.map_out && !weighted ? reinterpret_cast<unsigned long long *>(ws.map) : nullptr,
                           weighted ? keys_in : nullptr);
        e = hipGetLastError();
        if (e == hipSuccess && weighted) {
            size_t bytes = 0;
            e = rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, d_w, ws.w_sorted, (size_t)k, 0, end_bit, stream);
            if (e == hipSuccess) e = reserve_tmp(ws, bytes);
            if (e != hipSuccess) break;
            bytes = ws.tmp_bytes;
            e = rocprim::radix_sort_pairs(ws.tmp, bytes, keys_in, keys_out, d_w, ws.w_sorted, (size_t)k, 0, end_bit, stream);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(k_sum_runs, dim3(grid_for(k)), dim3(WG), 0, stream, k, keys_out, ws.w_sorted, (uint32_t)npix, ws.map);
            e = hipGetLastError();
        }
        if (e == hipSuccess && c.pix_out)
            e = hipMemcpyAsync(c.pix_out + c0, ws.pix, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess && c.map_out) {
        if (!weighted) {
            hipLaunchKernelGGL(k_counts_to_f64, dim3(grid_for(npix)), dim3(WG), 0, stream, npix, ws.map);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(c.map_out, ws.map, (size_t)npix * sizeof(double), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // nothing of this call is left in flight
    else (void)hipStreamSynchronize(stream);
    return e;
}

}  // namespace yawpix
