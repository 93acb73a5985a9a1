// HEALPix integer and pixel-centre arithmetic on the device, shared by yawhip_healpix.hip (pixels and maps of a catalogue,
// the pixels of a scalar map) and yawhip_random.hip (HealPixRandoms, at order 29). The integer steps are those of
// randoms._ring_position / randoms.nest2ring and the float64 steps those of randoms.pix2loc_nest, each one IEEE operation
// in the written order: the build contracts nothing (-ffp-contract=off), so the device repeats the host route bit for bit.
#ifndef YAWHIP_HEALPIX_MATH_H
#define YAWHIP_HEALPIX_MATH_H
#include <hip/hip_runtime.h>

#include <cstdint>

namespace yawpix {

constexpr double TWOPI = 0x1.921fb54442d18p+2;   // numpy's 2 pi
constexpr double HALFPI = 0x1.921fb54442d18p+0;  // numpy's pi / 2

// bits 0 .. 13 of v moved to the even positions 0, 2, .. 26
__device__ __forceinline__ int64_t spread_bits(int64_t v) {
    uint64_t x = (uint64_t)v;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return (int64_t)x;
}

// every second bit of v (bits 0, 2, 4, ...), packed
__device__ __forceinline__ int64_t even_bits(uint64_t v) {
    v &= 0x5555555555555555ull;
    v = (v | (v >> 1)) & 0x3333333333333333ull;
    v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
    v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
    v = (v | (v >> 16)) & 0x00000000ffffffffull;
    return (int64_t)v;
}

// Where the pixel (face, ix, iy) of `order` lies in the ring scheme: the integer steps of randoms._ring_position.
struct RingPos {
    int64_t jr, nr, kshift, jp;  // ring (1 .. 4 nside - 1 from the north), its pixels per quadrant, 1 on belt rings that start at
    bool north, south;           // phi = 0, position in the ring (1 .. 4 nr); the caps
};

__device__ __forceinline__ RingPos ring_position(int order, int64_t face, int64_t ix, int64_t iy) {
    const int64_t nside = (int64_t)1 << order;
    const int64_t jrll = 2 + (face >> 2);                                          // 2 2 2 2 3 3 3 3 4 4 4 4
    const int64_t jpll = (int64_t)((0x753164207531ull >> (4 * (face & 15))) & 7);  // 1 3 5 7 0 2 4 6 1 3 5 7
    RingPos r;
    r.jr = (jrll << order) - ix - iy - 1;
    r.north = r.jr < nside, r.south = r.jr > 3 * nside;
    r.nr = r.north ? r.jr : (r.south ? 4 * nside - r.jr : nside);
    r.kshift = (r.north || r.south) ? 0 : ((r.jr - nside) & 1);
    r.jp = (jpll * r.nr + ix - iy + 1 + r.kshift) / 2;  // the sum is even
    if (r.jp > 4 * nside) r.jp -= 4 * nside;
    if (r.jp < 1) r.jp += 4 * nside;
    return r;
}

__device__ __forceinline__ RingPos ring_position_nest(int order, int64_t q) {  // of the nested pixel q
    const uint64_t low = (uint64_t)q & (((uint64_t)1 << (2 * order)) - 1);
    return ring_position(order, q >> (2 * order), even_bits(low), even_bits(low >> 1));
}

// Ring-scheme number of a pixel of `order` at `r`: the integer steps of randoms.nest2ring.
__device__ __forceinline__ int64_t ring_number(int order, const RingPos &r) {
    const int64_t nside = (int64_t)1 << order;
    if (r.north) return 2 * r.jr * (r.jr - 1) + r.jp - 1;
    if (r.south) return 12 * nside * nside - 2 * r.nr * (r.nr + 1) + r.jp - 1;
    return 2 * nside * (nside - 1) + (r.jr - nside) * (4 * nside) + r.jp - 1;
}

// Centre of the pixel of `order` at `r`, phi and z = cos(theta): the float64 steps of randoms.pix2loc_nest, each rounded on
// its own. fact2 = 4 / npix and fact1 = 2 nside * fact2, computed by the caller as the host computes them.
__device__ __forceinline__ void pixel_centre(int order, const RingPos &r, double fact1, double fact2, double &phi, double &z) {
    const int64_t nside = (int64_t)1 << order;
    const double nrf = (double)r.nr;
    const double tmp = nrf * nrf * fact2;
    z = r.north ? 1.0 - tmp : (r.south ? tmp - 1.0 : (double)(2 * nside - r.jr) * fact1);
    phi = ((double)r.jp - (double)(r.kshift + 1) * 0.5) * (HALFPI / nrf);
}

}  // namespace yawpix
#endif
