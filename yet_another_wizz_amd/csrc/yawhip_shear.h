// Private to yawhip_shear.hip (tangential shear, shear-shear and excess-surface-density counts, yawhip_shear_* and
// yawhip_dsigma_* and yawhip_proj_*, include/yawhip.h; DESIGN.md sections 15 to 20): the source handle and what its kernels see of it. Never
// installed, not part of the C ABI.
#ifndef YAWHIP_SHEAR_H
#define YAWHIP_SHEAR_H
#include <cstdint>
#include <vector>

#include "yawhip_internal.h"

#pragma GCC visibility push(hidden)  // (its destructor is not an export)

// A shear catalogue resident on its context's device: the objects of every (patch, bin) segment sorted along `axis`; nb == 1
// (yawhip_shear_upload) is the unbinned catalogue of yawhip_shear_count, nb redshift bins that of yawhip_shear_auto_count and
// of yawhip_shear_pair_count. A handle of yawhip_dsigma_upload_sources is an unbinned one with the column u besides; one of
// yawhip_dsigma_upload_lenses (`lenses`) holds the lens columns f, c, as they came, in the place of wg1, wg2: only
// yawhip_dsigma_count takes it. One of yawhip_dsigma_upload_lenses_radial is such a lens handle with the column m besides
// (the squared transverse distance per radian of every lens), which yawhip_dsigma_count_radial bins by. One of
// yawhip_proj_upload (`projected`) is a lens handle whose two raw columns are d, c (transverse distance per radian and
// line-of-sight coordinate of every object): only yawhip_proj_count takes it.
struct yawhip_shear_sources {
    yawhip_ctx *ctx = nullptr;
    int64_t n = 0;
    int32_t n_patches = 0;
    int32_t nb = 1;
    int axis = 2;                               // coordinate the patch segments are sorted by (0 = x, 1 = y, 2 = z)
    yawhip_detail::DevPtr<double> x, y, z, w;   // w may be null (every weight 1.0)
    yawhip_detail::DevPtr<double> wg1, wg2;     // w * g1, w * g2, each product rounded on its own (g1, g2 without weights)
    yawhip_detail::DevPtr<double> u;            // the sources' column of yawhip_dsigma_count, or null
    bool lenses = false;                        // a lens handle: wg1, wg2 hold f, c
    yawhip_detail::DevPtr<double> m;            // a radial lens handle: the lenses' column m in segment order, or null
    std::vector<double> min_m;                  // ... and its minimum per redshift bin over all patches [nb] (+inf: no lens)
    bool projected = false;                     // a handle of yawhip_proj_upload: a lens handle whose wg1, wg2 hold d, c
    std::vector<double> min_d;                  // ... and the minimum of d per redshift bin over all patches [nb] (+inf: none)
    yawhip_detail::DevPtr<int64_t> off;         // [P * nb + 1]
    std::vector<int64_t> h_off;
    // per-call buffers of the counts (grow-only; yawhip_shear_pair_count uses those of its first handle)
    yawhip_detail::DevBuf<unsigned char> d_in;  // thresholds, window half widths, jobs or cells
    yawhip_detail::DevBuf<double> d_out;        // [3 or 4][cells][E-1] sums, then [cells] evaluated pairs (64-bit integers)
};

namespace yawhip_detail {

struct ShearView {
    const double *x, *y, *z, *w;  // w may be null
    const double *wg1, *wg2;
    const int64_t *off;           // [P * nb + 1]
    const double *key;            // the column the segments are sorted by
    int axis;
};

struct LensView : ShearView {  // a lens handle streamed by yawhip_dsigma_count: wg1, wg2 are f, c
    int nb;
};

struct RadialView : LensView {  // a radial lens handle streamed by yawhip_dsigma_count_radial
    const double *m;
};

struct SourceView : ShearView {  // the sources of yawhip_dsigma_count in the lanes
    const double *u;
};

}  // namespace yawhip_detail

#pragma GCC visibility pop
#endif
