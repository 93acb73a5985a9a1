// Private to yawhip_shear_upload.hip and yawhip_shear.hip (the yawhip_shear_*, yawhip_dsigma_* and yawhip_proj_* calls of
// include/yawhip.h; DESIGN.md sections 15 to 26): the one handle that the first makes and the second counts on, and what the
// kernels see of it. Never installed, not part of the C ABI.
#ifndef YAWHIP_SHEAR_H
#define YAWHIP_SHEAR_H
#include <cstdint>
#include <vector>

#include "yawhip_internal.h"

#pragma GCC visibility push(hidden)  // (its destructor is not an export)
namespace yawhip_detail {
// What a handle is: set by the upload that made it, asked for by every count (require_kind; DESIGN.md section 21 has the
// table). One bit each: a count names the kinds it takes as a sum.
enum Kind : unsigned {
    SHEAR = 1,           // yawhip_shear_upload (nb == 1), yawhip_shear_upload_binned: the two columns are w g1, w g2
    DSIGMA_SOURCES = 2,  // yawhip_dsigma_upload_sources: an unbinned shear catalogue with the column u besides
    DSIGMA_LENSES = 4,   // yawhip_dsigma_upload_lenses: the two columns are f, c as they came
    RADIAL_LENSES = 8,   // yawhip_dsigma_upload_lenses_radial: such lenses with the column m besides
    PROJECTED = 16,      // yawhip_proj_upload: the two columns are d, c as they came
    PROJECTED_SHAPES = 32,  // yawhip_proj_upload_shapes: the two columns are w g1, w g2, with the columns d and c besides
};
}  // namespace yawhip_detail

// A catalogue resident on its context's device: the objects of every (patch, bin) segment sorted along `axis`.
struct yawhip_shear_sources {
    yawhip_ctx *ctx = nullptr;
    yawhip_detail::Kind kind = yawhip_detail::SHEAR;
    int64_t n = 0;
    int32_t n_patches = 0, nb = 1;
    int axis = 2;                               // coordinate the patch segments are sorted by (0 = x, 1 = y, 2 = z)
    yawhip_detail::DevPtr<double> x, y, z, w;   // w may be null (every weight 1.0)
    yawhip_detail::DevPtr<double> wg1, wg2;     // the kind's two columns (a, b); the products w * g1, w * g2 each rounded on its own
    yawhip_detail::DevPtr<double> extra, extra2;  // what a kind has besides; a count reads them through the view of its kind:
    //   DSIGMA_SOURCES    extra = u
    //   RADIAL_LENSES     extra = m
    //   PROJECTED_SHAPES  extra = d, extra2 = c
    std::vector<double> least;                  // RADIAL_LENSES, PROJECTED, PROJECTED_SHAPES: least m or d per redshift bin over all patches [nb] (+inf: none)
    yawhip_detail::DevPtr<int64_t> off;         // [P * nb + 1]
    std::vector<int64_t> h_off;                 // the same on the host
    // per-call buffers of the counts (grow-only; a count over jobs uses those of its sources, one over cells those of its first handle)
    yawhip_detail::DevBuf<unsigned char> d_in;  // thresholds, window half widths, jobs or cells
    yawhip_detail::DevBuf<double> d_out;        // [planes][cells][E-1] sums, then [cells] evaluated pairs (64-bit integers)
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

struct ShapeView : ShearView {  // a shape handle streamed by yawhip_proj_count_shapes: wg1, wg2 are w g1, w g2, with d, c besides
    const double *d, *c;
};

}  // namespace yawhip_detail

#pragma GCC visibility pop
#endif
