// yawhip_shear_upload.hip -- the uploads of the handle that the shear, lensing and projected counts of yawhip_shear.hip take
// (yawhip_shear_sources, yawhip_shear.h): seven entry points, one per kind of handle and one more for the binned shear
// catalogue, over one upload_segments; and yawhip_shear_free. include/yawhip.h has the contracts. Nothing here knows a count.
//
//   k_gather_shear   the upload's one gather: columns into the order of the segment sort, with the two products (a lens
//                    handle keeps its two columns f, c as they came).
//   k_gather_column  the same gather of the sources' column u, of a radial lens handle's column m and of a shape handle's d, c.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>

#include "yawhip_shear.h"

using namespace yawhip_detail;

namespace {

__global__ void k_gather_shear(int64_t n, const uint32_t *__restrict__ perm, const double *__restrict__ sx,
                               const double *__restrict__ sy, const double *__restrict__ sz, const double *__restrict__ sw,
                               const double *__restrict__ sg1, const double *__restrict__ sg2, double *__restrict__ x,
                               double *__restrict__ y, double *__restrict__ z, double *__restrict__ w, double *__restrict__ wg1,
                               double *__restrict__ wg2, bool products) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = perm[i];
    x[i] = sx[j];
    y[i] = sy[j];
    z[i] = sz[j];
    const double g1 = sg1[j], g2 = sg2[j];
    if (sw) {
        const double wj = sw[j];
        w[i] = wj;
        wg1[i] = products ? wj * g1 : g1;
        wg2[i] = products ? wj * g2 : g2;
    } else {
        wg1[i] = g1;
        wg2[i] = g2;
    }
}

__global__ void k_gather_column(int64_t n, const uint32_t *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// The upload of every entry point: a handle of `kind` with n_bins segments per patch, each sorted along sort_axis and
// gathered. a, b: the kind's two columns, gathered as the products w a, w b for the two kinds of shear catalogue and as they
// came for the others; extra: the column u of DSIGMA_SOURCES, m of RADIAL_LENSES or d of PROJECTED_SHAPES, else NULL; extra2:
// the column c of PROJECTED_SHAPES, else NULL
int upload_segments(const char *fn, Kind kind, yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                    const double *w, const double *a, const double *b, const double *extra, const double *extra2, int32_t n_patches,
                    int32_t n_bins, const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out) {
    if (!out) return fail(YAWHIP_ERR_INVALID, "%s: out is NULL", fn);
    *out = nullptr;
    if (!ctx) return fail(YAWHIP_ERR_INVALID, "%s: ctx is NULL", fn);
    if (sort_axis < 0 || sort_axis > 2) return fail(YAWHIP_ERR_INVALID, "sort_axis must be 0 (x), 1 (y) or 2 (z)");
    if (n < 0 || n_patches <= 0 || n_bins <= 0 || !offsets || (n > 0 && (!x || !y || !z || !a || !b)))
        return fail(YAWHIP_ERR_INVALID, "%s: bad sizes or NULL columns", fn);
    if (n >= (1ll << 32)) return fail(YAWHIP_ERR_INVALID, "at most 2^32 - 1 objects per catalogue");
    const int64_t n_seg = (int64_t)n_patches * n_bins;
    if (offsets[0] != 0 || offsets[n_seg] != n) return fail(YAWHIP_ERR_INVALID, "offsets must start at 0 and end at n");
    for (int64_t i = 0; i < n_seg; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(YAWHIP_ERR_INVALID, "offsets must be non-decreasing");
    HIP_TRY(hipSetDevice(ctx->device));
    yawhip_shear_sources *s = new (std::nothrow) yawhip_shear_sources;
    if (!s) return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    s->ctx = ctx;
    s->kind = kind;
    s->n = n;
    s->n_patches = n_patches;
    s->nb = n_bins;
    s->axis = sort_axis;
    // the kinds counted in a radius keep the least entry per redshift bin of the column that bounds their reach (chord_reach)
    const bool has_least = (kind & (RADIAL_LENSES | PROJECTED | PROJECTED_SHAPES)) != 0;
    const double *scale = kind == PROJECTED ? a : extra;
    try {
        s->h_off.assign(offsets, offsets + n_seg + 1);
        if (has_least) s->least.assign((size_t)n_bins, INFINITY);  // (n == 0: the column may be NULL, and no segment reads it)
    } catch (const std::bad_alloc &) {
        delete s;
        return fail(YAWHIP_ERR_OOM, "%s: out of host memory", fn);
    }
    for (int64_t seg = 0; has_least && seg < n_seg; ++seg)
        for (int64_t i = offsets[seg]; i < offsets[seg + 1]; ++i)
            s->least[(size_t)(seg % n_bins)] = std::min(s->least[(size_t)(seg % n_bins)], scale[i]);
    DevPtr<double> *const d_extra = (kind & (DSIGMA_SOURCES | RADIAL_LENSES | PROJECTED_SHAPES)) ? &s->extra : nullptr;
    DevPtr<double> *const d_extra2 = kind == PROJECTED_SHAPES ? &s->extra2 : nullptr;
    const size_t n1 = (size_t)std::max<int64_t>(n, 1), col = (size_t)n * sizeof(double);
    constexpr int NC = 8;
    DevPtr<double> raw[NC];  // x, y, z, a, b, w, extra, extra2 as they came (temporary)
    const double *host[NC] = {x, y, z, a, b, w, extra, extra2};
    DevPtr<uint32_t> perm;
    hipError_t e = hipSuccess;
    for (DevPtr<double> *c : {&s->x, &s->y, &s->z, &s->wg1, &s->wg2})
        if (e == hipSuccess) e = c->alloc(n1);
    if (e == hipSuccess && w) e = s->w.alloc(n1);
    if (e == hipSuccess && d_extra) e = d_extra->alloc(n1);  // (an empty handle of the kind has the column too)
    if (e == hipSuccess && d_extra2) e = d_extra2->alloc(n1);
    if (e == hipSuccess) e = s->off.alloc((size_t)n_seg + 1);
    for (int c = 0; c < NC; ++c)
        if (e == hipSuccess && host[c]) e = raw[c].alloc(n1);
    if (e == hipSuccess) e = perm.alloc(n1);
    for (int c = 0; c < NC; ++c)
        if (e == hipSuccess && host[c] && n > 0) e = hipMemcpyAsync(raw[c], host[c], col, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->off, offsets, ((size_t)n_seg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && n > 0) {
        e = yawsort::sort_segments(ctx->sort_ws, ctx->stream, n, key_of(raw[0], raw[1], raw[2], sort_axis), s->off, n_seg, perm);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_gather_shear, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, perm, raw[0], raw[1], raw[2], raw[5],
                               raw[3], raw[4], s->x, s->y, s->z, s->w, s->wg1, s->wg2,
                               (kind & (SHEAR | DSIGMA_SOURCES | PROJECTED_SHAPES)) != 0);
            e = hipGetLastError();
        }
        if (e == hipSuccess && d_extra) {
            hipLaunchKernelGGL(k_gather_column, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, perm, raw[6], *d_extra);
            e = hipGetLastError();
        }
        if (e == hipSuccess && d_extra2) {
            hipLaunchKernelGGL(k_gather_column, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, perm, raw[7], *d_extra2);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (ctx->sort_ws.cap > ((size_t)1 << 25)) ctx->sort_ws.release();  // as the catalogue upload: keep only small workspaces
    if (e != hipSuccess) {
        yawhip_shear_free(s);
        return hip_fail(fn, e);
    }
    *out = s;
    return YAWHIP_OK;
}

// a column of an upload beyond the coordinates: every entry a finite number, and of the rule's sign
enum Rule { NOT_NEGATIVE, POSITIVE, ANY_SIGN };

int check_column(const char *fn, const char *name, int64_t n, const double *v, Rule rule) {
    static const char *const WANTED[] = {"a finite number >= 0", "a finite number > 0", "a finite number"};
    if (n > 0 && !v) return fail(YAWHIP_ERR_INVALID, "%s: column %s is NULL", fn, name);
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || (rule == NOT_NEGATIVE && !(v[i] >= 0.0)) || (rule == POSITIVE && !(v[i] > 0.0)))
            return fail(YAWHIP_ERR_INVALID, "%s: column %s has an entry that is not %s (index %lld)", fn, name, WANTED[rule], (long long)i);
    return YAWHIP_OK;
}

}  // namespace

extern "C" {

int yawhip_shear_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                        const double *g1, const double *g2, int32_t n_patches, const int64_t *offsets, int32_t sort_axis,
                        yawhip_shear_sources **out) {
    return upload_segments("yawhip_shear_upload", SHEAR, ctx, n, x, y, z, w, g1, g2, nullptr, nullptr, n_patches, 1, offsets, sort_axis, out);
}

int yawhip_shear_upload_binned(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                               const double *g1, const double *g2, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                               int32_t sort_axis, yawhip_shear_sources **out) {
    return upload_segments("yawhip_shear_upload_binned", SHEAR, ctx, n, x, y, z, w, g1, g2, nullptr, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_dsigma_upload_sources(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                 const double *g1, const double *g2, const double *u, int32_t n_patches, const int64_t *offsets,
                                 int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_dsigma_upload_sources";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "u", n, u, NOT_NEGATIVE)) return rc;
    return upload_segments(fn, DSIGMA_SOURCES, ctx, n, x, y, z, w, g1, g2, u, nullptr, n_patches, 1, offsets, sort_axis, out);
}

int yawhip_dsigma_upload_lenses(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                const double *f, const double *c, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                                int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_dsigma_upload_lenses";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "f", n, f, NOT_NEGATIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, NOT_NEGATIVE)) return rc;
    return upload_segments(fn, DSIGMA_LENSES, ctx, n, x, y, z, w, f, c, nullptr, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_dsigma_upload_lenses_radial(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                       const double *f, const double *c, const double *m, int32_t n_patches, int32_t n_bins,
                                       const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_dsigma_upload_lenses_radial";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "f", n, f, NOT_NEGATIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, NOT_NEGATIVE)) return rc;
    if (const int rc = check_column(fn, "m", n, m, POSITIVE)) return rc;
    return upload_segments(fn, RADIAL_LENSES, ctx, n, x, y, z, w, f, c, m, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_proj_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                       const double *d, const double *c, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                       int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_proj_upload";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "d", n, d, POSITIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, ANY_SIGN)) return rc;
    return upload_segments(fn, PROJECTED, ctx, n, x, y, z, w, d, c, nullptr, nullptr, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_proj_upload_shapes(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                              const double *g1, const double *g2, const double *d, const double *c, int32_t n_patches, int32_t n_bins,
                              const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out) {
    const char *fn = "yawhip_proj_upload_shapes";
    if (out) *out = nullptr;
    if (const int rc = check_column(fn, "g1", n, g1, ANY_SIGN)) return rc;
    if (const int rc = check_column(fn, "g2", n, g2, ANY_SIGN)) return rc;
    if (const int rc = check_column(fn, "d", n, d, POSITIVE)) return rc;
    if (const int rc = check_column(fn, "c", n, c, ANY_SIGN)) return rc;
    return upload_segments(fn, PROJECTED_SHAPES, ctx, n, x, y, z, w, g1, g2, d, c, n_patches, n_bins, offsets, sort_axis, out);
}

int yawhip_shear_free(yawhip_shear_sources *src) {
    if (!src) return YAWHIP_OK;
    if (src->ctx) {
        (void)hipSetDevice(src->ctx->device);
        if (src->ctx->stream) (void)hipStreamSynchronize(src->ctx->stream);
    }
    delete src;  // its device memory goes with it
    return YAWHIP_OK;
}

}  // extern "C"
