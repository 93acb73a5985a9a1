// yawhip_count.hip -- the count call behind yawhip_count_pairs and yawhip_job_work (include/yawhip.h), host code only:
//   * the argument checks (check_call) and the key a plan is kept under (CallKey);
//   * the plan (HostPlan, made by make_plan in the six steps of Planner): what a call derives from its inputs before
//     anything is launched -- kernel family and variant, layouts, tile and stage sizes, LDS, the tables of the item builder
//     and the count kernel -- kept for the next call with the same inputs;
//   * count_enqueue, which puts a call on the context's stream -- plan look-up, result block, item builder, count kernel(s),
//     reductions, tail -- and count_finish, which waits for it and hands over results and statistics; run_single cuts a job
//     list in halves where one call cannot take it, yawhip_count_pairs splits it over the devices of a context.
// No kernel is defined here. The kernels and the functions that launch them are the kernel units' (yawhip.hip and
// yawhip_kernel_*.hip, one per kernel family); yawhip_count_kernels.h is the interface between them and this unit: the
// geometry a plan reasons about, the counter block count_finish reads, and the launch record (CountLaunch) count_enqueue
// fills. Experiment flags (-D) of a variant build do not reach this unit.
// DESIGN.md sections 4 and 5 have the reasons and the measurements.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <numeric>
#include <utility>
#include <vector>

#include "yawhip_count_kernels.h"

using namespace yawhip_detail;

namespace {
inline DevTab make_tab(const double *x, const double *y, const double *z, const double *w, const int32_t *k, const int64_t *off,
                       const int64_t *vbase, const int64_t *slo, const int64_t *tiles, const TileRec *tile_rec, const RunGrid *grid,
                       int axis, const float *q = nullptr, int64_t q_stride = 0, const int32_t *idx = nullptr,
                       const LaneObj *q4 = nullptr) {
    return DevTab{(gf64p)x, (gf64p)y, (gf64p)z, (gf64p)w, (gi32p)k, (gi64p)off, (gi64p)vbase, (gi64p)slo, (gi64p)tiles,
                  tile_rec, grid, (gf32p)q, (gf32p)(q ? q + q_stride : nullptr), (gf32p)(q ? q + 2 * q_stride : nullptr), (glanep)q4,
                  (gi32p)idx, (gi32p)nullptr, axis, 0};
}

inline int64_t seg_len(const yawhip_catalog *c, int patch, int k) {
    const int kk = c->nb == 1 ? 0 : k;
    const int64_t i = (int64_t)patch * c->nb + kk;
    return c->h_off[i + 1] - c->h_off[i];
}

// the variant of a call from those of its pieces: pieces that launched none do not count, different ones make it mixed
int32_t merge_variant(int32_t a, int32_t b) { return a == 0 || a == b ? b : (b == 0 ? a : YAWHIP_VARIANT_MIXED); }

// Float32 bounds of every edge for k_count_band32 (see there): for unit vectors rounded to float32,
//   |s32 - s| <= g(t) = 2.1e-7 sqrt(t) + 5e-7 t + 1e-12 near s = t,
// so s32 < t - g proves s <= t and s32 > t + g proves s > t; in between the kernel evaluates in float64.
//   n_edges == 2: {c, h_in, h_out, 0}: |s32 - c| < h_in proves t0 < s <= t1, |s32 - c| >= h_out proves the opposite
//                 (s32 - c is what the kernel's three fused multiply-adds deliver; both widths carry their rounding);
//   else per edge {t - g rounded down, t + g rounded up}.
std::vector<float> build_thr32(const double *t, int n_bins, int n_edges) {
    auto down = [](double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; };
    auto up = [](double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; };
    auto guard = [](double te) { return BAND32_GUARD_SQRT * std::sqrt(te) + 5e-7 * te + 1e-12; };
    const int tw = thr32_width(n_edges);
    std::vector<float> out((size_t)n_bins * tw, 0.f);
    for (int k = 0; k < n_bins; ++k) {
        const double *tk = t + (size_t)k * n_edges;
        float *row = &out[(size_t)k * tw];
        if (n_edges == 2) {
            const double g0 = guard(tk[0]), g1 = guard(tk[1]);
            const float c = (float)(0.5 * (tk[0] + tk[1]));
            const double cd = (double)c;
            // q = fma(dz, dz, fma(dy, dy, fma(dx, dx, -c))): three roundings of intermediate sums that stay below 2 c wherever
            // a class is claimed (|q| < h_in <= c, or s inside the annulus: s32 <= t1 + g1 <= 2 c) -> 6 x 2^-24 x c = 3.6e-7 c
            const double fold = 4e-7 * cd;
            const double h_in = (std::min(cd - (tk[0] + g0), (tk[1] - g1) - cd) - fold) * (1.0 - 1e-6);
            const double h_out = (std::max(cd - (tk[0] - g0), (tk[1] + g1) - cd) + fold) * (1.0 + 1e-6);
            row[0] = c;
            row[1] = h_in > 0.0 ? down(h_in) : 0.f;   // |q| < 0 never holds: nothing is certain
            row[2] = up(std::max(h_out, 0.0));
            row[3] = 0.f;
        } else {
            for (int e = 0; e < n_edges; ++e) {
                const double g = guard(tk[e]);
                row[2 * e] = down(tk[e] - g);
                row[2 * e + 1] = up(tk[e] + g);
            }
        }
    }
    return out;
}

// Float32 table of k_count_band32_fine (see there), one row per redshift bin: {m, a, e0, e1}, then {t_j - g, t_j + g} per edge.
// Empty when the edges of some bin do not follow the log-spaced model closely enough for float32 (the caller then counts
// with the float64 band kernel): deviation above 0.05 fine bins, a guard wider than a fifth of a fine bin, t_0 = 0.
std::vector<float> build_fine32(const double *t, int n_bins, int n_edges) {
    auto down = [](double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; };
    auto up = [](double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; };
    auto guard = [](double te) { return BAND32_GUARD_SQRT * std::sqrt(te) + 5e-7 * te + 1e-12; };
    const int tw = fine32_width(n_edges), nf = n_edges - 1;
    std::vector<float> out((size_t)n_bins * tw, 0.f);
    for (int k = 0; k < n_bins; ++k) {
        const double *tk = t + (size_t)k * n_edges;
        if (!(tk[0] > 1e-12) || !(tk[nf] > tk[0])) return {};
        const double l0 = std::log2(tk[0]), l1 = std::log2(tk[nf]);
        const double m = (double)nf / (l1 - l0), a = l0 * m;
        double dev = 0.0;
        for (int j = 0; j <= nf; ++j) {
            if (j > 0 && !(tk[j] > tk[j - 1])) return {};
            dev = std::max(dev, std::fabs((std::log2(tk[j]) - l0) * m - (double)j));
        }
        // error of the device's f: hardware log2 (1 ulp of a result below 64), float32 images of m and a, the fma
        const double dev_f = m * (1e-5 + 6e-8 * 64.0) + 2.0 * 6e-8 * std::fabs(a) + 4e-5 + 6e-8 * (nf + 2);
        const double per_s = 1.05 * m / std::log(2.0);  // d f / (d s / s), with room for the second order
        // Admission: an s32 between the guard bands of edges j and j + 1 must round to one of the two, i.e. f may be off by
        // less than half a bin: the model's deviation at the edges, the device's arithmetic, and the guard (widest,
        // relative to t, at the first edge).
        if (dev + dev_f + per_s * guard(tk[0]) / tk[0] > 0.45) return {};
        float *row = &out[(size_t)k * tw];
        row[0] = (float)m; row[1] = (float)a; row[2] = 0.f; row[3] = 0.f;
        for (int j = 0; j <= nf; ++j) {
            const double g = guard(tk[j]);
            row[4 + 2 * j] = down(tk[j] - g);
            row[5 + 2 * j] = up(tk[j] + g);
        }
    }
    return out;
}

}  // namespace

namespace yawhip_detail {  // what the other units call (declared in yawhip_internal.h)

CallKey::CallKey(const yawhip_ctx *ctx, const CountArgs &a, bool want_counts_, bool want_sums_, bool for_work_, int32_t n_dev_)
    : c1_uid(a.c1->uid), c2_uid(a.c2->uid), opt_gen(ctx->opt_gen), n_jobs(a.n_jobs), n_bins(a.n_bins), n_edges(a.n_edges),
      kernel(a.kernel), n_dev(n_dev_), want_counts(want_counts_), want_sums(want_sums_), for_work(for_work_), jobs(a.jobs), t(a.t) {
    // word by word: a job is one 64-bit word, a threshold another
    auto mix = [this](uint64_t w) { hash = (hash ^ w) * 0x100000001b3ull; hash ^= hash >> 29; };
    for (uint64_t w : {c1_uid, c2_uid, opt_gen, (uint64_t)(uint32_t)n_jobs << 32 | (uint32_t)n_bins,
                       (uint64_t)(uint32_t)n_edges << 32 | (uint32_t)kernel,
                       (uint64_t)(uint32_t)n_dev << 32 | (uint64_t)(want_counts | want_sums << 1 | for_work << 2)})
        mix(w);
    for (size_t j = 0; j < (size_t)n_jobs; ++j) {
        uint64_t w;
        memcpy(&w, jobs + 2 * j, sizeof w);
        mix(w);
    }
    for (size_t i = 0; i < (size_t)n_bins * n_edges; ++i) {
        uint64_t w;
        memcpy(&w, t + i, sizeof w);
        mix(w);
    }
}

// What a count call derives from its inputs on the HOST before anything is launched -- kernel choice, layouts, tile and stage
// sizes, the job records / prefix / threshold tables of the item builder and the count kernel (uploaded once, into the plan's
// own device buffer) -- kept for the next call with the same inputs (CallKey). A repeated call (the next step of a bench, the
// same count of the next measurement, DR after DD with the same job list is ANOTHER plan) then marshals no tables at all; the
// item builder and the count kernels run every call. Plans die with their catalogues and options.
struct HostPlan {
    CallKey key;
    uint64_t stamp = 0;
    // decisions
    bool empty = false;   // nothing to count (no output values)
    bool split = false;   // the job list has to be counted in pieces (SPLIT_JOBS)
    int grid_div = 8;  // band kernels: workgroups = potential items / this
    int R = 0, band_ne = 0, cap = 0, hp_shift = 0, lean_bins = 0, mode = 0, reach = 0, kernel = 0, nf = 0, n_orient = 0;
    bool band = false, band32 = false, band_fine = false, filter = false, lean = false, merged = false, run_unweighted = false,
         run_weighted = false, strip_items = false, swap = false, sweep = false, triple = false, uni = false, uniform_t = false,
         weighted = false;
    int64_t abytes = 0, cand = 0, n_items = 0, n_out = 0, n_pslots = 0, n_sjobs = 0, n_slots = 0, slab = 0, tile = 0;
    double rwin_max = 0.0;
    double cap_c = 1.0, cap_s = 0.0;  // cos / sin of sep_angle(rwin_max): the strip builder's trimmed windows (cap_s = 0: untrimmed)
    size_t lds_band = 0, lds_merged = 0;
    // device tables, in one allocation (d_in) made when the plan's table image is uploaded (Planner::tables): jobs / job records,
    // prefix, thresholds, pre-filter thresholds, window widths, float32 classes, layout table, and -- weighted calls -- the chunk
    // prefix of the slab reduction
    DevPtr<unsigned char> d_in;
    int32_t *d_jobs = nullptr;
    int64_t *d_prefix = nullptr, *d_cprefix = nullptr;
    double *d_t = nullptr, *d_rwin = nullptr;
    float *d_dthr = nullptr, *d_ucap = nullptr, *d_thr32 = nullptr;
    DevTab *d_tabs = nullptr;
    int64_t n_chunks = 0;
};

// Forget the plans that involve catalogue `c` (nullptr: all of them).
void drop_plans(yawhip_ctx *ctx, const yawhip_catalog *c) {
    for (size_t i = 0; i < ctx->plans.size();) {
        if (!c || ctx->plans[i]->key.c1_uid == c->uid || ctx->plans[i]->key.c2_uid == c->uid) {
            delete ctx->plans[i];
            ctx->plans[i] = ctx->plans.back();
            ctx->plans.pop_back();
        } else ++i;
    }
}

// The argument checks of a count call, made by every entry point before any device work: handles, sizes, bin counts of the
// catalogues, thresholds and the patch ids of the jobs.
int check_call(const yawhip_ctx *ctx, const CountArgs &a) {
    const yawhip_catalog *c1 = a.c1, *c2 = a.c2;
    if (!ctx || !c1 || !c2) return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs: NULL handle");
    if (a.n_jobs < 0 || a.n_bins <= 0 || a.n_edges < 2 || a.n_edges > MAX_EDGES || !a.t || (a.n_jobs > 0 && !a.jobs))
        return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs: bad sizes (n_jobs=%d n_bins=%d n_edges=%d, max edges %d)",
                    a.n_jobs, a.n_bins, a.n_edges, MAX_EDGES);
    if (c1->ctx != ctx || c2->ctx != ctx) return fail(YAWHIP_ERR_MISMATCH, "catalogues belong to another context");
    if (c1->n_patches != c2->n_patches)
        return fail(YAWHIP_ERR_MISMATCH, "patch counts differ (%d vs %d)", c1->n_patches, c2->n_patches);
    if ((c1->nb != 1 && c1->nb != a.n_bins) || (c2->nb != 1 && c2->nb != a.n_bins))
        return fail(YAWHIP_ERR_MISMATCH, "catalogue bin counts (%d, %d) do not fit n_bins=%d", c1->nb, c2->nb, a.n_bins);
    for (int k = 0; k < a.n_bins; ++k)
        for (int e = 0; e < a.n_edges; ++e) {
            const double v = a.t[(size_t)k * a.n_edges + e];
            if (!(v >= 0.0) || (e > 0 && !(v >= a.t[(size_t)k * a.n_edges + e - 1])))
                return fail(YAWHIP_ERR_INVALID, "thresholds of bin %d are not ascending non-negative numbers", k);
        }
    for (int j = 0; j < a.n_jobs; ++j)
        if (a.jobs[2 * j] < 0 || a.jobs[2 * j] >= c1->n_patches || a.jobs[2 * j + 1] < 0 || a.jobs[2 * j + 1] >= c1->n_patches)
            return fail(YAWHIP_ERR_INVALID, "job %d has a patch id outside [0,%d)", j, c1->n_patches);
    return YAWHIP_OK;
}

// The band_cap option (yawhip_ctx_set_option): 0, or a stage capacity the band kernels are compiled for.
int check_band_cap(int64_t value) {
    if (value != 0 && value != BCAP && value != BCAP_MID && value != B32_CAP && value != B32_CAP_BIG)
        return fail(YAWHIP_ERR_INVALID, "band_cap must be 0 (auto), 192 or 288 (float64 / fine-grid band kernels), %d or %d (float32 band kernel)",
                    B32_CAP, B32_CAP_BIG);
    return YAWHIP_OK;
}

}  // namespace yawhip_detail

namespace {

// make_plan in steps, run in this order: each one fills its own fields of the plan; what a later step needs and the plan does
// not keep stays in the planner.
struct Planner : CountArgs {  // (the call's arguments, under their own names)
    yawhip_ctx *ctx;
    bool for_work;
    HostPlan &P;
    bool unit = false, auto_pick = false, half_ok = false;
    int tile_idx = 0;  // tile table of the layouts (R = 1, 2, 4)
    double layout_sep = 0.0;
    std::vector<double> rwin;     // window half width per bin
    std::vector<int32_t> orient;  // sort axis of the strip layouts of every job
    const StripLayout *L1[3] = {nullptr, nullptr, nullptr}, *L2[3] = {nullptr, nullptr, nullptr};
    const yawhip_catalog *c_lane = nullptr, *c_strm = nullptr;
    const StripLayout *const *LL = nullptr, *const *LS = nullptr;  // lane side, streamed side
    std::vector<float> fine32;
    std::vector<int64_t> prefix;
    std::vector<JobRec> job_recs;  // strip path, per job: what the builder needs of the two groups (JobRec)
    void sides(bool swap) {
        c_lane = swap ? c1 : c2; c_strm = swap ? c2 : c1;
        LL = swap ? L1 : L2; LS = swap ? L2 : L1;
    }
    int kernel_and_sizes(bool want_counts, bool want_sums);
    int layouts();
    int tile_and_stage();
    int histogram();
    int items();
    int tables();
};

// Step 1: the kernel, and the sizes of the output.
int Planner::kernel_and_sizes(bool want_counts, bool want_sums) {
    int32_t kernel = CountArgs::kernel;
    if (kernel == YAWHIP_KERNEL_AUTO) kernel = ctx->default_kernel;
    auto_pick = kernel == YAWHIP_KERNEL_AUTO;  // BAND or SWEEP, whichever suits the layouts (decided below)
    if (kernel == YAWHIP_KERNEL_AUTO) kernel = YAWHIP_KERNEL_BAND;
    if (kernel < YAWHIP_KERNEL_EXACT || kernel > YAWHIP_KERNEL_BAND)
        return fail(YAWHIP_ERR_INVALID, "unknown kernel id %d", kernel);
    // the FP32 pre-filter assumes unit vectors; anything else is evaluated pair by pair in FP64
    unit = c1->unit_norm && c2->unit_norm;
    if (kernel == YAWHIP_KERNEL_FILTER && !unit) kernel = YAWHIP_KERNEL_EXACT;
    // the window search compares the sorted coordinate of both sides: the axes must agree
    if ((kernel == YAWHIP_KERNEL_SWEEP || kernel == YAWHIP_KERNEL_BAND) && c1->axis != c2->axis)
        kernel = unit ? YAWHIP_KERNEL_FILTER : YAWHIP_KERNEL_EXACT;
    // the band kernels park finished lanes on a sentinel at coordinate 4.0 and bound their searches by it: unit vectors only
    if (kernel == YAWHIP_KERNEL_BAND && !unit) kernel = YAWHIP_KERNEL_EXACT;
    P.kernel = kernel;
    P.band = kernel == YAWHIP_KERNEL_BAND;
    P.sweep = kernel == YAWHIP_KERNEL_SWEEP || P.band;
    P.filter = unit && kernel != YAWHIP_KERNEL_EXACT;

    P.nf = n_edges - 1;
    P.n_slots = (int64_t)n_jobs * n_bins;
    P.n_out = P.n_slots * P.nf;
    P.weighted = (c1->w != nullptr) || (c2->w != nullptr);
    P.run_weighted = P.weighted && want_sums;
    P.run_unweighted = want_counts || (!P.weighted && want_sums);
    if (P.n_out == 0) { P.empty = true; return YAWHIP_OK; }
    if (P.n_slots > (1ll << 30)) return fail(YAWHIP_ERR_INVALID, "too many (job,bin) slots");
    HIP_TRY(hipSetDevice(ctx->device));

    // tile size: objects per lane. Larger tiles amortise the streamed-object read; small segments
    // prefer small tiles so that padded lanes do not dominate.
    // Lean path (k_count_merged): z-window culling + FP32 pre-filter + queued exact evaluation. Its merged
    // form (one item for all bins, strip layouts on both sides) serves c1 binned x c2 unbinned, i.e. every
    // count of a cross-correlation.
    P.lean = P.sweep && (P.filter || P.band);  // single-wave workgroups on windowed items (k_count_merged / k_count_band)
    return YAWHIP_OK;
}

// Step 2: layout mode, orientations and strip layouts, the float32 band kernels, the sides, BAND or SWEEP.
int Planner::layouts() {
    const int nf = P.nf;
    rwin.resize((size_t)n_bins);
    double rwin_max = 0.0;  // widest window half width over the bins
    for (int k = 0; k < n_bins; ++k) {
        rwin[(size_t)k] = std::sqrt(t[(size_t)k * n_edges + n_edges - 1]) * (1.0 + 1e-12) + 1e-15;
        rwin_max = std::max(rwin_max, rwin[(size_t)k]);
    }
    P.rwin_max = rwin_max;
    // strip pairing pays while a run has few partner runs; for separations far beyond the grid spacing the
    // ordinary (patch, bin) layout is used instead
    // (grid_sep: the largest separation in the grid's own unit -- chord for a grid linear in v, angle for one in latitude)
    const double grid_sep = c1->strip_grid ? sep_angle(rwin_max) : rwin_max;
    const bool strips = P.lean && c1->has_strips && c2->has_strips && c1->strip_width == c2->strip_width &&
                        c1->strip_grid == c2->strip_grid &&
                        (c1->strip_width <= 0.0 || grid_sep / c1->strip_width <= (double)MAX_STRIP_REACH);
    // mode 3: binned x binned on the per-segment strip layouts: ordinary (job, bin) items whose lane tiles and windows
    // come from (patch, bin, strip) runs -- it pays when the lane side is dense: runs of at least a few lane tiles per
    // (patch, bin, strip); estimated from the patch-level layout the upload built (B times as many runs)
    bool seg_ok = false;
    if (strips && c1->nb == n_bins && c2->nb == n_bins && n_bins > 1 && ctx->seg_strips) {
        const StripLayout &base2 = c2->strips[c2->axis];
        const int64_t seg_runs = base2.h_vbase[(size_t)base2.n_groups] * (int64_t)c2->nb;
        seg_ok = c2->n / std::max<int64_t>(seg_runs, 1) >= ctx->seg_min_run;
    }
    bool uniform_t = true;  // every bin has the same threshold row (angular scales)
    for (int k = 1; k < n_bins && uniform_t; ++k)
        uniform_t = memcmp(t, t + (size_t)k * n_edges, sizeof(double) * n_edges) == 0;
    P.uniform_t = uniform_t;
    // One item for all bins needs a histogram of B x (E - 1) cells (and B edge rows when they differ) in LDS. Where that
    // does not fit (hundreds of bins times dozens of separation-weight bins), the count falls back to ordinary
    // (job, bin) items, whose histogram has E - 1 cells.
    const size_t merged_need = (size_t)n_bins * nf * (P.weighted ? 8 : 4) + (size_t)(uniform_t ? 1 : n_bins) * n_edges * sizeof(double) +
                              (size_t)n_bins * sizeof(float) + band_lds_fixed(BCAP_MID) + (BCAP_MID + 2) * 8 + merged_stage_lds() + 1024;
    const bool merged_fits = merged_need <= (size_t)ctx->lds_limit;
    const int mode = P.mode = !strips ? 0 : (c1->nb > 1 && c2->nb == 1) ? (merged_fits ? 1 : 0) : (seg_ok ? 3 : 0);
    // per-segment strip layouts keep the grid linear in v (build_strip_layout): their short runs make items of fixed cost, and
    // the latitude grid's narrower strips away from v = 0 only add items there
    layout_sep = mode == 3 ? rwin_max : grid_sep;
    const bool merged = P.merged = mode == 1;                // one item covers all bins, output slot = job
    const bool strip_items = P.strip_items = mode != 0;      // items come from strip runs (k_build_items_strips)
    // Orientation of every job: the (u, v) projection that compresses the sphere least around its two patches, i.e.
    // the one that drops the coordinate w in which the patches lie farthest from the origin. (Projected along an
    // axis the patches are nearly perpendicular to, objects pile up in (u, v) -- density grows like 1 / |w| -- and
    // the opposite hemisphere folds onto the same cells: every u-window then holds several times the partners.)
    orient.assign((size_t)n_jobs, (int32_t)c1->axis);
    if (strip_items) {
        bool need[3] = {false, false, false};
        for (int j = 0; j < n_jobs; ++j) {
            if (ctx->auto_orient) {
                const double *b1 = &c1->h_box[(size_t)6 * jobs[2 * j]], *b2 = &c2->h_box[(size_t)6 * jobs[2 * j + 1]];
                double best = -1.0;
                int wax = (c1->axis + 1) % 3;
                for (int a = 0; a < 3; ++a) {
                    const double m = (b1[a] <= b1[3 + a] ? 0.5 * (b1[a] + b1[3 + a]) : 0.0) +
                                     (b2[a] <= b2[3 + a] ? 0.5 * (b2[a] + b2[3 + a]) : 0.0);
                    if (std::fabs(m) > best) { best = std::fabs(m); wax = a; }
                }
                orient[(size_t)j] = (wax + 2) % 3;  // sort axis u whose dropped axis (u + 1) % 3 is wax
            }
            need[orient[(size_t)j]] = true;
        }
        for (int o = 0; o < 3; ++o) {
            if (!need[o]) continue;
            int rc = build_strip_layout(ctx, const_cast<yawhip_catalog *>(c1), o, mode == 3);
            if (rc == YAWHIP_OK && c2 != c1) rc = build_strip_layout(ctx, const_cast<yawhip_catalog *>(c2), o, mode == 3);
            if (rc != YAWHIP_OK) return rc;
            L1[o] = mode == 3 ? &c1->seg[o] : &c1->strips[o];
            L2[o] = mode == 3 ? &c2->seg[o] : &c2->strips[o];
        }
    }
    // Float32 classification (k_count_band32) on strip layouts of unit vectors with up to four edges per bin. Where one
    // side is binned (merged items) the roles are swapped against k_count_band: lane tiles come from the binned catalogue
    // c1, the windows from the unbinned c2 (see the kernel).
    const bool want32 = P.band && strip_items && unit && n_edges <= 4 && ctx->band_fp32 != 0 &&
                        band32_lds(P.weighted, BCAP_MID, (merged ? n_bins : 1) * nf, merged && !uniform_t ? n_bins : 0, n_edges) <=
                            (size_t)ctx->lds_limit;
    // ... and the fine radial grids of separation weights (k_count_band32_fine), when their edges follow the log-spaced model
    if (P.band && strip_items && unit && n_edges > 4 && ctx->band_fp32 != 0 &&
        band32_fine_lds(P.weighted, BCAP_MID, (merged ? n_bins : 1) * nf, uniform_t ? 1 : n_bins, n_edges) <= (size_t)ctx->lds_limit)
        fine32 = build_fine32(t, n_bins, n_edges);
    const bool want_fine = !fine32.empty();
    // (Binned x binned counts of two different catalogues keep c2 on the lanes whichever is sparser: with the 10M data on the
    // lanes and the 100M randoms streamed, DR of config #4 has 570 k items instead of 1.28 M but walks 2.3 x the entries --
    // neighbouring lane objects of a sparse run lie far apart, their common band is long -- 4.1 against 2.2 ms.)
    P.swap = (want32 || want_fine) && merged;
    sides(P.swap);
    if (auto_pick && P.band && unit) {
        // The band kernel decides every entry of a per-object band: unbeatable while a band is a handful of entries of which
        // half are pairs (strip layouts). Without strips a band is the whole u-window of a segment, nearly all of it far away
        // along v -- the FP32 pre-filter of the sweep kernel is made for that. Sparse streamed runs (a few dozen objects: an
        // item is all fixed cost) went to the sweep kernel while the band kernel evaluated in float64; the float32 band kernel
        // has the smaller fixed cost (measured: DD of config #4 0.61 against 0.83 ms, 1M x 1M / 64 patches 0.047 against 0.102,
        // 3M x 0.3M 0.09 against 0.28; sweep stays ahead only where the two sides differ tenfold in density and the items are
        // tiny: DR of config #4 2.09 against 2.23 ms, 0.3M x 3M 0.092 against 0.119) -- so only the float64 band kernel
        // (band_fp32 = 0, more than four edges off the log grid) keeps the density rule.
        bool use_sweep = mode == 0;
        if (!use_sweep && !want32 && !want_fine) {
            double obj_run = 0.0;  // of the densest built orientation
            for (int o = 0; o < 3; ++o)
                if (LS[o]) obj_run = std::max(obj_run, LS[o]->obj_run);
            use_sweep = obj_run < (double)BAND_MIN_STREAM_RUN;
        }
        if (use_sweep) {
            P.kernel = YAWHIP_KERNEL_SWEEP;
            P.band = false;
        }
    }
    P.band32 = want32 && P.band;
    P.band_fine = want_fine && P.band;
    if (!P.band32 && !P.band_fine && P.swap) {  // the sweep kernel streams c1 past lane tiles of c2
        P.swap = false;
        sides(false);
    }
    P.uni = merged || P.band_fine ? uniform_t : true;  // UNI of the band kernels (per-bin items of the others: one threshold row)
    return YAWHIP_OK;
}

// Step 3: objects per lane, the expected window, merged triple runs, the stage capacity.
int Planner::tile_and_stage() {
    const bool band = P.band, strip_items = P.strip_items;
    const int mode = P.mode;
    int R = ctx->tile_r;
    double est_window = 0.0;  // band kernel: expected entries of one window
    if (R == 0) {
        int64_t max_seg = 0;
        if (strip_items) {  // lanes hold runs of a strip layout: their typical (mean) length decides
            int64_t n_runs = 1;
            for (int o = 0; o < 3; ++o)
                if (LL[o]) n_runs = std::max(n_runs, LL[o]->h_vbase[(size_t)LL[o]->n_groups]);
            max_seg = c_lane->n / std::max<int64_t>(n_runs, 1);
            if (mode == 3) max_seg = std::max<int64_t>(max_seg, 4 * MWG * 2);  // at least two objects per lane: per-bin runs are
                                                                                // sparse, the per-item cost outweighs the wider window
        } else {
            for (int j = 0; j < n_jobs; ++j)
                for (int k = 0; k < (c2->nb == 1 ? 1 : n_bins); ++k) max_seg = std::max(max_seg, seg_len(c2, jobs[2 * j + 1], k));
        }
        const int wg = P.lean ? MWG : WG;
        R = max_seg >= 8 * wg * 4 ? 4 : (max_seg >= 4 * wg * 2 ? 2 : 1);
        if (strip_items && R > 2) R = 2;  // on strip runs two objects per lane beat four at every size measured (10M: 2.25 / 2.5 ms, 50M: 68 / 72 ms)
        if (band && strip_items) {
            // band kernel: two neighbouring objects per lane at every density measured once a stage holds the whole
            // window (four per lane: 0.66 / 0.59 ms at the headline, 33 / 24 ms at 50M x 50M, 7.0 / 5.7 ms for RR of
            // config #4). Expected window = the tile's own extent in streamed entries + one band of
            // 2 r_win x (streamed objects of a run per unit of u).
            R = 2;
            auto per_u = [](const auto *c, const StripLayout *const *Ls) {
                int64_t runs = 1;
                for (int o = 0; o < 3; ++o)
                    if (Ls[o]) runs = std::max(runs, Ls[o]->h_vbase[(size_t)Ls[o]->n_groups]);
                double extent = 0.0;
                int n_ext = 0;
                for (int p = 0; p < c->n_patches; ++p) {
                    const double *b = &c->h_box[(size_t)6 * p];
                    double widest = 0.0;
                    for (int a = 0; a < 3; ++a) widest = std::max(widest, b[3 + a] - b[a]);
                    if (widest > 0.0) { extent += widest; ++n_ext; }
                }
                extent = n_ext ? extent / n_ext : 1.0;
                return ((double)c->n / (double)runs) / std::max(extent, 1e-6);
            };
            const double d1 = per_u(c_strm, LS), d2 = per_u(c_lane, LL);
            // binned x binned counts on per-(patch, bin) strip runs: runs are short (35 objects at 10 M, 350 at 100 M objects in
            // 30 bins), bands a handful of entries -- ONE object per lane then evaluates its own band instead of the union of
            // two (DD of config #4: 2.7e7 instead of 5.6e7 entries, 0.63 -> 0.41 ms; RR 3.74 -> 3.57), unless the streamed side
            // is much the sparser one and items are all fixed cost (DR: 2.05e6 items instead of 1.28e6, 1.86 -> 2.25 ms)
            if (mode == 3 && d1 >= 0.5 * d2) R = 1;
            est_window = 64.0 * R * d1 / std::max(d2, 1e-12) + 2.0 * P.rwin_max * d1;
        }
    }
    if (band && R == 0) R = 2;
    // Merged triple runs on the streamed side: one window per item instead of three (k_merge_triples), when the partner
    // strips are exactly c - 1, c, c + 1 (grid at least as wide as the largest separation) AND the merged window still goes
    // through the stage in one piece: cut in pieces it costs more than three whole windows (100M x 100M: 22.0 against 14.9 ms,
    // 50M x 50M with three scales 25.8 against 17.9). The fine-grid kernel has less room (a larger stage costs it residency:
    // 51 fine bins 1.25 against 1.06 ms in a 512-entry stage), so it merges only windows that fit the stage it uses anyway
    // (sparse streamed sides: DR of config #4 2.07 against 2.43). Weighted counts merge like unweighted ones since the kernel
    // with one chunk per round exists: the count kernel takes the same 0.48 ms at the headline in the big stage, the builder
    // searches one window per item instead of three (0.045 against 0.063 ms).
    bool triple = false;
    if ((P.band32 || P.band_fine) && strip_items && ctx->triple_runs && c_strm->n < (1ll << 31) && c1->strip_width > 0.0 &&
        (int)std::floor(layout_sep / c1->strip_width + 1e-6) + 1 == 1) {
        const double est3 = 3.0 * est_window;
        triple = ctx->triple_runs == 2 ||
                 (P.band32 ? est3 <= 0.88 * (B32_CAP_BIG - 4) : est3 <= 0.9 * BCAP_MID);
        for (int o = 0; o < 3 && triple; ++o) {
            if (!LS[o]) continue;
            const int rc = build_triples(ctx, const_cast<yawhip_catalog *>(c_strm), o, mode == 3);
            if (rc == YAWHIP_ERR_OOM) triple = false;  // no room for the copies: three windows per item as before
            else if (rc != YAWHIP_OK) return rc;
        }
        if (triple) est_window = est3;
    }
    P.triple = triple;
    if (g_trace.on) fprintf(stderr, "[yawhip trace] est_window %.1f (triple %d) R %d mode %d\n", est_window, (int)triple, R, mode);
    // stage capacity of the band kernel: the smallest compiled one that holds a whole window (see BCAP_MID)
    int cap = ctx->band_cap == BCAP || ctx->band_cap == BCAP_MID ? ctx->band_cap : 0;
    if (band && cap == 0) cap = R >= 4 || est_window > 0.95 * BCAP ? BCAP_MID : BCAP;
    if (band) {  // (R, stage) pairs that are compiled (the Stage lists of the launch functions, kernel units): the plan names one of them
        if (R == 1) cap = BCAP;
        if (R == 4 && cap == BCAP) cap = BCAP_MID;
    }
    int cap32 = ctx->band_cap == B32_CAP || ctx->band_cap == B32_CAP_BIG ? ctx->band_cap
                                                                         : (est_window > 0.75 * (B32_CAP - 4) ? B32_CAP_BIG : B32_CAP);
    // (0.75: window lengths scatter around the estimate, and a window cut in two costs more than a larger stage -- 50M x 50M
    // with windows of ~265 entries: 21.0 ms in the 320-entry stage, 18.3 ms in a 448-entry one)
    if (R == 1) cap32 = B32_CAP;  // (compiled pairs, as above)
    if (R >= 4) cap32 = B32_CAP_BIG;
    if (P.band32) cap = cap32;  // (the fine-grid kernel still stages window by window, with the capacities of k_count_band)
    P.R = R;
    tile_idx = R == 1 ? 0 : (R == 2 ? 1 : 2);
    P.cap = cap;
    P.tile = (int64_t)(P.lean ? MWG : WG) * R;
    P.lean_bins = P.merged ? n_bins : 1;
    P.lds_merged = merged_lds(P.weighted, P.lean_bins, n_edges);
    return YAWHIP_OK;
}

// Step 4: copies of the band kernel's LDS histogram, its compile-time edge count, its LDS.
int Planner::histogram() {
    const int lean_bins = P.lean_bins, nf = P.nf;
    const bool merged = P.merged, uniform_t = P.uniform_t;
    // Copies of the LDS histogram, lanes spread over them by lane id: same-address atomics of one instruction are
    // serialised. Four copies when there are few slots and the bins of neighbouring entries are unrelated (headline:
    // 0.535 ms with four, 0.565 with eight -- the flush grows with the copies). When the histogram has only the fine bins
    // of ONE redshift bin (per-bin items: every hit of the wave lands in 1-3 cells), or when redshift follows position
    // (same_bin: neighbours of the layout's order sharing their bin; clustered survey: 108 -> 62 ms weighted cross count,
    // 31 -> 18 ms autocorrelation count), more copies pay: up to 16 within 2 KB.
    int hp_shift = lean_bins * nf <= 32 ? 2 : 0;
    if (P.band) {
        double coherence = merged ? 0.0 : 1.0;
        if (merged)
            for (int o = 0; o < 3; ++o)
                if (L1[o]) coherence = std::max(coherence, L1[o]->same_bin);
        if (coherence > 0.25) {
            const int cell = P.weighted ? 8 : 4;
            while (hp_shift < (merged ? 3 : 4) && ((size_t)lean_bins * nf * cell << (hp_shift + 1)) <= 2048) ++hp_shift;
        }
    }
    if (ctx->hist_copies_log2 >= 0) hp_shift = ctx->hist_copies_log2;
    P.band_ne = (!merged || uniform_t) && n_edges <= 4 ? n_edges : (nf == 1 ? 2 : 0);  // compile-time edge count of k_count_band
    const bool band_thr = !(P.band_ne >= 2 && (!merged || uniform_t));
    const size_t LDS_FIXED = (size_t)band_lds_fixed(P.cap);
    auto band_lds_for = [&](int shift) {
        return band_lds_dynamic(P.weighted, band_thr, lean_bins, n_edges, 1 << shift, P.cap, merged && !uniform_t ? lean_bins : 1);
    };
    while (P.band && hp_shift > 0 && band_lds_for(hp_shift) + LDS_FIXED > (size_t)ctx->lds_limit) --hp_shift;  // copies are a tunable, not a need
    P.hp_shift = hp_shift;
    P.lds_band = band_lds_for(hp_shift);
    if (P.lean && (P.band ? P.lds_band + LDS_FIXED : P.lds_merged) > (size_t)ctx->lds_limit)
        return fail(YAWHIP_ERR_INVALID, "too many bins x edges for the LDS histogram (%zu bytes)", P.band ? P.lds_band + LDS_FIXED : P.lds_merged);
    return YAWHIP_OK;
}

// Step 5: the item table -- job records, prefix, candidates and bytes, half bands -- and whether the job list has to be split.
int Planner::items() {
    const bool strip_items = P.strip_items;
    const int mode = P.mode;
    // item table: prefix[slot] = first item of the slot; items of a slot are its lane tiles.
    // standard path: slot = (job, bin); merged path: slot = job (one item covers all bins).
    // strip path: slot = job; its potential items = (lane tiles of patch q) x (groups of up to MAX_WIN of the 2*reach+1
    // neighbouring strips), enumerated by the builder kernel from the catalogues' run tables.
    int64_t n_items = 0, cand = 0, abytes = 0;
    const int obj_bytes1 = c1->w ? 32 : 24, obj_bytes2 = c2->w ? 32 : 24;
    // strip paths: the builder's job table. Modes 1/2: the jobs themselves (groups = patches); mode 3: one pseudo job
    // per (job, bin) between the segments (p, k) and (q, k) (groups = segments), numbered like the output slots.
    P.n_sjobs = mode == 3 ? P.n_slots : (int64_t)n_jobs;
    // Half bands: a catalogue counted against ITSELF meets every unordered pair of a diagonal job twice -- a as lane object with b
    // in its window, b as lane object with a in its. On merged triple runs with one object per lane the lane walks only the
    // entries BEHIND its own place in the triple of its strip (one total order of objects in all triples, k_merge_triples): every
    // pair is met once and counts twice (an exact doubling, also of weighted sums). Half the walk of DD / RR of an autocorrelation.
    half_ok = P.band32 && P.triple && P.R == 1 && c1 == c2 && !P.swap && ctx->half_bands != 0 && !for_work;
    if (strip_items) {
        const double width = c1->strip_width;
        // |dv| <= rwin_max (|d latitude| <= sep_angle(rwin_max))  ->  grid indices differ by at most floor(layout_sep / width) + 1
        const int reach = P.reach = width > 0.0 ? (int)std::floor(layout_sep / width + 1e-6) + 1 : 0;
        std::vector<int32_t> sjobs((size_t)2 * P.n_sjobs);
        for (int j = 0; j < n_jobs; ++j)
            for (int k = 0; k < (mode == 3 ? n_bins : 1); ++k) {
                const int64_t sj = mode == 3 ? (int64_t)j * n_bins + k : j;
                sjobs[(size_t)2 * sj] = mode == 3 ? jobs[2 * j] * n_bins + k : jobs[2 * j];
                sjobs[(size_t)2 * sj + 1] = mode == 3 ? jobs[2 * j + 1] * n_bins + k : jobs[2 * j + 1];
            }
        prefix.resize((size_t)P.n_sjobs + 1);
        job_recs.assign((size_t)P.n_sjobs, JobRec{0, 0, 0, 0, 0});
        for (int64_t j = 0; j < P.n_sjobs; ++j) {
            const int p = sjobs[(size_t)2 * j + (P.swap ? 1 : 0)], q = sjobs[(size_t)2 * j + (P.swap ? 0 : 1)];  // streamed, lane side
            const int o = orient[(size_t)(mode == 3 ? j / n_bins : j)];
            const StripLayout &sl1 = *LS[o], &sl2 = *LL[o];
            const std::vector<int64_t> &tiles = sl2.h_tiles[tile_idx];
            JobRec &jr = job_recs[(size_t)j];
            jr.o = o | (half_ok && p == q ? 4 : 0);
            prefix[(size_t)j] = n_items;
            // strips of q whose grid index lies within `reach` of the strips group p occupies
            const int64_t cnt1 = sl1.h_vbase[(size_t)p + 1] - sl1.h_vbase[(size_t)p], lo1 = sl1.h_slo[(size_t)p];
            const int64_t cnt2 = sl2.h_vbase[(size_t)q + 1] - sl2.h_vbase[(size_t)q], lo2 = sl2.h_slo[(size_t)q];
            const int64_t s_lo = std::max<int64_t>(lo1 - reach - lo2, 0), s_hi = std::min<int64_t>(lo1 + cnt1 - 1 + reach - lo2, cnt2 - 1);
            if (cnt1 > 0 && s_hi >= s_lo) {
                const int64_t r0 = sl2.h_vbase[(size_t)q] + s_lo;
                jr.t_lo = tiles[(size_t)r0];
                jr.k_off = lo2 - sl2.h_vbase[(size_t)q] - lo1;  // strip index of lane run r2 on the common grid, relative to group p
                jr.vbase1 = sl1.h_vbase[(size_t)p];
                jr.n_strips1 = (int32_t)cnt1;
                if (P.triple) {  // triple runs of group p: strips [lo1 - 1, lo1 + cnt1], the first one at vbase + 2 p
                    jr.k_off += 1;
                    jr.vbase1 += 2 * (int64_t)p;
                    jr.n_strips1 += 2;
                }
                n_items += (tiles[(size_t)(r0 + s_hi - s_lo + 1)] - tiles[(size_t)r0]) * ((2 * reach + 1 + MAX_WIN - 1) / MAX_WIN);
            }
        }
        prefix[(size_t)P.n_sjobs] = n_items;
    } else {
        prefix.resize((size_t)P.n_slots + 1);
    }
    P.n_pslots = P.merged ? (int64_t)n_jobs : P.n_slots;
    auto patch_total = [](const yawhip_catalog *c, int patch) {  // objects of a patch over all its bins
        return c->h_off[(size_t)(patch + 1) * c->nb] - c->h_off[(size_t)patch * c->nb];
    };
    for (int j = 0; j < n_jobs; ++j) {
        const int p = jobs[2 * j], q = jobs[2 * j + 1];
        if (strip_items && (c1->nb == 1 || c2->nb == 1)) {
            // an unbinned side is one segment used for every bin: sum_k N1(p,k) N2(q,k) factorises
            cand += c1->nb == 1 ? patch_total(c1, p) * patch_total(c2, q) * (c2->nb == 1 ? n_bins : 1)
                                : patch_total(c1, p) * patch_total(c2, q);
        } else {
            for (int k = 0; k < n_bins; ++k) {
                const int64_t n1 = seg_len(c1, p, k), n2 = seg_len(c2, q, k);
                if (!strip_items) prefix[(size_t)j * n_bins + k] = n_items;
                if (n1 > 0 && n2 > 0) {
                    if (!strip_items) n_items += (n2 + P.tile - 1) / P.tile;
                    cand += n1 * n2;
                }
            }
        }
        // algorithmic bytes of a job = every object of the two patches once (Bobj * (N1 + N2))
        abytes += patch_total(c1, p) * obj_bytes1 + patch_total(c2, q) * obj_bytes2;
    }
    if (!strip_items) prefix[(size_t)P.n_pslots] = n_items;
    P.n_items = n_items;
    P.cand = cand;
    P.abytes = abytes;
    P.slab = P.merged ? (int64_t)n_bins * P.nf : P.nf;  // float64 values per item of the weighted slab
    // A weighted call keeps one slab of partial sums per potential item; long job lists of big catalogues would need
    // tens of GB (50M x 50M, three scales: 40 GB). Above the budget -- and when the items no longer fit 31 bits -- the
    // caller cuts the job list in two and counts the halves one after the other (rows of the result are independent).
    P.split = n_jobs > 1 && !for_work &&
              ((P.run_weighted && n_items * P.slab * (int64_t)sizeof(double) > ctx->slab_budget) || n_items >= (1ll << 31));
    return YAWHIP_OK;
}

// Step 6: the per-bin tables and the layout table; all tables packed into one image, uploaded once; the grid divisor.
int Planner::tables() {
    std::vector<float> dthr((size_t)3 * n_bins);  // per bin: pre-filter threshold, certain-band lower / upper bound
    auto round_down = [](double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -4.0f); return f; };
    for (int k = 0; k < n_bins; ++k) {
        const double thi = t[(size_t)k * n_edges + n_edges - 1];
        float thr32 = ctx->debug_no_hits ? 2.0f : round_down(1.0 - 0.5 * thi - FILTER_GUARD);
        dthr[(size_t)3 * k] = thr32;
        dthr[(size_t)3 * k + 1] = 0.f;  // reserved
        dthr[(size_t)3 * k + 2] = 0.f;
    }
    if (P.merged) rwin[0] = P.rwin_max;  // one window for all bins of the merged run
    // band_trim: {cos, sin} of the largest separation angle per row of rwin, float32 for the band kernels ({1, 0}: untrimmed).
    // The caps assume |a|^2 within UNIT_NORM_TOL of 1 (sep_angle).
    const bool trim = ctx->band_trim && c1->unit_norm && c2->unit_norm;
    std::vector<float> ucap((size_t)2 * n_bins);
    for (int k = 0; k < n_bins; ++k) {
        const double th = sep_angle(rwin[(size_t)k]);
        ucap[(size_t)2 * k] = trim ? (float)std::cos(th) : 1.0f;
        ucap[(size_t)2 * k + 1] = trim ? (float)std::sin(th) : 0.0f;
    }
    if (trim) {
        P.cap_c = std::cos(sep_angle(P.rwin_max));
        P.cap_s = std::sin(sep_angle(P.rwin_max));
    }
    // layout table of the call: [o] = c1, [3 + o] = c2 for orientation o (plain layouts: entries 0 and 3)
    DevTab h_tabs[6];
    memset(h_tabs, 0, sizeof h_tabs);
    if (P.strip_items) {
        for (int o = 0; o < 3; ++o) {
            if (!L1[o]) continue;
            const StripLayout &a = *L1[o], &b = *L2[o];
            h_tabs[o] = make_tab(a.x, a.y, a.z, a.w, P.merged ? a.k : nullptr, a.off, a.d_vbase, a.d_slo, a.d_tiles[tile_idx],
                                 a.d_tile_rec[tile_idx], a.d_grid, o, a.q, a.q_stride, nullptr, a.q4);
            h_tabs[3 + o] = make_tab(b.x, b.y, b.z, b.w, nullptr, b.off, b.d_vbase, b.d_slo, b.d_tiles[tile_idx],
                                     b.d_tile_rec[tile_idx], b.d_grid, o, b.q, b.q_stride, nullptr, b.q4);
            if (P.triple) {
                // the streamed side as merged triple runs: images, weights, offsets and grid index of the triples; the float64
                // columns stay the layout's own (reached through idx by the exact re-evaluation)
                const StripLayout &st = P.swap ? b : a;
                DevTab &tb = h_tabs[P.swap ? 3 + o : o];
                tb = make_tab(st.x, st.y, st.z, st.w3, nullptr, st.off3, st.d_vbase, st.d_slo, st.d_tiles[tile_idx],
                              st.d_tile_rec[tile_idx], st.d_grid3, o, st.q3, st.q3_stride, st.idx3);
                if (half_ok) h_tabs[3 + o].pos3 = (gi32p)(const int32_t *)b.pos3;  // (c1 == c2: the lane side's layout is the streamed one)
            }
        }
    } else {
        h_tabs[0] = make_tab(c1->x, c1->y, c1->z, c1->w, nullptr, c1->off, nullptr, nullptr, nullptr, nullptr, nullptr, c1->axis);
        h_tabs[3] = make_tab(c2->x, c2->y, c2->z, c2->w, nullptr, c2->off, nullptr, nullptr, nullptr, nullptr, nullptr, c2->axis);
    }
    // the tables of the call, packed into the pinned staging buffer and sent with one copy
    static_assert(sizeof(JobRec) == 8 * sizeof(int32_t), "JobRec is 32 bytes");
    const std::vector<float> thr32 = P.band32 ? build_thr32(t, n_bins, n_edges) : (P.band_fine ? fine32 : std::vector<float>());
    // weighted calls: the two-level ordered reduction of the slabs needs the first chunk of every output slot
    std::vector<int64_t> cprefix;
    if (P.run_weighted) {
        cprefix.assign((size_t)P.n_pslots + 1, 0);
        for (int64_t sl = 0; sl < P.n_pslots; ++sl)
            cprefix[(size_t)sl + 1] = cprefix[(size_t)sl] + (prefix[(size_t)sl + 1] - prefix[(size_t)sl] + REDUCE_CHUNK - 1) / REDUCE_CHUNK;
    }
    P.n_chunks = cprefix.empty() ? 0 : cprefix.back();
    const void *src[9] = {P.strip_items ? (const void *)job_recs.data() : (const void *)jobs, prefix.data(), t, dthr.data(),
                          rwin.data(), ucap.data(), thr32.data(), h_tabs, cprefix.data()};
    const size_t bytes[9] = {P.strip_items ? sizeof(JobRec) * (size_t)P.n_sjobs : sizeof(int32_t) * 2 * (size_t)n_jobs,
                             sizeof(int64_t) * ((size_t)P.n_pslots + 1), sizeof(double) * n_bins * n_edges, sizeof(float) * 3 * n_bins,
                             sizeof(double) * n_bins, sizeof(float) * 2 * n_bins, sizeof(float) * thr32.size(), sizeof h_tabs,
                             sizeof(int64_t) * cprefix.size()};
    size_t off[9], off_in = 0;
    for (int i = 0; i < 9; ++i) { off[i] = off_in; off_in = align16(off_in + bytes[i]); }
    std::vector<unsigned char> image(off_in, 0);
    for (int i = 0; i < 9; ++i)
        if (bytes[i]) memcpy(image.data() + off[i], src[i], bytes[i]);
    HIP_TRY(P.d_in.alloc(std::max<size_t>(off_in, 16)));
    HIP_TRY(hipMemcpy(P.d_in, image.data(), off_in, hipMemcpyHostToDevice));  // once per plan
    P.d_jobs = reinterpret_cast<int32_t *>(P.d_in + off[0]);
    P.d_prefix = reinterpret_cast<int64_t *>(P.d_in + off[1]);
    P.d_t = reinterpret_cast<double *>(P.d_in + off[2]);
    P.d_dthr = reinterpret_cast<float *>(P.d_in + off[3]);
    P.d_rwin = reinterpret_cast<double *>(P.d_in + off[4]);
    P.d_ucap = reinterpret_cast<float *>(P.d_in + off[5]);
    P.d_thr32 = reinterpret_cast<float *>(P.d_in + off[6]);
    P.d_tabs = reinterpret_cast<DevTab *>(P.d_in + off[7]);
    P.d_cprefix = reinterpret_cast<int64_t *>(P.d_in + off[8]);
    P.n_orient = (L1[0] ? 1 : 0) + (L1[1] ? 1 : 0) + (L1[2] ? 1 : 0);
    // Workgroups of the band kernels = potential items / grid_div (the kernel loops over the rest). Uniform catalogues, whose
    // items are alike, run best with few, longer-lived workgroups: / 8, / 16 for the per-bin items of binned x binned counts, of
    // which the builder keeps a third (headline 4 / 8 / 16 -> 0.277 / 0.275 / 0.292 ms; config #4 DR 1.59 / 1.53 / 1.48, RR 3.08 /
    // 3.04 / 3.02). On CLUSTERED catalogues items differ a hundredfold and the hardware's dispatch of many short workgroups is the
    // load balancer: / 4 (clustered survey, 3M x 4M: cross count 40.1 against 43.3 ms with / 8, autocorrelation count 7.1
    // against 8.2 with / 16). Clustered = the run the typical OBJECT sits in (sum len^2 / sum len) is more than twice the mean run.
    double skew = 1.0;
    for (const StripLayout *const *LX : {L1, L2})
        for (int o = 0; o < 3; ++o)
            if (LX[o] && LX[o]->built) {
                const yawhip_catalog *cx = LX == L1 ? c1 : c2;
                const double runs = (double)std::max<int64_t>(LX[o]->h_vbase[(size_t)LX[o]->n_groups], 1);
                skew = std::max(skew, LX[o]->obj_run / std::max((double)cx->n / runs, 1.0));
            }
    P.grid_div = ctx->band_grid_div > 0 ? ctx->band_grid_div : (skew > 2.0 ? 4 : (P.mode == 3 ? 16 : 8));
    if (g_trace.on) fprintf(stderr, "[yawhip trace] run skew %.2f -> grid / %d\n", skew, P.grid_div);
    return YAWHIP_OK;
}

// The host half of a count call (its arguments passed check_call): every decision, the tables -- into a plan (see HostPlan).
// for_work: the plan of a cost estimate (count_enqueue's job_work).
int make_plan(yawhip_ctx *ctx, const CountArgs &a, bool want_counts, bool want_sums, bool for_work, HostPlan &P) {
    Planner pl{a, ctx, for_work, P};
    int rc = pl.kernel_and_sizes(want_counts, want_sums);
    if (rc == YAWHIP_OK && !P.empty) rc = pl.layouts();
    if (rc == YAWHIP_OK && !P.empty) rc = pl.tile_and_stage();
    if (rc == YAWHIP_OK && !P.empty) rc = pl.histogram();
    if (rc == YAWHIP_OK && !P.empty) rc = pl.items();
    if (rc == YAWHIP_OK && !P.empty && !P.split) rc = pl.tables();
    if (rc == YAWHIP_OK) g_trace.mark("planned");
    return rc;
}

}  // namespace

namespace yawhip_detail {

// First half of yawhip_count_pairs on ONE device: everything up to and including the copy of the results into the
// context's pinned buffer is put on the context's stream; nothing waits for the device (SWEEP's grid sizing aside).
// The host side of it (make_plan) is done once per distinct set of inputs and looked up afterwards.
// job_work != nullptr: cost estimate only -- the item builder runs, evaluated pairs per job are returned, no counting.
int count_enqueue(yawhip_ctx *ctx, const CountArgs &a, bool want_counts, bool want_sums, int64_t *job_work, CallState &cs,
                  bool fetch_results) {
    cs = CallState{};
    cs.wall0 = std::chrono::steady_clock::now();
    g_trace.mark("enqueue");
    cs.want_counts = want_counts;
    cs.want_sums = want_sums;
    HIP_TRY(hipSetDevice(ctx->device));
    CallKey key(ctx, a, want_counts, want_sums, job_work != nullptr);
    HostPlan *plan = nullptr;
    for (HostPlan *cand_plan : ctx->plans)
        if (cand_plan->key == key) {
            plan = cand_plan;
            break;
        }
    if (!plan) {
        std::unique_ptr<HostPlan> fresh(new (std::nothrow) HostPlan());
        if (!fresh) return fail(YAWHIP_ERR_OOM, "host allocation failed");
        const int rc = make_plan(ctx, a, want_counts, want_sums, job_work != nullptr, *fresh);
        if (rc != YAWHIP_OK) return rc;
        key.keep();
        fresh->key = std::move(key);
        if (ctx->plans.size() >= MAX_PLANS) {  // evict the least recently used one (nothing of it is in flight: calls are blocking,
            size_t old = 0;                    // and a batch is never longer than the plans kept)
            for (size_t i = 1; i < ctx->plans.size(); ++i)
                if (ctx->plans[i]->stamp < ctx->plans[old]->stamp) old = i;
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            delete ctx->plans[old];
            ctx->plans[old] = ctx->plans.back();
            ctx->plans.pop_back();
        }
        plan = fresh.release();
        ctx->plans.push_back(plan);
    }
    plan->stamp = ++ctx->plan_clock;
    const HostPlan &P = *plan;
    cs.n_out = P.n_out;
    if (P.empty) return YAWHIP_OK;
    if (P.split) return SPLIT_JOBS;
    if (P.run_weighted) HIP_TRY(reserve_call(ctx->d_partials, (size_t)std::max<int64_t>(P.n_items, 1) * P.slab));
    g_trace.mark("plan");
    // results: [counters][counts][sums] in one device buffer; counters and counts are zero when no call of the slot is in
    // flight (CallBufs::dirty; sums are always fully written), and k_call_tail brings back what was asked for
    const size_t o_ctr = 0, o_counts = align16(N_CTR * sizeof(unsigned long long)),
                 o_sums = o_counts + align16((size_t)P.n_out * sizeof(unsigned long long));
    const size_t out_bytes = o_sums + align16((size_t)P.n_out * sizeof(double));
    const unsigned char *const block_was = ctx->out.d;
    HIP_TRY(ctx->out.reserve(out_bytes));
    if (ctx->out.d != block_was) {  // a new block: nothing is known of it, and no call has signed it off
        ctx->dirty = true;
        reinterpret_cast<unsigned long long *>(ctx->out.h)[CTR_DONE] = 0;
    }
    ctx->d_ctr = reinterpret_cast<unsigned long long *>(ctx->out.d + o_ctr);
    ctx->d_counts = reinterpret_cast<unsigned long long *>(ctx->out.d + o_counts);
    ctx->d_sums = reinterpret_cast<double *>(ctx->out.d + o_sums);
    // (no items: no kernel writes the sums either)
    const size_t zero_needed = P.n_items > 0 ? o_sums : out_bytes;
    if (ctx->dirty) ctx->zero_upto = 0;
    if (ctx->zero_upto < zero_needed) {
        HIP_TRY(hipMemsetAsync(ctx->out.d + ctx->zero_upto, 0, zero_needed - ctx->zero_upto, ctx->stream));
        ctx->zero_upto = zero_needed;
    }
    ctx->dirty = true;  // until count_finish has seen this call's tail complete
    cs.seq = ++ctx->seq;
    cs.stamps = P.n_items > 0;  // a builder runs

    // what the launches need from the plan and from the call's buffers (the buffers reserved below are entered as they come)
    CountLaunch L;
    L.stream = ctx->stream;
    L.R = P.R; L.cap = P.cap; L.band_ne = P.band_ne;
    L.merged = P.merged; L.uni = P.uni; L.nf1 = P.nf == 1; L.filter = P.filter;
    L.one_chunk = P.triple || !P.strip_items;  // every item has one window
    L.n_bins = a.n_bins; L.n_edges = a.n_edges; L.hp_shift = P.hp_shift;
    L.tile = P.tile; L.slab = P.slab; L.n_chunks = P.n_chunks; L.n_oslots = P.n_pslots;
    L.n_build_jobs = P.strip_items ? P.n_sjobs : P.n_pslots;
    L.reach = P.reach; L.swap = P.swap; L.triple = P.triple;
    L.rwin_max = P.rwin_max; L.cap_c = P.cap_c; L.cap_s = P.cap_s;
    L.c1 = view_of(a.c1); L.c2 = view_of(a.c2);
    L.d_tabs = P.d_tabs; L.d_jobs = P.d_jobs; L.d_prefix = P.d_prefix; L.d_cprefix = P.d_cprefix;
    L.d_t = P.d_t; L.d_rwin = P.d_rwin; L.d_dthr = P.d_dthr; L.d_ucap = P.d_ucap; L.d_thr32 = P.d_thr32;
    L.d_ctr = ctx->d_ctr; L.d_counts = ctx->d_counts; L.d_sums = ctx->d_sums; L.d_partials = ctx->d_partials.ptr;

    int launches = 0;
    const int64_t n_pot = L.n_pot = P.n_items;
    int64_t n_items = P.n_items;  // the count grid: all potential items, or what the builder kept (SWEEP)
    unsigned long long seg_cap = 0;  // > 0: the item list is kept in ITEM_SEGS segments of this many records
    g_trace.mark("memset");
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    if (n_pot > 0) {
        if (n_pot >= (1ll << 31))
            return fail(YAWHIP_ERR_INVALID, "too many work items (%lld) in one job", (long long)n_pot);
        const int bwg = build_wg_for(n_pot);
        const unsigned bgrid = (unsigned)((n_pot + bwg - 1) / bwg);
        // item list in segments (append_items): where the float32 band kernels consume what the strip builder keeps
        if (P.strip_items && (P.band32 || P.band_fine) && !job_work && ctx->item_segments)
            seg_cap = (unsigned long long)((bgrid + ITEM_SEGS - 1) / ITEM_SEGS) * (unsigned long long)bwg;
        HIP_TRY(reserve_call(ctx->d_items, seg_cap ? (size_t)(seg_cap * ITEM_SEGS) : (size_t)n_pot));
        if (P.run_weighted && P.sweep) {  // weighted runs of the culling builders: which potential items write a slab
            HIP_TRY(reserve_call(ctx->d_kept, (size_t)n_pot));
            HIP_TRY(hipMemsetAsync(ctx->d_kept.ptr, 0, (size_t)n_pot, ctx->stream));
            L.d_kept = ctx->d_kept.ptr;
        }
        L.build_grid = bgrid; L.build_wg = (unsigned)bwg; L.seg_cap = seg_cap; L.d_items = ctx->d_items.ptr;
        HIP_TRY(P.strip_items ? launch_build_strips(L) : (P.sweep ? launch_build_windows(L) : launch_build_whole(L)));
        ++launches;
        // The count kernels are launched over all potential items and return at once for indices beyond the
        // number the builder kept (device counter): no host round trip between the two kernels.
        n_items = n_pot;
        if (P.strip_items && !P.band && n_pot > SYNC_GRID_MIN_ITEMS) {
            // SWEEP: the strip path keeps about one potential item in five; a grid over all of them spends ~0.2 ms
            // dispatching workgroups that exit at once (measured at 1.6e6 potential items, 10M x 10M), more than
            // this round trip (~0.05 ms) costs. Small calls (one GPU's share of a sharded job list) skip it.
            // (The band kernel sizes its grid from the potential items and loops: no round trip.)
            HIP_TRY(hipMemcpyAsync(ctx->out.h, ctx->d_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            n_items = (int64_t)reinterpret_cast<unsigned long long *>(ctx->out.h)[CTR_KEPT];
        }
    }
    if (job_work) {  // cost estimate only: evaluated pairs per job from the item list, no counting
        HIP_TRY(reserve_call(ctx->d_jobwork, (size_t)a.n_jobs));
        HIP_TRY(hipMemsetAsync(ctx->d_jobwork.ptr, 0, sizeof(unsigned long long) * (size_t)a.n_jobs, ctx->stream));
        if (n_pot > 0) HIP_TRY(launch_item_work(L, P.merged ? 1 : a.n_bins, ctx->d_jobwork.ptr));
        HIP_TRY(hipMemcpyAsync(job_work, ctx->d_jobwork.ptr, sizeof(int64_t) * (size_t)a.n_jobs, hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return YAWHIP_OK;
    }
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->evc0, ctx->stream));
    // The count kernel(s): the family and the variant selectors come from the plan; every launch records the variant it ran in
    // cs.variant[weighted] (yawhip_stats.count_variant*).
    // Band kernels: grid from the number of POTENTIAL items (known on the host); the kernel reads the number the builder kept
    // from the device counter, workgroups beyond it exit, workgroups loop if more were kept than the grid holds.
    // The strip builder keeps about one potential item in five, ordinary items are all kept.
    int64_t grid = P.strip_items && n_pot > 65536 ? n_pot / P.grid_div : n_pot;
    // Batches of consecutive items (one flush of the histogram per batch) are a tunable, off by default: consecutive
    // items are tiles of the same run, so on clustered data a batch strings the heaviest items together on one
    // workgroup (measured: DD of the clustered survey with 31 fine bins 7.2 -> 20.6 ms with batches of four), and on
    // uniform data the flush they save is not what the time goes to (2.27 ms either way at the headline, 51 fine bins).
    const int batch_log2 = ctx->band_batch_log2 >= 0 ? ctx->band_batch_log2 : 0;
    if (!P.run_weighted) grid = std::max<int64_t>(grid >> batch_log2, 8);
    grid = std::min<int64_t>((grid + 7) & ~7ll, 1ll << 22);
    // 32-bit LDS counters: one stage adds at most 64 R x CAP to a cell, so flush at the latest every
    // 2^32 / (64 R CAP) stages (2^17 for two objects per lane and 192-entry stages, 2^15 for four and 288)
    int flush_log2 = ctx->flush_log2;
    while (flush_log2 > 0 && ((uint64_t)64 * P.R * 2 * P.cap << flush_log2) >= (1ull << 32)) --flush_log2;  // (x 2: half bands count double)
    const bool band_ran = n_items > 0 && P.lean && P.band;
    L.band_grid = (unsigned)grid; L.n_items = n_items; L.batch_log2 = batch_log2; L.flush_mask = (1u << flush_log2) - 1u;
    if (band_ran) {
        L.family = P.band32 ? CountFamily::BAND32 : (P.band_fine ? CountFamily::BAND32_FINE : CountFamily::BAND64);
        L.lds = P.band32 ? band32_lds(P.weighted, P.cap, P.lean_bins * P.nf, P.merged && !P.uniform_t ? a.n_bins : 0, a.n_edges)
                         : (P.band_fine ? band32_fine_lds(P.weighted, P.cap, P.lean_bins * P.nf, P.uniform_t ? 1 : a.n_bins, a.n_edges)
                                        : P.lds_band);
    } else {
        L.family = P.lean ? CountFamily::LEAN : CountFamily::PLAIN;
        L.lds = P.lds_merged;  // (k_count: per launch, below)
    }
    for (const bool wgt : {false, true}) {
        if (n_items <= 0 || !(wgt ? P.run_weighted : P.run_unweighted)) continue;
        if (L.family == CountFamily::PLAIN) {  // per-lane private histograms where they fit
            L.priv = count_lds(wgt, true, a.n_edges) <= (size_t)ctx->lds_limit;
            L.lds = count_lds(wgt, L.priv, a.n_edges);
        }
        HIP_TRY(launch_count(L, wgt, &cs.variant[wgt]));
        ++launches;
    }
    if (n_items > 0 && P.run_weighted) {
        // two-level ordered reduction of the weighted slabs (k_reduce_chunks / k_reduce_slots), per output slot
        HIP_TRY(reserve_call(ctx->d_chunk_sums, (size_t)std::max<int64_t>(P.n_chunks, 1) * P.slab));
        L.d_chunk_sums = ctx->d_chunk_sums.ptr;
        if (P.n_chunks > 0) HIP_TRY(launch_reduce_chunks(L));
        HIP_TRY(launch_reduce_slots(L));
        launches += 2;
    }
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->evc1, ctx->stream));
    if (!P.weighted && want_sums) {
        HIP_TRY(launch_counts_to_double(L, P.n_out));
        ++launches;
    }
    if (!cs.stamps) HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    // the tail brings back the counters and whatever was asked for, into pinned memory, and cleans behind itself
    // (fetch_results = false: the caller reduces the results on the device first and fetches what is left; counters only here,
    // and the counts stay where they are: the slot stays dirty)
    const size_t fetch = !fetch_results ? o_counts : (want_sums ? out_bytes : (want_counts ? o_sums : o_counts));
    const size_t clean = std::min(fetch, o_sums);
    const bool sums_written = P.n_items > 0 && (P.run_weighted || want_sums);
    cs.cleaned = clean == o_sums;
    cs.zero_after = sums_written ? o_sums : ctx->zero_upto;
    const unsigned n_copy = (unsigned)(fetch / 16), n_clean = (unsigned)(clean / 16);
    static_assert(N_CTR * sizeof(unsigned long long) % 16 == 0 && (CTR_DONE + 2) * sizeof(unsigned long long) <= N_CTR * sizeof(unsigned long long),
                  "the tail's words lie inside the counter block");
    if (fetch / 16 > 0xffffffffull) return fail(YAWHIP_ERR_INVALID, "result block too large (%zu bytes)", fetch);
    HIP_TRY(launch_call_tail(ctx->stream, ctx->out.d, ctx->out.h, n_copy, n_clean, (unsigned long long)cs.seq));
    ++launches;
    cs.pending = true;
    cs.o_ctr = o_ctr; cs.o_counts = o_counts; cs.o_sums = o_sums;
    cs.band_ran = band_ran; cs.run_unweighted = P.run_unweighted; cs.run_weighted = P.run_weighted;
    cs.cand = P.cand; cs.abytes = P.abytes; cs.n_pot = n_pot; cs.segmented = seg_cap != 0;
    cs.launches = launches; cs.kernel = P.kernel; cs.mode = P.mode;
    cs.n_orient = P.n_orient;
    cs.band_variant = !band_ran ? 0 : (P.band32 ? 32 : (P.band_fine ? 33 : 64));
    cs.merged_triples = band_ran && P.triple ? 1 : 0;
    g_trace.mark("launched");
    return YAWHIP_OK;
}

// Second half: wait for the context's stream, hand the results (contiguous rows of the jobs given to count_enqueue) and
// the statistics over.
// row_index != nullptr: row r of this call's result goes to row row_index[r] of the caller's arrays (rows of row_len values):
// the devices of a multi-device call write their shares straight into place.
// wait_done: wait for the active slot's ev_done (recorded by the caller behind everything this call put on the stream)
// instead of the whole stream -- the requests of a batch behind it keep running.
int count_finish(yawhip_ctx *ctx, const CallState &cs, int64_t *fine_counts, double *fine_sums, yawhip_stats *stats,
                 const int32_t *row_index, int64_t row_len, bool wait_done) {
    if (stats) memset(stats, 0, sizeof *stats);
    const int64_t n_rows = !row_index ? 1 : (row_len > 0 ? cs.n_out / row_len : 0), row = row_index ? row_len : cs.n_out;
    if (!cs.pending) {
        place_rows<int64_t>(fine_counts, nullptr, n_rows, row, row_index);
        place_rows<double>(fine_sums, nullptr, n_rows, row, row_index);
        return YAWHIP_OK;
    }
    g_trace.mark("meanwhile");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->spin_wait) {
        // poll for up to 2 ms (a headline call takes 0.5 ms; the wake-up of a blocked thread costs ~0.01 ms), then block.
        // What is polled is the completion word k_call_tail writes into the slot's pinned block behind the results -- no
        // runtime call per look -- unless the caller put more behind the tail: then the stream or the slot's ev_done, as before.
        const unsigned long long *done_word = reinterpret_cast<const unsigned long long *>(ctx->out.h) + CTR_DONE;
        auto query = [&]() { return wait_done ? hipEventQuery(ctx->ev_done) : hipStreamQuery(ctx->stream); };
        hipError_t qe = hipErrorNotReady;
        const auto spin0 = std::chrono::steady_clock::now();
        do {
            if (cs.word_wait) {
                if (__atomic_load_n(done_word, __ATOMIC_ACQUIRE) == cs.seq) qe = hipSuccess;
            } else {
                qe = query();
            }
            if (qe != hipErrorNotReady) break;
            __builtin_ia32_pause();
        } while (std::chrono::steady_clock::now() - spin0 < std::chrono::milliseconds(2));
        if (qe == hipSuccess && cs.word_wait) {  // one look at the runtime: an asynchronous error surfaces here, not a call later
            const hipError_t late = query();
            if (late != hipErrorNotReady) qe = late;  // (not ready: the packets behind the tail, or other slots' requests)
        }
        if (qe == hipErrorNotReady) qe = wait_done ? hipEventSynchronize(ctx->ev_done) : hipStreamSynchronize(ctx->stream);
        HIP_TRY(qe);
    } else {
        HIP_TRY(wait_done ? hipEventSynchronize(ctx->ev_done) : hipStreamSynchronize(ctx->stream));
    }
    g_trace.mark("waited");
    if (cs.cleaned) {  // the tail has left [counters][counts] of the slot's block at zero
        ctx->dirty = false;
        ctx->zero_upto = cs.zero_after;
    }
    place_rows(fine_counts, reinterpret_cast<const int64_t *>(ctx->out.h + cs.o_counts), n_rows, row, row_index);
    place_rows(fine_sums, reinterpret_cast<const double *>(ctx->out.h + cs.o_sums), n_rows, row, row_index);
    const unsigned long long *ctr = reinterpret_cast<const unsigned long long *>(ctx->out.h + cs.o_ctr);
    g_trace.mark("copied");
    if (stats) {
        float ms = 0.f, cms = 0.f;
        if (cs.stamps) {
            // device clock stamps (see CTR_T_BUILD): the builder's start to the tail's start, and the latest builder exit to the
            // start of the first kernel behind the count kernel(s) -- the count kernels with the dispatch gaps on either side
            unsigned long long built = 0;
            for (int sg = 0; sg < ITEM_SEGS; ++sg) built = std::max(built, ctr[SEG_EXIT_CTR(sg)]);
            ms = (float)((double)(ctr[CTR_T_TAIL] - ctr[CTR_T_BUILD]) * CLOCK_MS);
            cms = (float)((double)(ctr[CTR_T_COUNTED] - built) * CLOCK_MS);
        } else {
            HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            HIP_TRY(hipEventElapsedTime(&cms, ctx->evc0, ctx->evc1));
        }
        stats->count_ms = cms;
        stats->candidate_pairs = cs.cand;
        unsigned long long tile_pairs = 0;
        for (int i = 0; i < EVAL_SLOTS; ++i) tile_pairs += ctr[TILE_PAIR_CTR((size_t)i)];
        stats->evaluated_pairs = (int64_t)tile_pairs * ((cs.run_unweighted ? 1 : 0) + (cs.run_weighted ? 1 : 0));
        if (cs.band_ran) {  // band kernel: the entries its lanes really walked (both launches of a weighted + counts call)
            unsigned long long ev = 0;
            for (int i = 0; i < EVAL_SLOTS; ++i) ev += ctr[BAND_ENTRY_CTR((size_t)i)];
            stats->evaluated_pairs = (int64_t)ev;
        }
        stats->algorithmic_bytes = cs.abytes;
        stats->n_workgroups = cs.n_pot > 0 ? (int64_t)ctr[CTR_KEPT] : 0;
        if (cs.segmented && cs.n_pot > 0)
            for (int sg = 0; sg < ITEM_SEGS; ++sg) stats->n_workgroups += (int64_t)ctr[ITEM_SEG_CTR(sg)];
        stats->n_launches = cs.launches;
        stats->kernel_used = cs.kernel;
        stats->layout_mode = cs.mode;
        stats->n_orientations = cs.n_orient;
        stats->band_variant = cs.band_variant;
        stats->merged_triples = cs.merged_triples;
        stats->count_variant = cs.variant[0];
        stats->count_variant_weighted = cs.variant[1];
        if (cs.band_ran)
            for (int i = 0; i < EVAL_SLOTS; ++i) stats->exact_reevaluations += (int64_t)ctr[EXACT_EVAL_CTR((size_t)i)];
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - cs.wall0).count();
    }
    g_trace.mark("stats");
    return YAWHIP_OK;
}

void add_stats(yawhip_stats &total, const yawhip_stats &part, bool side_by_side) {
    total.candidate_pairs += part.candidate_pairs;
    total.evaluated_pairs += part.evaluated_pairs;
    total.algorithmic_bytes += part.algorithmic_bytes;
    total.n_workgroups += part.n_workgroups;
    total.n_launches += part.n_launches;
    total.kernel_used = part.kernel_used;
    total.layout_mode = part.layout_mode;
    total.n_orientations = std::max(total.n_orientations, part.n_orientations);
    total.band_variant = part.band_variant;
    total.merged_triples = part.merged_triples;
    total.count_variant = merge_variant(total.count_variant, part.count_variant);
    total.count_variant_weighted = merge_variant(total.count_variant_weighted, part.count_variant_weighted);
    total.exact_reevaluations += part.exact_reevaluations;
    if (side_by_side) {  // devices of one call run at the same time: the slowest counts
        total.kernel_ms = std::max(total.kernel_ms, part.kernel_ms);
        total.count_ms = std::max(total.count_ms, part.count_ms);
    } else {             // pieces of one job list on one device run one after the other
        total.kernel_ms += part.kernel_ms;
        total.count_ms += part.count_ms;
    }
}

// One job list on one device, cut in halves as often as count_enqueue asks for (SPLIT_JOBS).
int run_single(yawhip_ctx *ctx, const CountArgs &a, int64_t *fine_counts, double *fine_sums, yawhip_stats *stats,
               const std::function<void()> *meanwhile) {
    // meanwhile: host work of the caller that does not need the result, done while the device counts (once)
    CallState cs;
    int rc = count_enqueue(ctx, a, fine_counts != nullptr, fine_sums != nullptr, nullptr, cs);
    if (meanwhile && (rc == YAWHIP_OK || rc == SPLIT_JOBS)) (*meanwhile)();
    if (rc == YAWHIP_OK) return count_finish(ctx, cs, fine_counts, fine_sums, stats);
    if (rc != SPLIT_JOBS) return rc;
    const int32_t half = a.n_jobs / 2;
    const size_t row = (size_t)a.n_bins * (size_t)(a.n_edges - 1);
    yawhip_stats sa{}, sb{};
    rc = run_single(ctx, a.with_jobs(half, a.jobs), fine_counts, fine_sums, &sa);
    if (rc != YAWHIP_OK) return rc;
    rc = run_single(ctx, a.with_jobs(a.n_jobs - half, a.jobs + 2 * (size_t)half),
                    fine_counts ? fine_counts + (size_t)half * row : nullptr, fine_sums ? fine_sums + (size_t)half * row : nullptr, &sb);
    if (rc != YAWHIP_OK) return rc;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        add_stats(*stats, sa, false);
        add_stats(*stats, sb, false);
        stats->total_ms = sa.total_ms + sb.total_ms;
    }
    return YAWHIP_OK;
}

}  // namespace yawhip_detail

extern "C" {

int yawhip_count_pairs(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                       const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                       int64_t *fine_counts, double *fine_sums, yawhip_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const CountArgs args{c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel};
    const int rc_args = check_call(ctx, args);
    if (rc_args != YAWHIP_OK) return rc_args;
    if (ctx->peers.empty() || n_jobs < 2) return run_single(ctx, args, fine_counts, fine_sums, stats);
    // ---- several devices: the independent jobs are split over them (replaces the reference's process pool,
    // src/yaw/utils/parallel.py:251-346). Every device holds both catalogues; a job's rows of the result come from
    // exactly one device, so nothing has to be reduced: the rows are copied into place.
    const size_t n_dev = ctx->peers.size() + 1;
    if (c1->replicas.size() != n_dev - 1 || c2->replicas.size() != n_dev - 1)
        return fail(YAWHIP_ERR_MISMATCH, "catalogue was not uploaded to every device of the context");
    const auto wall0 = std::chrono::steady_clock::now();
    // the plan: evaluated pairs per job from the item builder (device 0), longest-processing-time-first over the devices;
    // it depends on the inputs only and is kept for the next call with the same inputs
    // (the inputs of the cost estimate below, and the device count)
    CallKey key(ctx, args, false, false, true, (int32_t)n_dev);
    if (!(ctx->plan.key == key)) {
        std::vector<int64_t> work((size_t)n_jobs, 0);
        CallState cs;
        int rc = count_enqueue(ctx, args, false, false, work.data(), cs);
        if (rc != YAWHIP_OK) return rc;
        std::vector<int32_t> order((size_t)n_jobs);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return work[(size_t)a] > work[(size_t)b]; });
        std::vector<double> load(n_dev, 0.0);
        ctx->plan.parts.assign(n_dev, {});
        const double fixed = 2.0e5;  // evaluated-pair equivalent of touching a job at all
        for (int32_t j : order) {
            const size_t d = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
            ctx->plan.parts[d].push_back(j);
            load[d] += (double)work[(size_t)j] + fixed;
        }
        for (auto &part : ctx->plan.parts) std::sort(part.begin(), part.end());
        key.keep();
        ctx->plan.key = std::move(key);
    }
    const int64_t row = (int64_t)n_bins * (n_edges - 1);
    std::vector<CallState> states(n_dev);
    std::vector<std::vector<int32_t>> sub(n_dev);
    std::vector<char> later(n_dev, 0);  // shares that have to be cut in pieces: counted after the others, one by one
    std::vector<CountArgs> share(n_dev, args);  // a device's share: its jobs, on its replicas of the catalogues
    for (size_t d = 0; d < n_dev; ++d) {  // enqueue everywhere first: the devices work side by side
        for (int32_t j : ctx->plan.parts[d]) { sub[d].push_back(jobs[2 * j]); sub[d].push_back(jobs[2 * j + 1]); }
        yawhip_ctx *dc = d == 0 ? ctx : ctx->peers[d - 1];
        share[d] = args.with_jobs((int32_t)ctx->plan.parts[d].size(), sub[d].data());
        if (d > 0) { share[d].c1 = c1->replicas[d - 1]; share[d].c2 = c2->replicas[d - 1]; }
        const int rc = count_enqueue(dc, share[d], fine_counts != nullptr, fine_sums != nullptr, nullptr, states[d]);
        if (rc == SPLIT_JOBS) {
            later[d] = 1;
        } else if (rc != YAWHIP_OK) {
            for (size_t e = 0; e < d; ++e) (void)hipStreamSynchronize((e == 0 ? ctx : ctx->peers[e - 1])->stream);
            return rc;
        }
    }
    std::vector<int64_t> rows_c;
    std::vector<double> rows_s;
    yawhip_stats total{}, part{};
    int rc_all = YAWHIP_OK;
    for (size_t d = 0; d < n_dev; ++d) {  // every device's copy into its pinned buffer is already under way: drain in turn
        yawhip_ctx *dc = d == 0 ? ctx : ctx->peers[d - 1];
        const size_t nj = ctx->plan.parts[d].size();
        int rc;
        if (later[d]) {  // a share that is counted in pieces: through a temporary, then into place
            if (fine_counts) rows_c.resize(nj * (size_t)row);
            if (fine_sums) rows_s.resize(nj * (size_t)row);
            rc = run_single(dc, share[d], fine_counts ? rows_c.data() : nullptr, fine_sums ? rows_s.data() : nullptr, &part);
            if (rc == YAWHIP_OK) {
                place_rows(fine_counts, (const int64_t *)rows_c.data(), (int64_t)nj, row, ctx->plan.parts[d].data());
                place_rows(fine_sums, (const double *)rows_s.data(), (int64_t)nj, row, ctx->plan.parts[d].data());
            }
        } else {         // rows go from the device's pinned buffer straight into the caller's arrays
            rc = count_finish(dc, states[d], fine_counts, fine_sums, &part, ctx->plan.parts[d].data(), row);
        }
        if (rc != YAWHIP_OK) { rc_all = rc; continue; }  // keep draining the other devices
        add_stats(total, part, true);
    }
    (void)hipSetDevice(ctx->device);  // leave the thread on the context's first device, as single-device calls do
    if (rc_all != YAWHIP_OK) return rc_all;
    total.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (stats) *stats = total;
    return YAWHIP_OK;
}

int yawhip_job_work(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs, const int32_t *jobs,
                    int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel, int64_t *work) {
    if (!ctx || !work) return fail(YAWHIP_ERR_INVALID, "yawhip_job_work: NULL argument");
    for (int j = 0; j < n_jobs; ++j) work[j] = 0;
    const CountArgs args{c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel};
    const int rc = check_call(ctx, args);
    if (rc != YAWHIP_OK) return rc;
    CallState cs;
    return count_enqueue(ctx, args, false, false, work, cs);
}

}  // extern "C"
