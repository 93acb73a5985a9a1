/*
 * yawhip.h -- C ABI of libyawhip.so: MI355X (gfx950) angular pair counting for yet_another_wizz.
 *
 * The reference (jlvdb/yet_another_wizz, pure Python) has no FFI of its own; the seam this library
 * replaces is the per-job loop of
 *     PatchLinkage.count_pairs                       src/yaw/correlation/measurements.py:344-364
 * i.e. for every linked patch pair and every redshift bin one call of
 *     process_patch_pair -> AngularTree.count        measurements.py:88-128, src/yaw/catalog/trees.py:303-362
 *     -> scipy KDTree.count_neighbors                trees.py:348-353
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md (a ctypes stub).
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer is caller-owned host memory unless stated otherwise,
 *     contiguous, 8-byte aligned; the library owns all device memory behind opaque handles;
 *   - one context = one GPU (yawhip_ctx_create) or several GPUs of the node (yawhip_ctx_create_multi) = one
 *     process; calls are blocking and must not be issued concurrently on the same context;
 *   - a context remembers what a count call derives from its inputs on the host (kernel choice, job / threshold tables on the
 *     device) for the next call with the same catalogue pair, job list, thresholds and options: inputs are compared by
 *     content, the item builder and the count kernels run every call;
 *   - every function returns 0 on success or a negative yawhip_status; nothing throws;
 *     yawhip_last_error() returns a thread-local, human readable message for the last failure.
 */
#ifndef YAWHIP_H
#define YAWHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YAWHIP_ABI_VERSION 6

typedef enum yawhip_status {
    YAWHIP_OK = 0,
    YAWHIP_ERR_INVALID = -1,   /* bad argument (NULL handle, negative size, unsorted thresholds ...) */
    YAWHIP_ERR_NO_DEVICE = -2, /* no usable HIP device / device id out of range */
    YAWHIP_ERR_HIP = -3,       /* a HIP runtime call failed (message has the HIP error string) */
    YAWHIP_ERR_OOM = -4,       /* device or host allocation failed */
    YAWHIP_ERR_MISMATCH = -5   /* catalogs do not fit together (patch count, bin count, context) */
} yawhip_status;

/* Which device code path counts the pairs. All of them return identical results. */
typedef enum yawhip_kernel {
    YAWHIP_KERNEL_AUTO = 0,   /* library picks the fastest exact path: BAND on every strip layout of unit vectors (its float32
                                 kernels; the float64 band kernel -- band_fp32 = 0, more than four edges off a log grid --
                                 only where the streamed runs are dense), SWEEP on layouts without strips, EXACT for
                                 input that is not unit vectors (stats->kernel_used / band_variant tell) */
    YAWHIP_KERNEL_EXACT = 1,  /* plain FP64 brute force over every candidate pair */
    YAWHIP_KERNEL_FILTER = 2, /* FP32 guard-banded pre-filter, FP64 re-evaluation of survivors */
    YAWHIP_KERNEL_SWEEP = 3,  /* FILTER + sorted-axis sweep that skips far-away tile pairs */
    YAWHIP_KERNEL_BAND = 4    /* sorted-axis windows as SWEEP, then every lane object walks only its own band |du| <= r of the
                                 window: classified in float32 against guard bands around the edges, the evaluations inside a
                                 guard band decided by the exact FP64 predicate (band_fp32 = 1, default; results identical),
                                 or every entry in FP64 (band_fp32 = 0) (ABI >= 3) */
} yawhip_kernel;

typedef struct yawhip_ctx yawhip_ctx;
typedef struct yawhip_catalog yawhip_catalog;

/* Filled by yawhip_count_pairs (may be NULL). Times are milliseconds. */
typedef struct yawhip_stats {
    int64_t candidate_pairs;   /* sum over (job, bin) of N1(p,k) * N2(q,k): the brute-force work unit   */
    int64_t evaluated_pairs;   /* pair distances the launched kernels actually evaluated (<= candidates
                                  when tile culling is active, padded lanes not included)               */
    int64_t algorithmic_bytes; /* compulsory HBM bytes: per job, every object of both patches once       */
    int64_t n_workgroups;      /* workgroups of the dominant (count) kernel                              */
    int32_t n_launches;        /* kernel launches in this call                                           */
    int32_t kernel_used;       /* yawhip_kernel actually run                                             */
    double kernel_ms;          /* device time from the first to the last kernel of the call (item builder, count
                                  kernel, reduction): start of the builder to start of the call's tail kernel, from
                                  stamps of the device's constant 100 MHz clock (HIP events when no builder ran) */
    double total_ms;           /* host wall time of the whole call (job upload, kernels, result download)*/
    double count_ms;           /* device time of the count kernel(s) alone (ABI >= 2): from the last builder workgroup's
                                  exit to the start of the next kernel behind them, from the same clock stamps --
                                  so it includes the two dispatch gaps next to the count kernel(s)            */
    int32_t layout_mode;       /* which device layouts the items came from (ABI >= 3): 0 = (patch, bin, u) segments,
                                  1 = (patch, strip) runs with all bins merged (binned x unbinned), 3 = (patch, bin,
                                  strip) runs (binned x binned, dense catalogues)                       */
    int32_t n_orientations;    /* strip layouts: how many of the three orientations the jobs used (ABI >= 3) */
    int64_t exact_reevaluations; /* band kernel, float32 classification: evaluations that fell into a guard band of an edge
                                  and were decided by the exact float64 predicate (ABI >= 4)                  */
    int32_t band_variant;      /* which band kernel ran (ABI >= 4): 0 none, 64 every entry in float64, 32 float32 classes +
                                  exact guard bands, 33 the same for fine log-spaced radial grids             */
    int32_t merged_triples;       /* 1: the float32 band kernel streamed merged triple runs (one window per item), else 0 */
    int32_t count_variant;        /* compiled count kernel of the call's unweighted launch, weighted launch (ABI >= 6): 0 none,
                                     YAWHIP_VARIANT_MIXED where pieces of the call (slab budget, devices) launched different
                                     variants, else the code below                                                    */
    int32_t count_variant_weighted;
} yawhip_stats;

/* Count-kernel variant codes (yawhip_stats.count_variant*): the kernel family and every template argument it was launched with.
 *   bits 0-3   family: 1 k_count<R, WEIGHTED, PRIV, FILTER>, 2 k_count_merged<R, WEIGHTED, NF1, MERGED>, 3 k_count_merged_occ8 (same),
 *              4 k_count_band<R, CAP, WEIGHTED, NE, MERGED, UNI>, 5 k_count_band32 (same), 6 k_count_band32_one (same),
 *              7 k_count_band32_fine<R, CAP, WEIGHTED, MERGED, UNI>
 *   bits 4-6   R            bits 8-17  CAP (LDS stage entries)      bit 18  WEIGHTED     bits 19-21  NE (edges)
 *   bit 22     MERGED       bit 23     UNI      bit 24  PRIV        bit 25  FILTER       bit 26      NF1 */
#define YAWHIP_VARIANT_MIXED (-1)

const char *yawhip_last_error(void);
int yawhip_abi_version(void);

/* Number of visible HIP devices. */
int yawhip_device_count(int *n);

/* Create / destroy a context on device `device_id` (creates one HIP stream). */
int yawhip_ctx_create(int device_id, yawhip_ctx **out);
int yawhip_ctx_destroy(yawhip_ctx *ctx);
/* One context over several GPUs of the node (ABI >= 3; replaces the worker pool behind `max_workers` of
 * PatchLinkage.count_pairs, src/yaw/correlation/measurements.py:344-350, src/yaw/utils/parallel.py:251-346):
 * catalogues uploaded to it are replicated on every device, yawhip_count_pairs splits its job list over the devices
 * (longest job first, by the work the item builder reports) and returns the complete result; options apply to all
 * devices. A device id may be listed more than once (several streams on one GPU; used by the tests). Everything
 * else behaves as for a single-device context; yawhip_assign_patches and yawhip_job_work use the first device. */
int yawhip_ctx_create_multi(const int *device_ids, int n_devices, yawhip_ctx **out);
/* Number of devices a context spans. */
int yawhip_ctx_device_count(const yawhip_ctx *ctx, int *n);

/* Tunables (all optional):
 *   "tile_r"            objects per lane (0 = auto, 1, 2, 4)
 *   "band_batch_log2"   band kernel: log2 of the consecutive items a workgroup takes per visit, carrying its unweighted
 *                       histogram while they add to the same output slot (-1 = default: 1 item; larger batches unbalance clustered data)
 *   "hist_copies_log2"  band kernel: log2 of the copies of its LDS histogram (-1 = auto: 4 copies for few slots, up to 16
 *                       for per-bin items or when neighbouring objects of a binned catalogue mostly share their bin; 0..6)
 *   "band_cap"          entries per LDS stage of the band kernel (0 = auto; 192 / 288: float64 and fine-grid kernels;
 *                       320 / 512: float32 kernel -- the larger one when a lane tile's window is expected to need it)
 *   "kernel"            default yawhip_kernel of yawhip_count_pairs(kernel = AUTO)
 *   "strip_width_micro" spacing, in 1e-6 rad of latitude (1e-6 chord units with strip_grid = 0), of the strip grid of
 *                       catalogues uploaded afterwards (0 = no strips, default 5000). Catalogues counted against each other
 *                       should share it; otherwise the cross-correlation path falls back to ordinary (job, bin) items.
 *   "strip_grid"        strip grid of catalogues uploaded afterwards: 1 (default) uniform in the latitude of the object's
 *                       direction about the strip axis, 0 linear in that coordinate (same results; catalogues counted
 *                       against each other must share it for the strip path)
 *   "band_trim"         1 (default): the strip item builder and the float32 band kernels cut every u-window and band to the
 *                       u-range the lane objects' largest separation angle can reach on the sphere; 0: +/- sqrt(t_max)
 *                       around the keys (same results)
 *   "seg_strips"        binned x binned counts use the per-(patch, bin) strip layouts of dense catalogues (default 1)
 *   "seg_strips_min_run" mean objects per (patch, bin, strip) run of the lane-side catalogue from which they are used (default 16)
 *   "debug_no_hits"     diagnostics: the pre-filter rejects everything (times the filter alone; wrong counts)
 *   "auto_orient"       1 (default): every job runs on the strip layouts of the orientation (sort axis u, strips along v,
 *                       dropped axis w) that suits its two patches -- w pointing at them; layouts of further
 *                       orientations are built on first use. 0: the sort axis the catalogues were uploaded with
 *   "slab_budget_bytes" weighted calls keep a slab of partial sums per potential work item; a job list that would need more
 *                       than this many bytes (default 2^30) is counted in pieces, one after the other (same results)
 *   "band_fp32"         1 (default): on strip layouts of unit vectors the band kernel classifies every evaluation in float32
 *                       and decides the ones inside a guard band of an edge with the exact float64 predicate (same results);
 *                       0: every evaluation in float64
 *   "triple_runs"       float32 band kernels: the streamed side is read from MERGED runs of three neighbouring strips (one
 *                       window per work item instead of three) when the strip grid is as wide as the largest separation --
 *                       1 (default): where the merged window still fits one LDS stage, 2: always, 0: never (same results)
 *   "half_bands"        1 (default): a catalogue counted against ITSELF on merged triple runs with one object per lane takes every
 *                       unordered pair of a diagonal job once and counts it twice (half the walk of DD / RR of an
 *                       autocorrelation; an exact doubling, also of weighted sums); 0: both sides walk their full bands
 *   "item_segments"     1 (default): the strip builder keeps its work items in eight segments, one per XCD, each with its
 *                       own append counter; 0: one list, dealt to the XCDs in blocks (same results)
 *   "band_grid_div"     band kernels: workgroups = potential work items / this (1..64; default 0 = auto: 8, 16 for the per-bin
 *                       items of binned x binned counts, 4 on clustered catalogues); the kernel loops over the rest
 *   "spin_wait"         1 (default): the host waits for a call's results by polling the stream for the first 2 ms, then blocks;
 *                       0: it blocks at once
 *   "flush_stages_log2" band kernel: the 32-bit LDS counters of an item are flushed to the 64-bit result every
 *                       2^value stages (default 17: 128 lane objects x 192 entries x 2^17 < 2^32; tests lower it)
 *   "hist_chunk_log2"   yawhip_redshift_histogram uploads its columns in chunks of 2^value objects (8..30, default 23);
 *                       peak device memory does not grow with n (same results) */
int yawhip_ctx_set_option(yawhip_ctx *ctx, const char *key, int64_t value);

/*
 * Upload one catalogue (replaces: Catalog.build_trees + the per-job pickle.load of trees.pkl,
 * catalog.py:1406-1461, trees.py:365-429,597).
 *   n            objects kept (objects outside the redshift binning are already dropped, trees.py:414)
 *   x,y,z        unit vectors, float64[n], exactly the host's AngularCoordinates.to_3d() values
 *   w            float64[n] weights or NULL (unweighted)
 *   n_patches    P
 *   n_bins_or_1  B for a catalogue binned in redshift, 1 for an unbinned one (single tree re-used
 *                for every bin, trees.py:600-601)
 *   offsets      int64[P * n_bins_or_1 + 1], CSR over (patch, bin) segments; objects are sorted by
 *                (patch, bin); offsets[0] == 0, offsets[last] == n, non-decreasing
 * Order of objects inside a segment is free (it only permutes floating point summation order).
 */
int yawhip_catalog_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                          const double *w, int32_t n_patches, int32_t n_bins_or_1, const int64_t *offsets,
                          yawhip_catalog **out);
/* Same, choosing the coordinate (0 = x, 1 = y, 2 = z) along which the library keeps each segment sorted
 * for its window culling; yawhip_catalog_upload uses z. Pick the axis most perpendicular to the survey
 * footprint (a footprint around a pole is flat in z and culls badly along it). Two catalogues counted
 * against each other should use the same axis, otherwise the culling is skipped (results unchanged). */
int yawhip_catalog_upload_axis(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                               const double *w, int32_t n_patches, int32_t n_bins_or_1, const int64_t *offsets,
                               int32_t sort_axis, yawhip_catalog **out);
/*
 * One catalogue with a scalar field ("kappa") as the TWO catalogues a scalar count runs on (ABI 6, additive; replaces the
 * per-count weight product of AngularTree.get_pair_weights, trees.py:270-301): the coordinates are copied to the device once
 * and every (patch, bin) segment is sorted once, then one gather writes
 *   cat_n   the catalogue yawhip_catalog_upload_axis(x, y, z, w) makes (unweighted when w is NULL): the "n" side
 *   cat_k   the same objects in the same order with the weight column kappa * w (kappa when w is NULL): the "k" side
 *   kappa   float64[n], any sign
 * The product is one float64 multiply on the device, rounded on its own: cat_k is, bit for bit, the catalogue
 * yawhip_catalog_upload_axis makes from a host column kappa * w. Both are ordinary catalogues -- each has its own identity
 * for the plans, builds its strip layouts as any other, is replicated on every device of a multi-device context and is
 * released by its own yawhip_catalog_free. On failure neither is returned: both are NULL, whichever check failed.
 */
int yawhip_catalog_upload_scalar(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                                 const double *w, const double *kappa, int32_t n_patches, int32_t n_bins_or_1,
                                 const int64_t *offsets, int32_t sort_axis, yawhip_catalog **cat_n, yawhip_catalog **cat_k);
/*
 * Sum of the weight column over every (patch, bin) segment of a resident catalogue (ABI 6, additive; AngularTree.sum_weights
 * and .sum_kappa, trees.py:225-244, for all trees at once: cat_n gives sum w, cat_k sum kappa * w).
 *   sums   float64[P * n_bins_or_1] (host), segment order of the offsets; an unweighted catalogue reports its object counts
 * Summed on the device in a fixed order per segment (256 strided partial sums, folded in halves): the same catalogue gives the
 * same bits every time; numpy's pairwise sum of the same values agrees to rounding. No atomics.
 */
int yawhip_catalog_segment_sums(const yawhip_catalog *cat, double *sums);
int yawhip_catalog_sort_axis(const yawhip_catalog *cat, int32_t *axis);
int yawhip_catalog_free(yawhip_catalog *cat);
/* Device bytes held by a catalogue (for memory accounting). */
/* (The library also exports a symbol yawhip_debug_lane_image. It is a hook of the test suite, deliberately not declared
 * here and not part of this ABI: it builds a strip layout as a side effect and may change or go without notice.) */
int yawhip_catalog_device_bytes(const yawhip_catalog *cat, int64_t *bytes);

/*
 * Count pairs for a list of jobs (replaces measurements.py:344-364 up to, not including, the
 * scatter into [S,B,P,P] and the rweight / scale recombination of trees.py:358-362: this entry point
 * returns the per-job fine values; yawhip_count_pairs_dense below does the epilogue as well -- the
 * recombination of several fine bins on the device, the scatter on the host).
 *   c1, c2     catalogues on the same context with equal n_patches; c1 == c2 is allowed (DD / RR
 *              of an autocorrelation): every ordered pair a != b is then counted, self pairs have
 *              s == 0 and never fall above an edge, exactly as in the reference
 *   jobs       int32[n_jobs][2] = (patch id in c1, patch id in c2)
 *   n_bins     B; a catalogue uploaded with n_bins_or_1 == 1 uses its single segment for every bin,
 *              otherwise its n_bins_or_1 must equal n_bins
 *   n_edges    E >= 2 thresholds per bin
 *   t          float64[B][E], ascending in E: t[k][e] = pow(2 sin(ang_bins[k][e] / 2), 2.0) computed
 *              on the host (trees.py:107-117, coordinates.py:277)
 *   kernel     yawhip_kernel
 * Pair (a in c1 segment (p,k), b in c2 segment (q,k)) belongs to fine bin e (0 <= e < E-1) iff
 *       t[k][e] < s <= t[k][e+1],   s = ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2   in float64 without FMA.
 * Outputs (either may be NULL; on success every element is written, the caller need not clear them):
 *   fine_counts  int64[n_jobs][B][E-1]  number of pairs            (bit exact)
 *   fine_sums    float64[n_jobs][B][E-1] sum of w_a * w_b, a missing weight column counts as 1.0.
 *                No floating point atomics touch global memory: per-item partial sums are combined in a fixed
 *                order. BAND and SWEEP add into a histogram that one wave owns (LDS float64 adds in program
 *                order; adds of ONE instruction that hit the same cell are assumed to be serialised by the LDS in a
 *                fixed lane order, as observed on MI355X): bit-reproducible from run to run for a given build and tile_r. EXACT / FILTER keep
 *                per-lane private histograms, reduced in a fixed order, while (E-1) * 2 KiB fits LDS (E-1 <= 78);
 *                beyond that they share one LDS histogram between four waves, whose float64 adds are ordered
 *                by the hardware: sums then agree only to rounding (1e-10 relative is what the tests ask)
 * When both catalogues are unweighted fine_sums, if requested, is the exact conversion of fine_counts.
 */
int yawhip_count_pairs(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                       const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                       int64_t *fine_counts, double *fine_sums, yawhip_stats *stats);

/*
 * The same count, returned as the result tensor of PatchLinkage.count_pairs (ABI >= 4; replaces measurements.py:344-364
 * INCLUDING the host epilogue: the separation weights and per-scale recombination of trees.py:358-362,134-160, the x 0.5
 * of the diagonal jobs of an autocorrelation, measurements.py:362-363, and the scatter of every job into its slot):
 *   n_scales        S
 *   slices          int32[B][S][2]: scale s of bin k sums the fine bins [first, last) of that bin (the indices of the edges
 *                   nearest to the scale's limits, trees.py:134-160)
 *   fine_factors    float64[B][E-1] multiplied into the fine bins before they are summed (separation weights,
 *                   trees.py:358-360), or NULL
 *   halve_diagonal  non-zero: jobs with equal patch ids count x 0.5 (autocorrelation)
 *   dense           float64[S][B][P][P], P = the catalogues' patch count; slot [s][k][i][j] of job (i, j), 0 elsewhere
 * The weighted-sum reproducibility note of yawhip_count_pairs applies; it further assumes that the LDS serialises float64
 * adds of ONE instruction to the same address in a fixed lane order (observed on MI355X; tested run to run).
 */
int yawhip_count_pairs_dense(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                             const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                             int32_t n_scales, const int32_t *slices, const double *fine_factors, int32_t halve_diagonal,
                             double *dense, yawhip_stats *stats);

/*
 * Several counts of ONE measurement from one call (ABI >= 5): the reference's crosscorrelate issues DD, DR, RD, RR back to
 * back on one linkage (src/yaw/correlation/measurements.py:617-628), autocorrelate DD, DR, RR (:517-523) -- same binning,
 * thresholds and recombination, other catalogue pairs and job lists. All requests are put on the context's stream at once
 * (up to four in flight, each with its own work items and result block): the host prepares count k + 1 and writes the
 * tensor of count k while the device counts. Results are those of n_requests calls of yawhip_count_pairs_dense, bit for bit.
 *   requests   n_requests records; `dense` and `stats` of every record are written (stats may be NULL)
 * A context of several devices counts the requests one after the other (each split over the devices).
 */
typedef struct yawhip_dense_request {
    const yawhip_catalog *c1, *c2; /* catalogue pair of this count (c1 == c2: DD / RR of an autocorrelation)      */
    int32_t n_jobs;                /* linked patch pairs of this count                                            */
    int32_t halve_diagonal;        /* non-zero: jobs with equal patch ids count x 0.5 (autocorrelation)           */
    const int32_t *jobs;           /* int32[n_jobs][2]                                                            */
    double *dense;                 /* out: float64[S][B][P][P]                                                    */
    yawhip_stats *stats;           /* out, may be NULL                                                            */
} yawhip_dense_request;
int yawhip_count_pairs_dense_batch(yawhip_ctx *ctx, int32_t n_requests, const yawhip_dense_request *requests, int32_t n_bins,
                                   int32_t n_edges, const double *t, int32_t kernel, int32_t n_scales, const int32_t *slices,
                                   const double *fine_factors);

/*
 * The count of ONE rank of a job list sharded over processes (one process per GPU; ABI >= 4), left on the device for the
 * final reduce (replaces the result messages of the reference's task farm, src/yaw/utils/parallel.py:251-346):
 *   jobs, n_jobs    this rank's share
 *   n_rows_total    jobs of the whole list
 *   row_index       int32[n_jobs]: position of each of this rank's jobs in the whole list
 *   device_rows     out: DEVICE pointer to float64[n_rows_total * B * (E-1) + 1], owned by the context and valid until its
 *                   next call: this rank's rows in place (weighted sums, or the exact conversion of the counts), zero
 *                   elsewhere -- every row is non-zero on one rank only, so a sum all-reduce (RCCL) over the ranks yields the
 *                   complete tensor, exactly. The last element is zero: callers use it as a status flag in the reduce.
 * The context's stream has been waited for when the call returns. Single-device contexts only.
 */
int yawhip_count_pairs_rows_device(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                                   const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                                   int64_t n_rows_total, const int32_t *row_index, double **device_rows, yawhip_stats *stats);

/*
 * Nearest patch centre of n objects in Euclidean xyz (replaces scipy.cluster.vq.vq in assign_patch_centers,
 * catalog/catalog.py:229-249, same arithmetic: identical ids including ties, first minimum wins).
 *   x,y,z        float64[n] unit vectors (host)
 *   centers_xyz  float64[n_centers][3] (host, row-major)
 *   patch_out    int32[n] (host)
 */
int yawhip_assign_patches(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z,
                          int32_t n_centers, const double *centers_xyz, int32_t *patch_out);

/*
 * Uniform random points in an ra / dec box with optional attached values -- BoxRandoms.__call__ of the reference
 * (src/yaw/randoms.py:152-178, 256-259) called for n values in chunks of chunksize, as Catalog.from_random does
 * (catalog/readers.py:137-192) -- drawn on the device from numpy's PCG64 stream: every value and the end state are
 * numpy's, bit for bit. Per chunk of k values: k x ~ U(x_min, x_min + x_range), k y the same way, then, with attached
 * data, k indices Generator.integers(0, n_data) and the values at them.
 *   state        numpy's bit_generator.state before the first chunk: state hi, state lo, inc hi, inc lo (64-bit halves)
 *   has_uint32, uinteger   its pending 32-bit half (read before any other half by the first index draw)
 *   n_data       -1: nothing attached (no index draws); else 1 .. 2^32 (more: YAWHIP_ERR_INVALID, numpy's 64-bit path)
 *   data_w, data_z         float64[n_data] values to draw from (host, may be NULL), w_out / z_out float64[n] given with them
 *   x_out, y_out float64[n] (host): x = ra in radian, y = sin(dec)
 *   idx_out      int64[n] drawn indices (host, may be NULL)
 *   state_out, has_uint32_out, uinteger_out   numpy's state after the last chunk (inc does not change)
 */
int yawhip_random_box(yawhip_ctx *ctx, int64_t n, int64_t chunksize, const uint64_t state[4], int32_t has_uint32,
                      uint32_t uinteger, double x_min, double x_range, double y_min, double y_range, int64_t n_data,
                      const double *data_w, const double *data_z, double *x_out, double *y_out, double *w_out,
                      double *z_out, int64_t *idx_out, uint64_t state_out[2], int32_t *has_uint32_out,
                      uint32_t *uinteger_out);

/*
 * Random points inside a HEALPix mask or probability map with optional attached values -- HealPixRandoms.__call__ called
 * for n values in chunks of chunksize, on the stream that generator defines (the reference picks its mask pixels from
 * numpy's global RNG, so there is no reference stream): every value and the end state are the host route's, bit for bit.
 * Per chunk of k values: k 64-bit outputs give u = (out >> 11) * 2^-53 and the pixel ipix_unmasked[j], j = number of
 * cdf values <= u (numpy's searchsorted(cdf, u, "right")); k more give sub = out >> (64 - 2 (29 - order)) and the nested
 * order-29 pixel ipix * 4^(29 - order) + sub, whose centre is the point; then the indices as for yawhip_random_box.
 * Arguments as for yawhip_random_box, with the map instead of the box:
 *   order          of the map, 0 .. 13
 *   n_unmasked     1 .. 12 * 4^order
 *   ipix_unmasked  int64[n_unmasked] nested pixel numbers at `order` (host)
 *   cdf            float64[n_unmasked] cumulative probabilities, non-decreasing, cdf[n_unmasked - 1] == 1 (host)
 *   x_out, y_out   float64[n] (host): x = ra = phi in radian, y = sin(dec) = z of the pixel centre
 *   pix_out        int64[n] drawn order-29 pixels (host, may be NULL)
 * The pixel list and the cdf are copied to the device once per call.
 */
int yawhip_random_healpix(yawhip_ctx *ctx, int64_t n, int64_t chunksize, const uint64_t state[4], int32_t has_uint32,
                          uint32_t uinteger, int32_t order, int64_t n_unmasked, const int64_t *ipix_unmasked,
                          const double *cdf, int64_t n_data, const double *data_w, const double *data_z, double *x_out,
                          double *y_out, double *w_out, double *z_out, int64_t *idx_out, int64_t *pix_out,
                          uint64_t state_out[2], int32_t *has_uint32_out, uint32_t *uinteger_out);

/*
 * Per-patch redshift histogram (HistData.from_catalog / _redshift_histogram, src/yaw/redshifts.py:44-57, 101-151).
 *   z, w          float64[n] host columns, grouped by patch (the catalogue's own order); w may be NULL
 *   offsets       int64[n_patches + 1], offsets[0] == 0, offsets[n_patches] == n, non-decreasing (empty patches allowed)
 *   edges         float64[n_edges], strictly increasing, n_edges >= 2
 *   closed_right  1: "right", 0: "left"
 *   out           float64[n_patches][n_edges - 1] (host): object count (w == NULL) or sum of weights per patch and bin
 * The reference's rule: first its mask (z > edges[0] when closed right, z < edges[B] when closed left), then numpy's
 * histogram rule: bin i if edges[i] <= z < edges[i + 1], the last bin also takes z == edges[B]; values outside
 * [edges[0], edges[B]] and NaN are dropped. Bins are decided by float64 comparisons against the given edges. Counts are
 * exact; weighted sums are float64 per tile of at most 4096 objects of one patch, tiles summed in object order (ABI >= 6).
 */
int yawhip_redshift_histogram(yawhip_ctx *ctx, int64_t n, const double *z, const double *w, int32_t n_patches,
                              const int64_t *offsets, int32_t n_edges, const double *edges, int32_t closed_right,
                              double *out);

/*
 * HEALPix pixels of n points and their map (healpix.ang2pix / healpix.healpix_map, Catalog.healpix_map; what the reference
 * leaves to healpy's ang2pix and np.bincount). The pixel is HEALPix' loc2pix in the float64 steps healpix.py documents,
 * one IEEE operation each: every pixel is the host route's, bit for bit. A ring-scheme number is the nested pixel put
 * through the ring arithmetic of yawhip_random_healpix' pixel centres (ABI >= 6).
 *   chunksize   objects per pass (0: 2^24; values above 2^28 are cut to 2^28); the results do not depend on it
 *   phi, z      float64[n] host columns: ra in radian (any finite value) and sin(dec)
 *   w           float64[n] weights (host), may be NULL; read only for map_out
 *   order       of the map, 0 .. 13 (nside = 2^order)
 *   nested      1: NESTED numbers, 0: RING numbers
 *   pix_out     int64[n] pixel of every point (host, may be NULL); -1 for a point with a non-finite phi or z or |z| > 1
 *   map_out     float64[12 * 4^order] (host, may be NULL): objects per pixel (w == NULL; 64-bit integer counters on the
 *               device, exact) or the sum of weights per pixel; points with pixel -1 are left out
 * pix_out and map_out may not both be NULL. The weighted map equals numpy's sequential np.bincount(pix, w) bit for bit
 * and is the same from run to run: per pass a stable radix sort by pixel, then one thread per pixel adds its weights to
 * the map's value in object order (no floating-point atomics). That thread is alone with its pixel, so a weighted map of
 * few pixels and many objects is slow (order 0: twelve threads).
 */
int yawhip_healpix_map(yawhip_ctx *ctx, int64_t n, int64_t chunksize, const double *phi, const double *z,
                       const double *w, int32_t order, int32_t nested, int64_t *pix_out, double *map_out);

/*
 * The unmasked pixels of a full-sky HEALPix scalar map as the columns of a catalogue (healpix.map_pixels,
 * Catalog.from_healpix_map): what a user of the reference does with healpy's pix2ang and a mask. A pixel is selected when
 * its value is finite and not healpy's UNSEEN (-1.6375e30) and, with a weight map, its weight is finite and > 0. The
 * outputs list the selected pixels in ascending NESTED number, whatever the scheme of the maps (ABI >= 6).
 *   n_pix       12 * 4^order
 *   chunksize   nested pixels per pass (0: 2^24; values above 2^28 are cut to 2^28); the results do not depend on it
 *   values      float64[n_pix] the map (host)
 *   weights     float64[n_pix] weight / coverage map in the same scheme (host), may be NULL
 *   order       of the maps, 0 .. 13 (nside = 2^order)
 *   nested      1: the maps are in NESTED order, 0: in RING order
 *   capacity    entries of every output: the number of selected pixels, counted by the caller with the same rule
 *   ipix_out    int64[capacity] pixel number in the maps' own scheme: values[ipix] is kappa (host)
 *   phi_out, z_out   float64[capacity] pixel centre: ra in radian and sin(dec), the float64 steps of randoms.pix2loc_nest,
 *               one IEEE operation each, bit for bit the host route's
 *   kappa_out   float64[capacity] the value
 *   w_out       float64[capacity] the weight; not written (may be NULL) without weights
 *   n_selected  pixels selected and written (out)
 * Outputs may be NULL when capacity is 0. Nothing is written at or beyond `capacity`: a pass that would go beyond it ends
 * the call with YAWHIP_ERR_MISMATCH before it is copied, and so does a total other than `capacity`. Per pass a count kernel
 * (wave ballot, one count per workgroup), an exclusive scan and a write kernel that places every selected pixel by its
 * rank: order preserving, without atomics or floating-point sums; all pixel and element indices are 64-bit.
 */
int yawhip_healpix_pixels(yawhip_ctx *ctx, int64_t n_pix, int64_t chunksize, const double *values, const double *weights,
                          int32_t order, int32_t nested, int64_t capacity, int64_t *ipix_out, double *phi_out,
                          double *z_out, double *kappa_out, double *w_out, int64_t *n_selected);

/*
 * Host-only helper of the ingest path (no device, no context): stable grouping of float64 columns by an integer key --
 * what the reference does per chunk with groupby(patch_ids, chunk) (catalog/catalog.py:293, utils/misc.py:40-51) and
 * groupby(bin_idx, chunk) (catalog/trees.py:413), i.e. np.argsort(kind="stable") + a gather per column, here as one
 * threaded counting sort. Entries with key < 0 are dropped (objects outside the binning, trees.py:414).
 *   keys       int32[n] or int64[n] (key_bytes = 4 | 8), every key < num_groups
 *   in, out    n_cols pointers to float64[n] each; out[c] receives the kept entries of in[c], group after group, input
 *              order inside a group; out[c] must not alias in[c]
 *   sizes      int64[num_groups] entries per group (out)
 *   n_threads  0 = one per core, at most 16
 */
int yawhip_host_group_columns(int64_t n, const void *keys, int32_t key_bytes, int64_t num_groups, int32_t n_cols,
                              const double *const *in, double *const *out, int64_t *sizes, int32_t n_threads);

/*
 * Host-only helper of the epilogue: the dense result tensor from the per-job values -- the loop
 * counts[:, id1, id2] = result (x 0.5 on the diagonal of an autocorrelation) of PatchLinkage.count_pairs
 * (correlation/measurements.py:358-364), for all scales and bins at once.
 *   out         float64[n_rows][row_len], zero-filled, then out[r][cols[j]] = vals[r][j] * (col_factor ? col_factor[j] : 1)
 *               (n_rows = scales x bins, row_len = P x P, cols[j] = id1 * P + id2 of job j)
 *   vals        float64, element (r, j) at vals[r * val_row_stride + j * val_col_stride] (strides in elements: the per-job
 *               values arrive job-major from yawhip_count_pairs)
 */
int yawhip_host_scatter_rows(int64_t n_rows, int64_t row_len, double *out, int64_t n_cols, const int64_t *cols,
                             const double *vals, int64_t val_row_stride, int64_t val_col_stride, const double *col_factor);

/*
 * Evaluated pair distances per job, without counting anything: runs the item builder of yawhip_count_pairs for the
 * same arguments and sums lane-tile x window sizes per job (for the brute-force kernels that is N1*N2 per bin).
 * This is the cost the host balances when it shards the job list over GPUs (replaces the "largest jobs first"
 * scheduling heuristic of measurements.py:262-273). work: int64[n_jobs].
 */
int yawhip_job_work(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                    const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                    int64_t *work);

/*
 * Deterministic k-means over ALL objects of a catalogue, columns resident on the device (patches.create_patch_centers,
 * Catalog.from_*(patch_num=..., patch_method="full"); stands in for treecorr's k-means behind create_patch_centers,
 * catalog/catalog.py:183-226). Everything summed over objects is an integer, so the results do not depend on the order of
 * the additions (atomics, grid shape) and equal the numpy route of patches.py bit for bit. Additive to ABI 6.
 * The squared distance of object i and centre c is ((x_i - c_x)^2 + (y_i - c_y)^2) + (z_i - c_z)^2, every product and sum
 * rounded on its own (the arithmetic of yawhip_assign_patches); among equal distances the lowest centre index wins.
 *
 * yawhip_kmeans_open   uploads the columns ONCE (first device of a multi-device context); the other calls move centre
 *                      tables, k-sized results and scalars only (and ids, where asked for).
 *   n        1 .. 2^31 objects;  x, y, z  float64[n] unit vectors (host);  w  float64[n] finite weights (host) or NULL
 *   wscale   with w: the power of two 2^(30 - e), e the binary exponent of max |w| (frexp), so that |w x wscale| <= 2^30
 * yawhip_kmeans_seed   one k-means++ step: m_i = d(i, centre) (first = 1) or min(m_i, d(i, centre)) (first = 0), then
 *                      q_i = floor(m_i * 2^29) as an integer; *total = sum of all q_i (exact).
 * yawhip_kmeans_pick   after a seed: *index = the smallest i whose inclusive prefix sum of q exceeds r; r < total.
 * yawhip_kmeans_step   one Lloyd round against centres[k][3]: id_i = nearest centre; per cluster counts[c] = objects,
 *                      sums[c][axis] = sum of a_i, a_i = rint(x_i * 2^30), with weights rint((w_i * x_i) * wscale)
 *                      (round half to even), all int64; *inertia = sum of floor(d(i, id_i) * 2^29); ids int32[n] (host)
 *                      or NULL. 3 k doubles must fit the LDS (as for yawhip_assign_patches), else YAWHIP_ERR_INVALID.
 *                      Where the per-workgroup partial sums [k][4] fit the LDS beside the centres they are kept there and
 *                      flushed once per workgroup, otherwise every object adds to global memory (integer atomics both).
 * yawhip_kmeans_query  what = 0: objects per segment of the seed sums, 1: path of the last step (0 none, 1 LDS partials,
 *                      2 global atomics), 2: largest k of the LDS-partials path, 3: largest k of yawhip_kmeans_step.
 * yawhip_kmeans_close  frees the handle (NULL: nothing happens). Close it before its context is destroyed.
 */
typedef struct yawhip_kmeans yawhip_kmeans;
int yawhip_kmeans_open(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                       double wscale, yawhip_kmeans **out);
int yawhip_kmeans_seed(yawhip_kmeans *km, const double centre[3], int32_t first, uint64_t *total);
int yawhip_kmeans_pick(yawhip_kmeans *km, uint64_t r, int64_t *index);
int yawhip_kmeans_step(yawhip_kmeans *km, int32_t k, const double *centres, int64_t *sums, int64_t *counts,
                       uint64_t *inertia, int32_t *ids);
int yawhip_kmeans_query(const yawhip_kmeans *km, int32_t what, int64_t *value);
void yawhip_kmeans_close(yawhip_kmeans *km);

/*
 * Tangential and cross shear of a source catalogue around the lenses of a catalogue binned in redshift
 * (measurements.crosscorrelate_shear; no counterpart in the reference). Additive to ABI 6.
 *
 * yawhip_shear_upload   a shear catalogue as an opaque handle on the context (first device of a multi-device context): the
 *                       columns are copied up once, every patch segment is sorted along sort_axis on the device and the
 *                       columns are gathered into that order; the handle keeps x, y, z, w, w * g1 and w * g2 (each product
 *                       one float64 multiply, rounded on its own; g1, g2 when w is NULL).
 *   x, y, z      float64[n] unit vectors (host);  w  float64[n] weights or NULL (every weight 1.0)
 *   g1, g2       float64[n] shear components in the local frame whose first axis points east (+RA) and whose second axis
 *                points north: g1 > 0 stretches along east-west, g2 > 0 along the diagonal between +east and +north
 *   offsets      int64[n_patches + 1] CSR over the patches (these sources are not binned); objects are grouped by patch
 * yawhip_shear_free     frees the handle (NULL: nothing happens). Free it before its context is destroyed.
 * yawhip_shear_count    for every job (lens patch p, source patch q) and redshift bin k, over the pairs (lens l of segment
 *                       (p, k), source s of patch q) with t[k][e] < s2 <= t[k][e + 1] -- s2 and the thresholds exactly those of
 *                       yawhip_count_pairs -- the sums, in float64 with every product and sum rounded on its own,
 *       a = x ly - y lx,  rho2 = x x + y y,  b = rho2 lz - z (x lx + y ly),  den = a a + b b     (x, y, z: the source)
 *       c2 = (a a - b b) / den,  s2p = (2 a b) / den      cos and sin of twice the position angle of the lens seen from the
 *                                                         source, from east towards north
 *       fine_t += w_l * -((w_s g1) c2 + (w_s g2) s2p)     tangential
 *       fine_x += w_l *  ((w_s g1) s2p - (w_s g2) c2)     cross
 *       fine_w += w_l * w_s
 *     A pair with den == 0 (the source on a pole of the frame) adds to fine_w only.
 *   lenses       a resident catalogue of the same context with n_bins_or_1 equal to 1 or n_bins
 *   jobs         int32[n_jobs][2] = (lens patch, source patch);  t  float64[B][E] as for yawhip_count_pairs, E <= 256
 *   fine_t, fine_x, fine_w   float64[n_jobs][B][E-1] each (host); every element is written
 *   stats        may be NULL; candidate / evaluated pairs, workgroups, launches and the times are filled, the rest is 0
 * One workgroup per (job, bin) cell adds into one float64 LDS histogram per wave and stores the cell with plain stores: no
 * floating-point atomics on global memory; the reproducibility note of yawhip_count_pairs' BAND path applies (tested run
 * to run). The count runs on the context's first device. Errors as for yawhip_count_pairs (handles of another context or
 * unequal patch counts: YAWHIP_ERR_MISMATCH), checked before any device work.
 */
typedef struct yawhip_shear_sources yawhip_shear_sources;
int yawhip_shear_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                        const double *g1, const double *g2, int32_t n_patches, const int64_t *offsets, int32_t sort_axis,
                        yawhip_shear_sources **out);
int yawhip_shear_free(yawhip_shear_sources *sources);
int yawhip_shear_count(yawhip_ctx *ctx, const yawhip_catalog *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                       const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, double *fine_t, double *fine_x,
                       double *fine_w, yawhip_stats *stats);

/*
 * Shear-shear sums of ONE shear catalogue inside its own redshift bins: the numerators of xi_plus, xi_minus and of the
 * parity-odd xi_cross (measurements.autocorrelate_shear; no counterpart in the reference). Additive to ABI 6: new symbols
 * only, the opaque handle is the one above.
 *
 * yawhip_shear_upload_binned   yawhip_shear_upload for a catalogue grouped by (patch, redshift bin): offsets is
 *                       int64[n_patches * n_bins + 1], every (patch, bin) segment is sorted along sort_axis. The handle
 *                       carries n_bins; yawhip_shear_upload is the n_bins = 1 case. yawhip_shear_count refuses a handle with
 *                       n_bins != 1 (YAWHIP_ERR_MISMATCH).
 * yawhip_shear_auto_count      objects a, b of the same redshift bin k, unit vectors (ax, ay, az), (bx, by, bz), weights w (1.0
 *                       without a weight column) and wg1 = w g1, wg2 = w g2 as the upload made them. Pair membership is that
 *                       of every count: s2 = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2, fine bin e iff
 *                       t[k][e] < s2 <= t[k][e + 1] -- a pair at s2 == 0 never counts, an object with itself included. A pair
 *                       in a fine bin adds, in float64 with every product and sum rounded on its own,
 *       pa   = ax by - ay bx                       dot = ax bx + ay by
 *       pbA  = (ax ax + ay ay) bz - az dot         b seen from a: (east, north) cos(dec_a) = (pa, pbA)
 *       pbB  = (bx bx + by by) az - bz dot         a seen from b: (-pa, pbB)
 *       denA = pa pa + pbA pbA                     denB = pa pa + pbB pbB
 *       cA = (pa pa - pbA pbA) / denA   sA = ((2 pa) pbA) / denA        cos, sin of twice the position angle at a
 *       cB = (pa pa - pbB pbB) / denB   sB = ((-2 pa) pbB) / denB       cos, sin of twice the position angle at b
 *       tA = -(wg1a cA + wg2a sA)       xA = wg1a sA - wg2a cA          the shear of a along / across the great circle
 *       tB = -(wg1b cB + wg2b sB)       xB = wg1b sB - wg2b cB
 *       fine_p += tA tB + xA xB     fine_m += tA tB - xA xB     fine_c += tA xB + xA tB     fine_w += w_a w_b
 *     denA == 0 or denB == 0 (one of the two on a pole of the frame): fine_w only. All four terms are bit-symmetric under
 *     swapping a and b. Cell (job (p, q), bin k, fine bin e) holds the sum over the pairs a in (p, k), b in (q, k) for p < q,
 *     and over every UNORDERED pair {a, b} of segment (p, k) once for p == q (what an autocorrelation count holds after its
 *     x 0.5 of the diagonal).
 *   jobs         int32[n_jobs][2] with p <= q;  n_bins must be the handle's;  t  float64[B][E] as for yawhip_count_pairs,
 *                E <= 256 (58 KiB of LDS at the cap: two stages of 48-byte objects, thresholds, four histograms [4][E-1])
 *   fine_p, fine_m, fine_c, fine_w   float64[n_jobs][B][E-1] each (host); every element is written, a cell with an empty
 *                segment is exactly 0
 *   stats        as for yawhip_shear_count; candidate pairs count a diagonal cell's unordered pairs
 * Kernel, accumulation and reproducibility as yawhip_shear_count (one workgroup per (job, bin) cell, one float64 LDS
 * histogram per wave, plain stores); a diagonal cell walks only partners with a larger index. Errors: the checks of
 * yawhip_shear_count, a job with p > q: YAWHIP_ERR_INVALID, a handle with another bin count: YAWHIP_ERR_MISMATCH.
 */
int yawhip_shear_upload_binned(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                               const double *g1, const double *g2, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                               int32_t sort_axis, yawhip_shear_sources **out);
int yawhip_shear_auto_count(yawhip_ctx *ctx, yawhip_shear_sources *sources, int32_t n_jobs, const int32_t *jobs, int32_t n_bins,
                            int32_t n_edges, const double *t, double *fine_p, double *fine_m, double *fine_c, double *fine_w,
                            yawhip_stats *stats);

/*
 * Shear-shear sums between ANY two (patch, redshift bin) segments of one or of two binned shear catalogues: the cross-bin
 * signals xi^{ij} of a tomographic analysis and the correlations between two shape samples
 * (measurements.correlate_shear_tomographic; no counterpart in the reference). Additive to ABI 6: one new symbol.
 *
 * yawhip_shear_pair_count   a, b: two handles of yawhip_shear_upload_binned (or yawhip_shear_upload: one bin) on the context;
 *                       they may be the same handle, and need neither equal patch counts nor equal bin counts nor one sort
 *                       axis. Cell c = (p, q, ka, kb, row) holds, per fine bin e, the sums over the pairs (object a_obj of
 *                       segment (p, ka) of a, object b_obj of segment (q, kb) of b) with t[row][e] < s2 <= t[row][e + 1].
 *                       Membership and the four terms fine_p, fine_m, fine_c, fine_w of a pair are those of
 *                       yawhip_shear_auto_count above, operation by operation, with the same den == 0 rule.
 *     A cell is DIAGONAL iff a == b, ka == kb and p == q: it holds every unordered pair of the segment once. Every other cell
 *     holds every (a_obj, b_obj) once -- also (p, p, k, k) between two different handles. With a == b and ka == kb a cell
 *     with p > q is refused, as a job with p > q is by yawhip_shear_auto_count; cells (p, q, k, k, k) with p <= q on one
 *     handle return the bits of yawhip_shear_auto_count for the jobs (p, q), the same thresholds and bin k.
 *   cells        int32[n_cells][5];  t  float64[n_rows][E] ascending and non-negative per row, E <= 256
 *   fine_p, fine_m, fine_c, fine_w   float64[n_cells][E-1] each (host); every element is written
 *   stats        as for yawhip_shear_auto_count
 * Kernel, accumulation and reproducibility as yawhip_shear_auto_count: one workgroup per cell, (p, ka) of a streamed through
 * LDS and (q, kb) of b in the lanes; the sort-key window is used iff the two handles are sorted along the same axis. The
 * per-call device buffers are those of a. n_cells == 0 returns at once. Errors, before any device work: a patch, bin or row
 * outside its range, thresholds that do not ascend, E > 256, p > q as above: YAWHIP_ERR_INVALID; a handle of another
 * context: YAWHIP_ERR_MISMATCH.
 */
int yawhip_shear_pair_count(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                            int32_t n_rows, int32_t n_edges, const double *t, double *fine_p, double *fine_m, double *fine_c,
                            double *fine_w, yawhip_stats *stats);

/*
 * Excess surface density sums of a source catalogue around the lenses of a catalogue binned in redshift: tangential and
 * cross shear with the per-pair factor Sigma_crit^-1 (z_l, z_s), which is zero for a source in front of its lens
 * (measurements.crosscorrelate_delta_sigma; no counterpart in the reference). Additive to ABI 6: new symbols only, the
 * opaque handle is yawhip_shear_sources.
 *
 * The library is unit-free. For a flat cosmology Sigma_crit^-1 = (4 pi G / c^2) D_A(z_l) max(0, 1 - chi_l / chi_s); the caller
 * passes three extra columns, every entry a finite number >= 0 (else YAWHIP_ERR_INVALID):
 *   lenses:   f (the driver passes D_A(z_l) in Mpc) and c (chi_l in Mpc)
 *   sources:  u (1 / chi_s in 1/Mpc; u = 0 is a source at infinity)
 *
 * yawhip_dsigma_upload_lenses    the lenses as a handle MARKED as lenses: n_bins segments per patch (offsets
 *                       int64[n_patches * n_bins + 1]), every segment sorted along sort_axis and gathered as
 *                       yawhip_shear_upload_binned does; it keeps x, y, z, w (NULL: every weight 1.0) and f, c AS THEY CAME
 *                       (no product with w). Only yawhip_dsigma_count takes it: yawhip_shear_count, yawhip_shear_auto_count
 *                       and yawhip_shear_pair_count refuse it (YAWHIP_ERR_MISMATCH).
 * yawhip_dsigma_upload_sources   yawhip_shear_upload (unbinned: offsets int64[n_patches + 1]) with the extra column u. The
 *                       three shear counts accept the handle and ignore u.
 * Both are freed by yawhip_shear_free.
 * yawhip_dsigma_count   for every job (lens patch p, source patch q) and redshift bin k, over the pairs (lens l of segment
 *                       (p, k) -- (p, 0) when the lenses have one bin --, source s of patch q). Pair membership is the
 *                       predicate of every count, bit for bit: t[k][e] < s2 <= t[k][e + 1]. The rotation and the den == 0
 *                       rule are yawhip_shear_count's, operation by operation:
 *       a = x ly - y lx,  rho2 = x x + y y,  b = rho2 lz - z (x lx + y ly),  den = a a + b b     (x, y, z: the source)
 *       c2 = (a a - b b) / den,  s2p = (2 a b) / den
 *       tv = -((w_s g1) c2 + (w_s g2) s2p)      xv = (w_s g1) s2p - (w_s g2) c2
 *     A pair in fine bin e then adds, in float64 with every product and sum rounded on its own and nothing contracted
 *     (1 - c u is a multiply and a subtract, never an FMA):
 *       eff = 1.0 - c_l u_s
 *       if eff > 0.0:                       otherwise the pair adds NOTHING, not to fine_w either
 *           s  = f_l eff
 *           ws = w_l s
 *           fine_t += ws tv                 (den == 0: fine_t and fine_x skipped, fine_w still added)
 *           fine_x += ws xv
 *           fine_w += (ws s) w_s
 *     With f = 1, c = 0 and any u every operation reduces to that of yawhip_shear_count: the call returns its bits.
 *     fine_t / fine_w summed over cells is sum(w_l w_s S gamma_t) / sum(w_l w_s S^2) with S = f (1 - c u): Delta Sigma up to the
 *     constant c^2 / (4 pi G) of the caller's units.
 *   lenses       a handle of yawhip_dsigma_upload_lenses with n_bins equal to 1 or the call's n_bins
 *   sources      a handle of yawhip_dsigma_upload_sources
 *   jobs, t, fine_t, fine_x, fine_w, stats    shapes and meaning as for yawhip_shear_count; every element is written, a cell
 *                without pairs is exactly 0
 * Kernel, accumulation and reproducibility as yawhip_shear_count: the same streaming walk with the lens segment (48-byte
 * objects x, y, z, w, f, c) going through LDS and the sources with u in the lanes, one float64 LDS histogram per wave, plain
 * stores, no floating-point atomics on global memory; the sort-key window is used iff both handles are sorted along the same
 * axis and knows nothing of the three columns: the evaluated separations are those of yawhip_shear_count on the same
 * catalogues. The per-call device buffers are those of the sources. Errors, before any device work: the checks of
 * yawhip_shear_count (sizes, thresholds, jobs outside the patches: YAWHIP_ERR_INVALID; handles of another context, unequal
 * patch counts, a lens bin count that is neither 1 nor n_bins: YAWHIP_ERR_MISMATCH); a lens handle given as sources, a source
 * handle without u, or a handle that is not marked as lenses given as lenses: YAWHIP_ERR_MISMATCH.
 */
int yawhip_dsigma_upload_lenses(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                const double *f, const double *c, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                                int32_t sort_axis, yawhip_shear_sources **out);
int yawhip_dsigma_upload_sources(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                 const double *g1, const double *g2, const double *u, int32_t n_patches, const int64_t *offsets,
                                 int32_t sort_axis, yawhip_shear_sources **out);
int yawhip_dsigma_count(yawhip_ctx *ctx, yawhip_shear_sources *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                        const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, double *fine_t, double *fine_x,
                        double *fine_w, yawhip_stats *stats);

/*
 * The excess surface density sums binned in each lens's OWN radius R = D(z_l) theta instead of one angle per redshift slice
 * (measurements.crosscorrelate_delta_sigma(radius="lens")). Additive to ABI 6: new symbols only.
 *
 * yawhip_dsigma_upload_lenses_radial   yawhip_dsigma_upload_lenses with one more column m, float64[n]: the SQUARED transverse
 *                       distance per radian of the lens, in the squared unit of the radii the caller will pass (the library is
 *                       unit-free; the driver passes D_A(z_l)^2 for physical radii). Every m is finite and > 0, else
 *                       YAWHIP_ERR_INVALID (the host pass that checks f and c). The handle keeps m in segment order and, per
 *                       redshift bin, the minimum of m over all patches (one value with n_bins = 1). It is freed by
 *                       yawhip_shear_free; yawhip_dsigma_count accepts it and ignores m; the three shear counts refuse it
 *                       as they refuse any lens handle.
 * yawhip_dsigma_count_radial   yawhip_dsigma_count with r2 in the place of t: float64[n_bins][n_edges] ascending SQUARED radius
 *                       edges per row, finite and >= 0, n_edges <= 256. Jobs, cells, segments, output planes and statistics are
 *                       those of yawhip_dsigma_count. A pair (lens l of segment (p, k), source s of patch q) is handled in
 *                       float64, every operation rounded on its own and nothing contracted:
 *       s2  = ((sx - lx)^2 + (sy - ly)^2) + (sz - lz)^2          the separation of every count, source minus lens
 *       q   = 1/16632;  q = 1/3150 + s2 q;  q = 1/560 + s2 q;  q = 1/90 + s2 q;  q = 1/12 + s2 q;  q = 1 + s2 q
 *       th2 = s2 q                                               (2 asin(sqrt(s2) / 2))^2: the squared angle
 *       R2  = m_l th2
 *       fine bin e  iff  r2[k][e] < R2 <= r2[k][e + 1]           none: the pair adds nothing
 *     (the coefficients are the double quotients 1.0 / 12.0 ... 1.0 / 16632.0). The pair term, the den == 0 rule and the
 *     eff <= 0 rule are yawhip_dsigma_count's, operation by operation.
 *     The series is within 2 * 2^-53 (relative) of the squared angle for s2 <= 0.01, i.e. theta <= 5.73 degrees. The call
 *     refuses larger reaches before any device work: with smax[k] = r2[k][n_edges - 1] / min_m[k] * (1 + 1e-12) (min_m[k] the
 *     handle's minimum of bin k, of its one bin when the lenses are unbinned; a bin without lenses has smax = 0), any
 *     smax[k] > 0.01 is YAWHIP_ERR_INVALID, "a lens is too close for the largest radius".
 *   lenses       a handle of yawhip_dsigma_upload_lenses_radial (one without m: YAWHIP_ERR_MISMATCH)
 * Kernel: the walk of yawhip_dsigma_count with 64-byte streamed objects (x, y, z, m | w, f, c, pad); the sort-key window of
 * row k has the half width sqrt(smax[k]) (1 + 1e-12) + 1e-15, so the evaluated separations follow the NEAREST lens of the bin.
 * Accumulation, reproducibility and every other error are those of yawhip_dsigma_count.
 */
int yawhip_dsigma_upload_lenses_radial(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                                       const double *f, const double *c, const double *m, int32_t n_patches, int32_t n_bins,
                                       const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out);
int yawhip_dsigma_count_radial(yawhip_ctx *ctx, yawhip_shear_sources *lenses, yawhip_shear_sources *sources, int32_t n_jobs,
                               const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *r2, double *fine_t, double *fine_x,
                               double *fine_w, yawhip_stats *stats);

/*
 * Projected pair counts: the pairs of one or two catalogues binned in each PAIR's own transverse radius, inside a cut on the
 * line-of-sight separation -- DD, DR and RR of the projected clustering w_p(r_p) (measurements.autocorrelate_projected;
 * DESIGN.md section 20; no counterpart in the reference). Additive to ABI 6: new symbols only, the opaque handle is
 * yawhip_shear_sources.
 *
 * The library is unit-free. Every object carries two columns besides x, y, z, w:
 *   d   its transverse distance per radian, finite and > 0 (the driver passes D_A(z) or D_A(z) (1 + z) in Mpc)
 *   c   its line-of-sight coordinate, finite (the driver passes the comoving distance chi(z) in Mpc)
 *
 * yawhip_proj_upload    yawhip_dsigma_upload_lenses with the two raw columns read as (d, c), on one code path with it: n_bins
 *                       segments per patch (offsets int64[n_patches * n_bins + 1]), every segment sorted along sort_axis and
 *                       gathered; the handle keeps x, y, z, w (NULL: every weight 1.0) and d, c as they came, is MARKED as
 *                       projected and keeps, per redshift bin, the minimum of d over all patches. A d that is not finite and
 *                       > 0 or a c that is not finite: YAWHIP_ERR_INVALID (a host pass before any device work). Freed by
 *                       yawhip_shear_free. The three shear counts and the two excess-surface-density counts refuse the handle
 *                       (YAWHIP_ERR_MISMATCH); yawhip_proj_count refuses every other handle (YAWHIP_ERR_MISMATCH).
 * yawhip_proj_count     a, b: two projected handles on the context; they may be the same handle, and need neither equal patch
 *                       counts nor equal bin counts nor one sort axis. Cell c = (sa, sb, row, diagonal) holds, per fine bin e,
 *                       the sum over the pairs (object a_obj of segment sa of a, object b_obj of segment sb of b; a segment is
 *                       patch * n_bins + bin of its handle). A pair is handled in float64, every operation rounded on its own
 *                       and nothing contracted:
 *       s2  = ((bx - ax)^2 + (by - ay)^2) + (bz - az)^2          the separation of every count (b_obj minus a_obj)
 *       D   = 0.5 * (d_a + d_b);   DD = D * D
 *       q   = 1/16632;  q = 1/3150 + s2 q;  q = 1/560 + s2 q;  q = 1/90 + s2 q;  q = 1/12 + s2 q;  q = 1 + s2 q
 *       th2 = s2 q                                               the series of yawhip_dsigma_count_radial, the same constants
 *       R2  = DD th2
 *       fine bin e  iff  r2[row][e] < R2 <= r2[row][e + 1]       none: the pair adds nothing
 *       p   = fabs(c_a - c_b);   the pair counts  iff  p <= pmax
 *       fine_w[c][e] += w_a * w_b
 *     Every term is bit-symmetric under swapping the two objects. A cell is DIAGONAL iff a == b and sa == sb: it holds every
 *     unordered pair of the segment once (a pair at R2 == 0, an object with itself included, never counts where r2[row][0]
 *     >= 0). Every other cell holds every (a_obj, b_obj) once. The fourth entry of a cell must say which it is (non-zero:
 *     diagonal), else YAWHIP_ERR_INVALID.
 *     Reach: with least[row] the minimum of d over the redshift bins that the cells of the row pair (0 where a row has no cell
 *     or a bin has no object), smax[row] = r2[row][n_edges - 1] / least[row]^2 * (1 + 1e-12); any smax[row] > 0.01 is
 *     YAWHIP_ERR_INVALID, "an object is too close for the largest radius", before any device work (the cap of
 *     yawhip_dsigma_count_radial: the series is within 2 * 2^-53 of the squared angle up to there).
 *   cells        int32[n_cells][4];  r2  float64[n_rows][n_edges] ascending squared radius edges, finite and >= 0,
 *                n_edges <= 256;  pmax  >= 0, +inf: no line-of-sight cut (negative or NaN: YAWHIP_ERR_INVALID)
 *   fine_w       float64[n_cells][n_edges - 1] (host), ONE plane; every element is written
 *   stats        as for yawhip_shear_pair_count; candidate pairs count a diagonal cell's unordered pairs, and so do the
 *                evaluated pairs: of a diagonal cell the separations inside the key window whose streamed object has the larger
 *                index (the waves also evaluate, and drop, the other order inside a lane tile's own range; the shear counts
 *                report those too). evaluated <= candidates always, with equality where no window is used
 * Kernel: the walk of yawhip_shear_pair_count (one workgroup per cell, segment sa of a streamed through LDS, sb of b in the
 * lanes, a diagonal cell walks only partners with a larger index) with 48-byte streamed objects (x, y, z, d | w, c); the
 * sort-key window is used iff the two handles are sorted along the same axis and has the half width
 * sqrt(smax[row]) (1 + 1e-12) + 1e-15, so the evaluated separations follow the NEAREST object. Accumulation and
 * reproducibility as yawhip_shear_count. The per-call device buffers are those of a. n_cells == 0 returns at once.
 */
int yawhip_proj_upload(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                       const double *d, const double *c, int32_t n_patches, int32_t n_bins, const int64_t *offsets,
                       int32_t sort_axis, yawhip_shear_sources **out);
int yawhip_proj_count(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                      int32_t n_rows, int32_t n_edges, const double *r2, double pmax, double *fine_w, yawhip_stats *stats);

/*
 * Projected pair counts binned in the line-of-sight separation besides: the planes DD, DR and RR of xi(r_p, pi), from which
 * w_p(r_p) = 2 sum_j xi(r_p, pi_j) dpi_j is summed (measurements.autocorrelate_projected(pi_bins=...); DESIGN.md section 22;
 * no counterpart in the reference). Additive to ABI 6: one new symbol.
 *
 * yawhip_proj_count_pi  yawhip_proj_count argument for argument, with the call-wide edges pe float64[n_pi + 1] (host) in the
 *                       place of pmax. s2, D, DD, q, th2, R2 and the fine bin e of a pair are exactly yawhip_proj_count's
 *                       (float64, every operation rounded on its own). Then
 *       p = fabs(c_a - c_b)
 *       j = the number of edges pe[1 .. n_pi] that are < p        plane 0 is [0, pe[1]], plane j is (pe[j], pe[j + 1]]
 *       the pair counts  iff  j < n_pi                            that is, p <= pe[n_pi]
 *       fine_w[j][c][e] += w_a * w_b
 *     p is bit-symmetric, so a diagonal cell holds every unordered pair once, as in yawhip_proj_count. A pair behind the
 *     outer test whose R2 lies beyond the last radius edge is in no plane.
 *     Two consequences: over unit weights the sum over j of fine_w[j] equals the fine_w of yawhip_proj_count with
 *     pmax = pe[n_pi], as integers; and candidate_pairs and evaluated_pairs equal those of that call -- it is the same
 *     walk, with the same window and the same count of a diagonal cell's kept separations.
 *   n_pi, pe     n_pi >= 1; pe[0] exactly 0; pe finite and strictly ascending, except that pe[n_pi] may be +inf (no outer
 *                cut). Anything else (NaN, ties, a NULL pe): YAWHIP_ERR_INVALID.
 *   the cap      a workgroup keeps two stages of 48-byte objects, the n_edges thresholds, the n_pi + 1 pi edges (both
 *                rounded up to an even number of float64) and one histogram [n_pi][n_edges - 1] per wave, four waves, in
 *                the 64 KiB of dynamic LDS of every count here:
 *                  24576 + 8 (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 32 n_pi (n_edges - 1) <= 65536
 *                -- n_pi <= 104 at 13 edges, <= 4 at 256, <= 1023 at 2. A larger n_pi is YAWHIP_ERR_INVALID with a message
 *                that names the largest n_pi that fits at this n_edges; the library does not split a call.
 *   fine_w       float64[n_pi][n_cells][n_edges - 1] (host); every element is written
 *   checks       those of yawhip_proj_count in its order -- handles, sizes and context, both handles projected
 *                (YAWHIP_ERR_MISMATCH), then n_pi and pe and the cap where that call checks pmax, the radius edges, the
 *                cells, the reach. stats, buffers, n_cells == 0: as yawhip_proj_count.
 * Kernel: yawhip_proj_count's, its loop up to the wave-wide test unchanged; the pi edges are staged into LDS once per
 * workgroup, and behind the test p is bisected over them as R2 is over the row. Accumulation and reproducibility as
 * yawhip_shear_count: per-wave LDS histograms, folded in a fixed order, plain stores.
 */
int yawhip_proj_count_pi(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                         int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine_w,
                         yawhip_stats *stats);

/*
 * Redshift-space pair counts: the planes DD, DR and RR of xi(s, mu), from which the multipoles xi_l(s) are summed
 * (measurements.autocorrelate_multipoles; no counterpart in the reference). Additive to ABI 6: one new
 * symbol.
 *
 * yawhip_proj_count_smu  yawhip_proj_count_pi argument for argument: handles (both of yawhip_proj_upload), cell list
 *                        (segment of a, segment of b, row, diagonal), window, diagonal rule and statistics are
 *                        yawhip_proj_count's. The rows s2 float64[n_rows][n_edges] (host) hold SQUARED edges of s, the call-wide
 *                        m2 float64[n_mu + 1] (host) SQUARED edges of mu. s2c (the squared chord), D, DD, th2 and R2 of a pair
 *                        are exactly yawhip_proj_count's (float64, every operation rounded on its own). Then
 *       p = fabs(c_a - c_b),   P2 = p p,   S2 = R2 + P2
 *       e = the fine bin with s2[row][e] < S2 <= s2[row][e + 1]     a pair with S2 beyond the last edge, or not above the
 *                                                                   first, is in no bin
 *       j = the number of INNER edges k = 1 .. n_mu - 1 with fl(m2[k] S2) < P2
 *                                                                   plane 0 is mu^2 in [0, m2[1]], plane j (m2[j], m2[j + 1]]
 *       fine_w[j][c][e] += w_a * w_b
 *     m2 ascends and rounding is monotone, so the predicate holds for a prefix of the edges. m2[0] and m2[n_mu] are never
 *     read by the kernel: fl(R2 + P2) >= P2 always, so every pair inside the s range lands in a plane -- there is no
 *     line-of-sight cut. All terms are bit-symmetric under a <-> b, so a diagonal cell holds every unordered pair once.
 *     Consequences: over unit weights the sum over j of fine_w[j] equals the n_mu = 1 call as integers; on handles whose c
 *     column is constant (p = 0, S2 = R2 exactly) the n_mu = 1 plane is yawhip_proj_count's fine_w at pmax = +inf and every
 *     pair of a several-plane call is in plane 0; candidate_pairs and evaluated_pairs equal those of yawhip_proj_count on
 *     the same cells and table; two objects at one sky position with different c (R2 = 0, S2 = P2) ARE counted, in the last
 *     plane, which yawhip_proj_count never does; exact duplicates (S2 = 0) are in no bin.
 *   n_mu, m2     n_mu >= 1; m2[0] exactly 0 and m2[n_mu] exactly 1; finite and strictly ascending. Anything else (NaN, ties,
 *                a NULL m2): YAWHIP_ERR_INVALID.
 *   the cap      the carve-up of a workgroup's LDS is yawhip_proj_count_pi's with m2 in the place of pe, and so is the cap:
 *                n_mu <= 104 at 13 edges, <= 25 at 51, <= 4 at 256. A larger n_mu is YAWHIP_ERR_INVALID with a message that
 *                names the largest number of mu bins that fits at this n_edges; the library does not split a call.
 *   the reach    R2 <= S2 (P2 >= 0, rounding is monotone), so the reach of the largest s bounds the reach of every counted
 *                pair: the s2 table is checked as yawhip_proj_count checks its radius table, with the same refusals.
 *   fine_w       float64[n_mu][n_cells][n_edges - 1] (host); every element is written
 *   checks       those of yawhip_proj_count_pi in its order, with n_mu and m2 and the cap where that call checks n_pi and
 *                pe. stats, buffers, n_cells == 0: as yawhip_proj_count.
 * Kernel: the walk of yawhip_proj_count with an outer test that knows the line of sight: the wave-wide test holds
 * fl(fl(DD s2c) + P2) against the row's last edge -- an exact superset of the pairs in range, since fl(DD s2c) <= R2 and the
 * one sum is rounded monotonely (an FMA of p, p and DD s2c would not be: it adds the unrounded square). Accumulation and
 * reproducibility as yawhip_shear_count: per-wave LDS histograms, folded in a fixed order, plain stores.
 */
int yawhip_proj_count_smu(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                          int32_t n_rows, int32_t n_edges, const double *s2, int32_t n_mu, const double *m2, double *fine_w,
                          yawhip_stats *stats);

/*
 * The two counts above BETWEEN two samples, with a signed line of sight: the planes D1D2, D1R2, R1D2 and R1R2 of
 * xi(r_p, pi) and xi(s, mu) of two different tracers, which are not symmetric in pi and have odd multipoles
 * (measurements.crosscorrelate_projected / crosscorrelate_multipoles with signed=True; no counterpart in
 * the reference). Additive to ABI 6: two new symbols.
 *
 * Both take yawhip_proj_count_pi's arguments one for one. Handles (both of yawhip_proj_upload, nothing is uploaded again),
 * cells (sa, sb, row, diagonal), the rows of squared radius / s edges, the reach rule, the window, the statistics, the outer
 * (wave-wide) tests, the accumulation and the output layout [n][n_cells][n_edges - 1] are those of the unsigned siblings.
 * Every operation is float64, rounded on its own, nothing contracted.
 *       ps = c_b - c_a                 b_obj an object of the SECOND handle, a_obj one of the first: "b minus a", as s2 is
 *                                      defined. The sign belongs to the handle order of the call; it does not depend on
 *                                      which side the kernel streams. fabs(ps) is the siblings' p bit for bit, so R2, P2
 *                                      and S2 are the siblings' values.
 *   cells        a segment against itself has no order: a cell whose fourth entry is non-zero, or with a == b and sa == sb,
 *                is YAWHIP_ERR_INVALID. Every cell holds every (a_obj, b_obj) once. Swapping the handles, the cells' first
 *                two columns and the edges for their negatives in reverse order gives the planes in reverse order.
 *
 * yawhip_proj_count_pi_signed   R2 and the fine bin e are yawhip_proj_count's. Then
 *       the pair counts  iff  pe[0] <= ps <= pe[n_pi]
 *       j = the number of INNER edges pe[1 .. n_pi - 1] that are < ps     plane 0 is [pe[0], pe[1]], plane j (pe[j], pe[j + 1]]
 *       fine_w[j][c][e] += w_a * w_b
 *     Only the inner edges are bisected (at n_pi == 1 nothing is); the two cuts are asked first.
 *     Consequence: over edges mirrored about 0, pe = {-q[n] .. -q[1], 0, q[1] .. q[n]}, and where no pair has ps == 0 or lies on
 *     an edge, fine_w[n + j] + fine_w[n - 1 - j] equals plane j of yawhip_proj_count_pi at the edges q, as integers over unit
 *     weights (a pair at ps == 0 is in plane n - 1 here; a pair at ps == -q[j] is in plane n - 1 - j, the mirror of the
 *     unsigned plane j, where the unsigned call has p == q[j] in plane j - 1).
 *   n_pi, pe     n_pi >= 1; pe finite and strictly ascending, of any sign: pe[0] may be negative, zero or positive (a one-
 *                sided range). Anything else (NaN, an infinity, ties, a NULL pe): YAWHIP_ERR_INVALID.
 *   the cap      yawhip_proj_count_pi's formula with the signed bins counted as they are: n_pi <= 104 at 13 edges, <= 25 at
 *                51, <= 4 at 256; the same refusal.
 *
 * yawhip_proj_count_smu_signed  S2 and the fine bin e are yawhip_proj_count_smu's (by the UNSIGNED S2). The host passes the
 *                        signed squares sm2[k] = copysign(mu_k mu_k, mu_k). Then
 *       sP2 = copysign(P2, ps)
 *       j = the number of INNER edges k = 1 .. n_mu - 1 with fl(sm2[k] S2) < sP2
 *                                                                   plane 0 is mu in [-1, mu_1], plane j is (mu_j, mu_j+1]
 *       fine_w[j][c][e] += w_a * w_b
 *     sm2 ascends, S2 >= 0 and rounding is monotone, so fl(sm2[k] S2) ascends with k and the predicate holds for a prefix of
 *     the edges whatever the sign of sP2 (for ps < 0 the negative edges, whose squares descend; for ps > 0 every negative
 *     edge and then a prefix of the others). sm2[0] and sm2[n_mu] are never read: there is no cut.
 *     yawhip_proj_count_smu is the special case in which all signs are positive: the predicate then reads fl(m2[k] S2) < P2.
 *     A pair with c_a == c_b has ps == +0 and sP2 == +0 whichever handle comes first: every product of a negative edge is
 *     below it, fl(+-0 S2) < +0 fails, so the pair is in the plane whose UPPER edge is the first one >= 0 -- at an edge
 *     mu == 0 (of either sign of zero) the plane below it, which is closed above. Exchanging the handles and passing
 *     -sm2 reversed therefore mirrors the planes of every pair but these, which stay below 0 in both calls.
 *     Consequence: over edges mirrored about 0 and where no pair has ps == 0 and no product fl(m2[k] S2) equals P2,
 *     fine_w[n + j] + fine_w[n - 1 - j] equals plane j of yawhip_proj_count_smu at the edges m2, as integers over unit weights.
 *   n_mu, sm2    n_mu >= 1; sm2[0] exactly -1 and sm2[n_mu] exactly 1; strictly ascending -- a sequence of mu that does not
 *                ascend strictly after squaring is refused, as yawhip_proj_count_smu refuses it. Anything else (NaN, ties, a
 *                NULL sm2): YAWHIP_ERR_INVALID.
 *   the cap, the reach   yawhip_proj_count_smu's.
 *   checks       those of the sibling in its order, with the refusal of diagonal cells after the edges.
 * Kernels: the siblings' walks without diagonal cells; the lane carries the lower cut pe[0] next to the upper one.
 */
int yawhip_proj_count_pi_signed(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells,
                                const int32_t *cells, int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi,
                                const double *pe, double *fine_w, yawhip_stats *stats);
int yawhip_proj_count_smu_signed(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells,
                                 const int32_t *cells, int32_t n_rows, int32_t n_edges, const double *s2, int32_t n_mu,
                                 const double *sm2, double *fine_w, yawhip_stats *stats);

/*
 * Projected position-shape sums: the tangential and cross ellipticity of the shapes of one catalogue about the objects of
 * another, binned in each PAIR's own radius and in the line-of-sight separation -- the planes of the intrinsic-alignment
 * measurement w_g+(r_p) and its null test w_gx(r_p) (measurements.crosscorrelate_alignment; no
 * counterpart in the reference). Additive to ABI 6: two new symbols.
 *
 * yawhip_proj_upload_shapes  yawhip_proj_upload with the shear columns g1, g2 (east / north frame, as yawhip_shear_upload)
 *                        besides d, c, on the one code path of every upload: the handle keeps x, y, z, w (NULL: every
 *                        weight 1.0), the products w g1, w g2 each rounded on its own (as a handle of yawhip_shear_upload
 *                        makes them), d and c as they came and, per redshift bin, the minimum of d over all patches. g1, g2
 *                        or c not finite, or a d that is not finite and > 0: YAWHIP_ERR_INVALID (a host pass before any
 *                        device work). The handle is MARKED as a shape handle: freed by yawhip_shear_free, and refused by
 *                        every other count of this header (YAWHIP_ERR_MISMATCH).
 * yawhip_proj_count_shear    dens: a handle of yawhip_proj_upload, as it is -- a density sample or its randoms that sit on
 *                        the device for yawhip_proj_count are not uploaded again; shapes: a handle of
 *                        yawhip_proj_upload_shapes. The wrong kind in either slot is YAWHIP_ERR_MISMATCH. Cell
 *                        c = (segment of dens, segment of shapes, row, 0): the fourth entry must be 0, two handles of
 *                        different kinds never pair a segment with itself (else YAWHIP_ERR_INVALID). With a the shape and b
 *                        the density object, s2, D, DD, q, th2, R2 and the fine bin e are exactly yawhip_proj_count's, p and
 *                        j exactly yawhip_proj_count_pi's (float64, every operation rounded on its own, nothing contracted):
 *       p = fabs(c_a - c_b);   j = the number of edges pe[1 .. n_pi] that are < p;   the pair counts  iff  j < n_pi
 *       pa = ax by - ay bx;   dot = ax bx + ay by;   pb = (ax ax + ay ay) bz - az dot
 *       a2 = pa pa;   b2 = pb pb;   den = a2 + b2
 *       den != 0:   c2 = (a2 - b2) / den;   s2p = ((2 pa) pb) / den
 *                   tv = -(wg1_a c2 + wg2_a s2p);   xv = wg1_a s2p - wg2_a c2
 *                   T[j][c][e] += w_b tv;   X[j][c][e] += w_b xv
 *       W[j][c][e] += w_b w_a                                     (den == 0, the shape on a pole of the frame: W only)
 *     This is yawhip_shear_count's pair term, term for term, with the density object in the place of the lens: T is the
 *     tangential ellipticity of the shape about the density object (negative for a shape that points at it). A shape and a
 *     density object at one sky position have R2 == 0 and are in no bin, so a sample that serves as both sides never pairs
 *     an object with itself. Consequences: with g == 0 T and X are exactly 0; (g1, g2) -> (-g2, g1) gives T' == -X and
 *     X' == T bit for bit; over unit weights W equals yawhip_proj_count_pi's planes on the shapes' (x, y, z, w, d, c) as
 *     integers, and candidate_pairs and evaluated_pairs equal that call's.
 *   n_pi, pe     as yawhip_proj_count_pi; the single cylinder |pi| <= pmax is n_pi = 1, pe = {0, pmax}
 *   the cap      the carve-up of yawhip_proj_count_pi with three planes per pi bin:
 *                  24576 + 8 (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 96 n_pi (n_edges - 1) <= 65536
 *                -- n_pi <= 35 at 13 edges, <= 8 at 51, <= 1 at 256, <= 393 at 2. A larger n_pi is YAWHIP_ERR_INVALID with a
 *                message that names the largest n_pi that fits at this n_edges; the library does not split a call.
 *   fine         float64[3][n_pi][n_cells][n_edges - 1] (host), the planes in the order T, X, W; every element is written
 *   checks       those of yawhip_proj_count_pi in its order, with the two kinds where that call asks for two projected
 *                handles. r2, the reach rule and its refusal, stats, n_cells == 0: as yawhip_proj_count_pi. The per-call
 *                device buffers are those of dens.
 * Kernel: yawhip_proj_count_pi's walk with dens streamed and the shapes in the lanes; its loop up to the wave-wide test is
 * unchanged (fl(DD s2) against the row's last edge, an exact superset). Behind it R2 and p are bisected as there, and only a
 * pair that counts is rotated. Accumulation and reproducibility as yawhip_shear_count: per-wave LDS histograms, folded in a
 * fixed order, plain stores.
 */
int yawhip_proj_upload_shapes(yawhip_ctx *ctx, int64_t n, const double *x, const double *y, const double *z, const double *w,
                              const double *g1, const double *g2, const double *d, const double *c, int32_t n_patches, int32_t n_bins,
                              const int64_t *offsets, int32_t sort_axis, yawhip_shear_sources **out);
int yawhip_proj_count_shear(yawhip_ctx *ctx, yawhip_shear_sources *dens, yawhip_shear_sources *shapes, int32_t n_cells,
                            const int32_t *cells, int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe,
                            double *fine, yawhip_stats *stats);

/*
 * Projected shape-shape sums: the products of the ellipticities of two shapes, BOTH rotated to the great circle through the
 * pair, binned in each PAIR's own radius and in the line-of-sight separation -- the planes of the intrinsic-alignment
 * measurements w_++(r_p) and w_xx(r_p) and of the parity-odd null test w_+x (measurements.autocorrelate_alignment; DESIGN.md
 * section 25; no counterpart in the reference). Additive to ABI 6: one new symbol, no new upload and no new handle kind.
 *
 * yawhip_proj_count_shapes   a (streamed) and b (in the lanes): handles of yawhip_proj_upload_shapes, which may be ONE handle;
 *                        they need neither equal patch counts, nor equal bin counts, nor one sort axis. Any other kind in
 *                        either slot is YAWHIP_ERR_MISMATCH. Cell c = (segment of a, segment of b, row, diagonal) with the
 *                        rules of yawhip_proj_count: a cell is diagonal iff a == b and the two segments are one segment, it
 *                        then holds every unordered pair once, and a wrong flag is refused as there. s2, D, DD, q, th2, R2
 *                        and the fine bin e are exactly yawhip_proj_count's, p and j exactly yawhip_proj_count_pi's, and the
 *                        pair term is yawhip_shear_auto_count's up to tA, xA, tB, xB (float64, every operation rounded on
 *                        its own, nothing contracted):
 *       p = fabs(c_a - c_b);   j = the number of edges pe[1 .. n_pi] that are < p;   the pair counts  iff  j < n_pi
 *       pa = ax by - ay bx;   dot = ax bx + ay by
 *       pbA = (ax ax + ay ay) bz - az dot;   pbB = (bx bx + by by) az - bz dot
 *       a2 = pa pa;   bA2 = pbA pbA;   bB2 = pbB pbB;   denA = a2 + bA2;   denB = a2 + bB2
 *       denA != 0 and denB != 0:
 *                   cA = (a2 - bA2) / denA;   sA = ((2 pa) pbA) / denA;   cB = (a2 - bB2) / denB;   sB = ((-2 pa) pbB) / denB
 *                   tA = -(wg1_a cA + wg2_a sA);   xA = wg1_a sA - wg2_a cA
 *                   tB = -(wg1_b cB + wg2_b sB);   xB = wg1_b sB - wg2_b cB
 *                   PP[j][c][e] += tA tB;   XX[j][c][e] += xA xB;   PX[j][c][e] += tA xB + xA tB
 *       W[j][c][e] += w_a w_b                  (denA == 0 or denB == 0, a shape on a pole of the frame: W only)
 *     The planes are ++, xx and +x separately, not xi_+ / xi_-: the estimator wants ++ and xx apart. All four terms are
 *     BIT-SYMMETRIC under a <-> b (products and two-operand sums commute; pa changes its sign and enters as pa pa and as
 *     (2 pa) pbA against (-2 pa) pbB; pbA and pbB swap), so it does not matter which of the two objects a lane holds, and a
 *     diagonal cell walks every unordered pair once. Consequences: with g == 0 on either side PP, XX and PX are exactly 0;
 *     (g1, g2) -> (-g2, g1) on both sides gives PP' == XX, XX' == PP and PX' == -PX bit for bit; over unit weights W equals
 *     yawhip_proj_count_pi's planes on the same (x, y, z, w, d, c) as integers, and candidate_pairs and evaluated_pairs equal
 *     that call's, diagonal cells included; two objects at one sky position have R2 == 0 and are in no bin.
 *   n_pi, pe     as yawhip_proj_count_pi; the single cylinder |pi| <= pmax is n_pi = 1, pe = {0, pmax}
 *   the cap      two stages of 64-byte streamed objects (x, y, z, d | w, c, wg1, wg2) and four planes per pi bin:
 *                  32768 + 8 (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 128 n_pi (n_edges - 1) <= 65536
 *                -- n_pi <= 21 at 13 edges, <= 5 at 51, <= 1 at 241, <= 240 at 2; above n_edges = 241 not even one pi bin
 *                fits. A larger n_pi is YAWHIP_ERR_INVALID with a message that names the largest n_pi that fits at this
 *                n_edges, or, where none does, the largest n_edges at one pi bin; the library does not split a call.
 *   fine         float64[4][n_pi][n_cells][n_edges - 1] (host), the planes in the order PP, XX, PX, W; every element is written
 *   checks       those of yawhip_proj_count_pi in its order, with the shape kind where that call asks for two projected
 *                handles. r2, the reach rule and its refusal, stats, n_cells == 0: as yawhip_proj_count_pi. The per-call
 *                device buffers are those of a.
 * Kernel: yawhip_proj_count_shear's walk with a shape handle streamed too; its loop up to the wave-wide test is unchanged
 * (fl(DD s2) against the row's last edge, an exact superset) and reads the first 32 bytes of the streamed object. Behind it
 * R2 and p are bisected as there, the lower half of a diagonal cell is dropped, and only a pair that counts is rotated.
 * Accumulation and reproducibility as yawhip_shear_count: per-wave LDS histograms, folded in a fixed order, plain stores.
 */
int yawhip_proj_count_shapes(yawhip_ctx *ctx, yawhip_shear_sources *a, yawhip_shear_sources *b, int32_t n_cells, const int32_t *cells,
                             int32_t n_rows, int32_t n_edges, const double *r2, int32_t n_pi, const double *pe, double *fine,
                             yawhip_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* YAWHIP_H */
