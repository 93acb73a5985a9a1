// yawhip_api.hip -- the entry points of include/yawhip.h that touch no count kernel: error reporting (fail,
// yawhip_last_error), contexts and their options, the argument checks in front of yawhip_hist.hip (redshift histograms),
// yawhip_healpix.hip (HEALPix maps and pixels) and yawhip_random.hip (random catalogues), and the host-side grouping and
// scatter of catalogue columns (yawhip_host_*). Those units run on the context's stream; this one owns their error reporting.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "yawhip_internal.h"
#include "yawhip_hist.h"
#include "yawhip_random.h"

namespace yawhip_detail {

thread_local Trace g_trace;
thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace yawhip_detail

using namespace yawhip_detail;

namespace {
// Host-side grouping of catalogue columns (no device involved): a stable counting sort by key, run by a few threads.
// Chunk c of the input counts its keys; group g then holds the entries of chunk 0, chunk 1, ... in input order, so every
// chunk knows where its entries of every group go and scatters all columns in one pass over its slice.
template <typename K>
static int group_columns(int64_t n, const K *keys, int64_t num_groups, int32_t n_cols, const double *const *in, double *const *out,
                         int64_t *sizes, int n_threads) {
    const int64_t min_chunk = 1 << 16;
    int T = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, (n + min_chunk - 1) / min_chunk));
    std::vector<std::vector<int64_t>> hist((size_t)T, std::vector<int64_t>((size_t)num_groups, 0));
    std::atomic<int> bad{0};
    auto bounds = [&](int c) { return std::make_pair(n * c / T, n * (c + 1) / T); };
    auto run = [&](auto &&fn) {
        if (T == 1) { fn(0); return; }
        std::vector<std::thread> th;
        for (int c = 0; c < T; ++c) th.emplace_back(fn, c);
        for (auto &t : th) t.join();
    };
    run([&](int c) {
        auto [lo, hi] = bounds(c);
        int64_t *h = hist[(size_t)c].data();
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t k = (int64_t)keys[i];
            if (k >= num_groups) { bad.store(1); return; }
            if (k >= 0) ++h[k];
        }
    });
    if (bad.load()) return fail(YAWHIP_ERR_INVALID, "yawhip_host_group_columns: key >= num_groups");
    int64_t at = 0;
    for (int64_t g = 0; g < num_groups; ++g) {
        int64_t size = 0;
        for (int c = 0; c < T; ++c) {
            const int64_t cnt = hist[(size_t)c][(size_t)g];
            hist[(size_t)c][(size_t)g] = at + size;  // first slot of chunk c in group g
            size += cnt;
        }
        sizes[g] = size;
        at += size;
    }
    if (n_cols > 0)
        run([&](int c) {
            auto [lo, hi] = bounds(c);
            int64_t *h = hist[(size_t)c].data();
            for (int64_t i = lo; i < hi; ++i) {
                const int64_t k = (int64_t)keys[i];
                if (k < 0) continue;
                const int64_t dst = h[k]++;
                for (int32_t col = 0; col < n_cols; ++col) out[col][dst] = in[col][i];
            }
        });
    return YAWHIP_OK;
}

// What the HEALPix entry points check alike (`fn`: the name in the message); YAWHIP_OK or the failure.
int check_healpix_order(const char *fn, int32_t order) {
    if (order < 0 || order > yawpix::MAX_ORDER) return fail(YAWHIP_ERR_INVALID, "%s: order %d outside 0 .. %d", fn, order, yawpix::MAX_ORDER);
    return YAWHIP_OK;
}
int check_healpix_nested(const char *fn, int32_t nested) {
    if (nested != 0 && nested != 1) return fail(YAWHIP_ERR_INVALID, "%s: nested must be 0 or 1", fn);
    return YAWHIP_OK;
}
// objects (pixels) per pass of the two: the caller's, the default for 0, at most MAX_CHUNK
int64_t healpix_chunk(int64_t chunksize) { return std::min(chunksize > 0 ? chunksize : yawpix::DEFAULT_CHUNK, yawpix::MAX_CHUNK); }

}  // namespace

// ================================================================================================
extern "C" {

const char *yawhip_last_error(void) { return g_last_error.c_str(); }
int yawhip_abi_version(void) { return YAWHIP_ABI_VERSION; }

int yawhip_device_count(int *n) {
    if (!n) return fail(YAWHIP_ERR_INVALID, "yawhip_device_count: n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(YAWHIP_ERR_NO_DEVICE, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *n = c;
    return YAWHIP_OK;
}

int yawhip_ctx_create(int device_id, yawhip_ctx **out) {
    if (!out) return fail(YAWHIP_ERR_INVALID, "yawhip_ctx_create: out is NULL");
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0)
        return fail(YAWHIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is mandatory; there is no CPU fallback)");
    if (device_id < 0 || device_id >= c)
        return fail(YAWHIP_ERR_NO_DEVICE, "device id %d out of range [0,%d)", device_id, c);
    HIP_TRY(hipSetDevice(device_id));
    yawhip_ctx *ctx = new (std::nothrow) yawhip_ctx();
    if (!ctx) return fail(YAWHIP_ERR_OOM, "host allocation failed");
    ctx->device = device_id;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = ctx->make_events();
    if (e != hipSuccess) {
        delete ctx;
        return fail(YAWHIP_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        if (prop.sharedMemPerBlock > 0) ctx->lds_limit = (int)std::min<size_t>(prop.sharedMemPerBlock, 160 * 1024);
        if (prop.multiProcessorCount > 0) ctx->n_cu = prop.multiProcessorCount;
    }
    *out = ctx;
    return YAWHIP_OK;
}

int yawhip_ctx_destroy(yawhip_ctx *ctx) {
    if (!ctx) return YAWHIP_OK;
    for (yawhip_ctx *peer : ctx->peers) (void)yawhip_ctx_destroy(peer);
    ctx->peers.clear();
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    drop_plans(ctx, nullptr);
    ctx->release_all();
    for (CallBufs &pb : ctx->parked) pb.release_all();
    ctx->d_jobwork.release();
    ctx->d_full.release();
    ctx->d_rowidx.release();
    ctx->sort_ws.release();
    ctx->pix_ws.release();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return YAWHIP_OK;
}

int yawhip_ctx_set_option(yawhip_ctx *ctx, const char *key, int64_t value) {
    if (!ctx || !key) return fail(YAWHIP_ERR_INVALID, "yawhip_ctx_set_option: NULL argument");
    // The option is checked before anything changes: a refused key or value leaves plans, option set and devices as they were.
    std::function<void(yawhip_ctx &)> set;
    auto flag = [&](int yawhip_ctx::*field) { set = [=](yawhip_ctx &c) { c.*field = value != 0; }; };
    auto number = [&](int yawhip_ctx::*field) { set = [=](yawhip_ctx &c) { c.*field = (int)value; }; };
    if (!strcmp(key, "half_bands")) {
        flag(&yawhip_ctx::half_bands);
    } else if (!strcmp(key, "tile_r")) {
        if (value != 0 && value != 1 && value != 2 && value != 4)
            return fail(YAWHIP_ERR_INVALID, "tile_r must be 0 (auto), 1, 2 or 4");
        number(&yawhip_ctx::tile_r);
    } else if (!strcmp(key, "band_batch_log2")) {
        if (value < -1 || value > 6) return fail(YAWHIP_ERR_INVALID, "band_batch_log2 must be -1 (auto) or 0..6");
        number(&yawhip_ctx::band_batch_log2);
    } else if (!strcmp(key, "hist_copies_log2")) {
        if (value < -1 || value > 6) return fail(YAWHIP_ERR_INVALID, "hist_copies_log2 must be -1 (auto) or 0..6");
        number(&yawhip_ctx::hist_copies_log2);
    } else if (!strcmp(key, "triple_runs")) {  // 0: never, 1: where the merged window fits the stage, 2: wherever the partner strips are c - 1, c, c + 1
        if (value < 0 || value > 2) return fail(YAWHIP_ERR_INVALID, "triple_runs must be 0, 1 or 2");
        number(&yawhip_ctx::triple_runs);
    } else if (!strcmp(key, "item_segments")) {
        flag(&yawhip_ctx::item_segments);
    } else if (!strcmp(key, "spin_wait")) {
        flag(&yawhip_ctx::spin_wait);
    } else if (!strcmp(key, "band_cap")) {
        if (const int rc = check_band_cap(value)) return rc;
        number(&yawhip_ctx::band_cap);
    } else if (!strcmp(key, "strip_grid")) {  // 1: latitude, 0: linear in v (catalogues uploaded afterwards)
        if (value != 0 && value != 1) return fail(YAWHIP_ERR_INVALID, "strip_grid must be 0 (linear in v) or 1 (latitude)");
        number(&yawhip_ctx::strip_grid);
    } else if (!strcmp(key, "band_trim")) {
        if (value != 0 && value != 1) return fail(YAWHIP_ERR_INVALID, "band_trim must be 0 or 1");
        number(&yawhip_ctx::band_trim);
    } else if (!strcmp(key, "strip_width_micro")) {  // strip grid spacing in units of 1e-6 rad (latitude grid) or chord (0 = off)
        if (value != 0 && (value < 1000 || value > 2000000))
            return fail(YAWHIP_ERR_INVALID, "strip_width_micro must be 0 (off) or in [1e3, 2e6]");
        set = [=](yawhip_ctx &c) { c.strip_width = (double)value * 1e-6; };
    } else if (!strcmp(key, "seg_strips_min_run")) {
        if (value < 1) return fail(YAWHIP_ERR_INVALID, "seg_strips_min_run must be >= 1");
        set = [=](yawhip_ctx &c) { c.seg_min_run = (int)std::min<int64_t>(value, INT32_MAX); };
    } else if (!strcmp(key, "seg_strips")) {
        flag(&yawhip_ctx::seg_strips);
    } else if (!strcmp(key, "debug_no_hits")) {
        flag(&yawhip_ctx::debug_no_hits);
    } else if (!strcmp(key, "auto_orient")) {
        flag(&yawhip_ctx::auto_orient);
    } else if (!strcmp(key, "slab_budget_bytes")) {
        if (value < 4096) return fail(YAWHIP_ERR_INVALID, "slab_budget_bytes must be >= 4096");
        set = [=](yawhip_ctx &c) { c.slab_budget = value; };
    } else if (!strcmp(key, "band_grid_div")) {
        if (value < 0 || value > 64) return fail(YAWHIP_ERR_INVALID, "band_grid_div must be 0 (auto) or in [1, 64]");
        number(&yawhip_ctx::band_grid_div);
    } else if (!strcmp(key, "flush_stages_log2")) {
        if (value < 0 || value > 17) return fail(YAWHIP_ERR_INVALID, "flush_stages_log2 must be in [0, 17]");
        number(&yawhip_ctx::flush_log2);
    } else if (!strcmp(key, "band_fp32")) {
        flag(&yawhip_ctx::band_fp32);
    } else if (!strcmp(key, "hist_chunk_log2")) {
        if (value < 8 || value > 30) return fail(YAWHIP_ERR_INVALID, "hist_chunk_log2 must be in [8, 30]");
        number(&yawhip_ctx::hist_chunk_log2);
    } else if (!strcmp(key, "kernel")) {
        if (value < YAWHIP_KERNEL_AUTO || value > YAWHIP_KERNEL_BAND)
            return fail(YAWHIP_ERR_INVALID, "unknown kernel id %lld", (long long)value);
        number(&yawhip_ctx::default_kernel);
    } else {
        return fail(YAWHIP_ERR_INVALID, "unknown option '%s'", key);
    }
    std::vector<yawhip_ctx *> devices(ctx->peers);  // every device of a multi-device context follows
    devices.push_back(ctx);
    for (yawhip_ctx *c : devices) {
        ++c->opt_gen;  // options change every decision of a plan and the work per job
        drop_plans(c, nullptr);
        set(*c);
    }
    return YAWHIP_OK;
}

int yawhip_ctx_create_multi(const int *device_ids, int n_devices, yawhip_ctx **out) {
    if (!out) return fail(YAWHIP_ERR_INVALID, "yawhip_ctx_create_multi: out is NULL");
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return fail(YAWHIP_ERR_INVALID, "yawhip_ctx_create_multi: 1 to 64 device ids");
    yawhip_ctx *ctx = nullptr;
    int rc = yawhip_ctx_create(device_ids[0], &ctx);
    if (rc != YAWHIP_OK) return rc;
    for (int i = 1; i < n_devices; ++i) {
        yawhip_ctx *peer = nullptr;
        rc = yawhip_ctx_create(device_ids[i], &peer);
        if (rc != YAWHIP_OK) {
            yawhip_ctx_destroy(ctx);
            return rc;
        }
        ctx->peers.push_back(peer);
    }
    *out = ctx;
    return YAWHIP_OK;
}

int yawhip_ctx_device_count(const yawhip_ctx *ctx, int *n) {
    if (!ctx || !n) return fail(YAWHIP_ERR_INVALID, "yawhip_ctx_device_count: NULL argument");
    *n = (int)ctx->peers.size() + 1;
    return YAWHIP_OK;
}

int yawhip_redshift_histogram(yawhip_ctx *ctx, int64_t n, const double *z, const double *w, int32_t n_patches,
                              const int64_t *offsets, int32_t n_edges, const double *edges, int32_t closed_right, double *out) {
    if (!ctx || !offsets || !edges || !out) return fail(YAWHIP_ERR_INVALID, "yawhip_redshift_histogram: NULL argument");
    if (n < 0 || n_patches < 1 || n_edges < 2 || (n > 0 && !z))
        return fail(YAWHIP_ERR_INVALID, "yawhip_redshift_histogram: bad sizes (n=%lld n_patches=%d n_edges=%d) or NULL z",
                    (long long)n, n_patches, n_edges);
    if (closed_right != 0 && closed_right != 1) return fail(YAWHIP_ERR_INVALID, "yawhip_redshift_histogram: closed_right must be 0 or 1");
    if (offsets[0] != 0 || offsets[n_patches] != n) return fail(YAWHIP_ERR_INVALID, "offsets must start at 0 and end at n");
    for (int32_t p = 0; p < n_patches; ++p)
        if (offsets[p + 1] < offsets[p]) return fail(YAWHIP_ERR_INVALID, "offsets must be non-decreasing");
    for (int32_t i = 0; i + 1 < n_edges; ++i)
        if (!(edges[i + 1] > edges[i])) return fail(YAWHIP_ERR_INVALID, "bin edges must increase strictly (edge %d)", i + 1);
    HIP_TRY(hipSetDevice(ctx->device));
    yawhist::HistCall c;
    c.n = n, c.z = z, c.w = w;
    c.n_patches = n_patches, c.offsets = offsets;
    c.n_edges = n_edges, c.edges = edges, c.closed_right = closed_right;
    c.chunk_log2 = ctx->hist_chunk_log2;
    c.out = out;
    const hipError_t e = yawhist::redshift_histogram(ctx->stream, c);
    if (e != hipSuccess) return hip_fail("yawhip_redshift_histogram", e);
    return YAWHIP_OK;
}

int yawhip_healpix_map(yawhip_ctx *ctx, int64_t n, int64_t chunksize, const double *phi, const double *z, const double *w, int32_t order,
                       int32_t nested, int64_t *pix_out, double *map_out) {
    if (!ctx) return fail(YAWHIP_ERR_INVALID, "yawhip_healpix_map: ctx is NULL");
    if (!pix_out && !map_out) return fail(YAWHIP_ERR_INVALID, "yawhip_healpix_map: pix_out and map_out are both NULL");
    if (n < 0 || chunksize < 0 || (n > 0 && (!phi || !z)))
        return fail(YAWHIP_ERR_INVALID, "yawhip_healpix_map: n < 0, chunksize < 0 or NULL phi / z");
    if (const int rc = check_healpix_order("yawhip_healpix_map", order)) return rc;
    if (const int rc = check_healpix_nested("yawhip_healpix_map", nested)) return rc;
    if (n == 0) {
        if (map_out) std::fill(map_out, map_out + ((size_t)12 << (2 * order)), 0.0);
        return YAWHIP_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    yawpix::MapCall c;
    c.n = n, c.chunksize = healpix_chunk(chunksize);
    c.phi = phi, c.z = z, c.w = w;
    c.order = order, c.nested = nested;
    c.pix_out = pix_out, c.map_out = map_out;
    const hipError_t e = yawpix::healpix_map(ctx->pix_ws, ctx->stream, c);
    if (ctx->pix_ws.bytes() > ((size_t)1 << 28)) ctx->pix_ws.release();  // keep only small workspaces, as the sort workspace
    if (e != hipSuccess) return hip_fail("yawhip_healpix_map", e);
    return YAWHIP_OK;
}

int yawhip_healpix_pixels(yawhip_ctx *ctx, int64_t n_pix, int64_t chunksize, const double *values, const double *weights, int32_t order,
                          int32_t nested, int64_t capacity, int64_t *ipix_out, double *phi_out, double *z_out, double *kappa_out,
                          double *w_out, int64_t *n_selected) {
    static const char fn[] = "yawhip_healpix_pixels";
    if (!ctx) return fail(YAWHIP_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!values || !n_selected) return fail(YAWHIP_ERR_INVALID, "%s: NULL values or n_selected", fn);
    *n_selected = 0;
    if (const int rc = check_healpix_order(fn, order)) return rc;
    if (n_pix != (int64_t)12 << (2 * order))
        return fail(YAWHIP_ERR_INVALID, "%s: n_pix %lld is not 12 * 4^order (order %d)", fn, (long long)n_pix, order);
    if (const int rc = check_healpix_nested(fn, nested)) return rc;
    if (chunksize < 0 || capacity < 0) return fail(YAWHIP_ERR_INVALID, "%s: chunksize < 0 or capacity < 0", fn);
    if (capacity > 0 && (!ipix_out || !phi_out || !z_out || !kappa_out || (weights && !w_out)))
        return fail(YAWHIP_ERR_INVALID, "%s: NULL output with capacity %lld", fn, (long long)capacity);
    HIP_TRY(hipSetDevice(ctx->device));
    yawpix::PixelsCall c;
    c.chunksize = healpix_chunk(chunksize);
    c.values = values, c.weights = weights;
    c.order = order, c.nested = nested;
    c.capacity = capacity;
    c.ipix_out = ipix_out, c.phi_out = phi_out, c.z_out = z_out, c.kappa_out = kappa_out, c.w_out = w_out;
    int64_t selected = 0;
    bool overflow = false;
    const hipError_t e = yawpix::healpix_pixels(ctx->pix_ws, ctx->stream, c, selected, overflow);
    if (ctx->pix_ws.bytes() > ((size_t)1 << 28)) ctx->pix_ws.release();  // keep only small workspaces, as yawhip_healpix_map
    if (e != hipSuccess) return hip_fail(fn, e);
    *n_selected = selected;
    if (overflow)
        return fail(YAWHIP_ERR_MISMATCH, "%s: the map selects more pixels than the capacity %lld of the outputs", fn, (long long)capacity);
    if (selected != capacity)
        return fail(YAWHIP_ERR_MISMATCH, "%s: the map selects %lld pixels, the outputs were sized for %lld", fn, (long long)selected,
                    (long long)capacity);
    return YAWHIP_OK;
}

// What yawhip_random_box and yawhip_random_healpix check alike (`fn`: the name in the message); YAWHIP_OK or the failure.
static int check_random_args(const char *fn, const yawhip_ctx *ctx, int64_t n, int64_t chunksize, const uint64_t state[4], int64_t n_data,
                             const double *data_w, const double *data_z, const double *x_out, const double *y_out, const double *w_out,
                             const double *z_out, const int64_t *idx_out, const uint64_t state_out[2], const int32_t *has_uint32_out,
                             const uint32_t *uinteger_out) {
    if (!ctx || !state || !state_out || !has_uint32_out || !uinteger_out) return fail(YAWHIP_ERR_INVALID, "%s: NULL argument", fn);
    if (n < 0 || chunksize < 1) return fail(YAWHIP_ERR_INVALID, "%s: n < 0 or chunksize < 1", fn);
    if (n_data > (int64_t)1 << 32)
        return fail(YAWHIP_ERR_INVALID, "%s: n_data = %lld > 2^32: numpy draws these indices from its 64-bit bounded "
                    "path, which the device does not implement", fn, (long long)n_data);
    if (n_data == 0 || n_data < -1) return fail(YAWHIP_ERR_INVALID, "%s: n_data must be -1 or 1 .. 2^32", fn);
    if (n_data == -1 && (data_w || data_z || idx_out))
        return fail(YAWHIP_ERR_INVALID, "%s: data arrays or indices without attached data (n_data = -1)", fn);
    if (!data_w != !w_out || !data_z != !z_out)
        return fail(YAWHIP_ERR_INVALID, "%s: w_out / z_out must be given exactly with data_w / data_z", fn);
    if (n > 0 && (!x_out || !y_out)) return fail(YAWHIP_ERR_INVALID, "%s: x_out / y_out is NULL", fn);
    if ((state[3] & 1) == 0) return fail(YAWHIP_ERR_INVALID, "%s: the increment of a PCG64 state is odd", fn);
    return YAWHIP_OK;
}

static void fill_draw(yawrand::Draw &d, int64_t n, int64_t chunksize, const uint64_t state[4], int32_t has_uint32, uint32_t uinteger,
                      int64_t n_data, const double *data_w, const double *data_z, double *x_out, double *y_out, double *w_out,
                      double *z_out, int64_t *idx_out) {
    d.n = n;
    d.chunksize = chunksize;
    d.state_hi = state[0], d.state_lo = state[1], d.inc_hi = state[2], d.inc_lo = state[3];
    d.has_uint32 = has_uint32, d.uinteger = uinteger;
    d.n_data = n_data, d.data_w = data_w, d.data_z = data_z;
    d.x_out = x_out, d.y_out = y_out, d.w_out = w_out, d.z_out = z_out, d.idx_out = idx_out;
}

static int finish_draw(const char *fn, hipError_t e, const yawrand::DrawEnd &end, uint64_t state_out[2], int32_t *has_uint32_out,
                       uint32_t *uinteger_out) {
    if (e != hipSuccess) return hip_fail(fn, e);
    state_out[0] = end.state_hi;
    state_out[1] = end.state_lo;
    *has_uint32_out = end.has_uint32;
    *uinteger_out = end.uinteger;
    return YAWHIP_OK;
}

int yawhip_random_box(yawhip_ctx *ctx, int64_t n, int64_t chunksize, const uint64_t state[4], int32_t has_uint32, uint32_t uinteger,
                      double x_min, double x_range, double y_min, double y_range, int64_t n_data, const double *data_w,
                      const double *data_z, double *x_out, double *y_out, double *w_out, double *z_out, int64_t *idx_out,
                      uint64_t state_out[2], int32_t *has_uint32_out, uint32_t *uinteger_out) {
    static const char fn[] = "yawhip_random_box";
    if (const int rc = check_random_args(fn, ctx, n, chunksize, state, n_data, data_w, data_z, x_out, y_out, w_out, z_out, idx_out,
                                         state_out, has_uint32_out, uinteger_out))
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    yawrand::BoxDraw d;
    fill_draw(d, n, chunksize, state, has_uint32, uinteger, n_data, data_w, data_z, x_out, y_out, w_out, z_out, idx_out);
    d.x_min = x_min, d.x_range = x_range, d.y_min = y_min, d.y_range = y_range;
    yawrand::DrawEnd end;
    return finish_draw(fn, yawrand::draw_box(ctx->stream, d, end), end, state_out, has_uint32_out, uinteger_out);
}

int yawhip_random_healpix(yawhip_ctx *ctx, int64_t n, int64_t chunksize, const uint64_t state[4], int32_t has_uint32,
                          uint32_t uinteger, int32_t order, int64_t n_unmasked, const int64_t *ipix_unmasked, const double *cdf,
                          int64_t n_data, const double *data_w, const double *data_z, double *x_out, double *y_out, double *w_out,
                          double *z_out, int64_t *idx_out, int64_t *pix_out, uint64_t state_out[2], int32_t *has_uint32_out,
                          uint32_t *uinteger_out) {
    static const char fn[] = "yawhip_random_healpix";
    if (const int rc = check_random_args(fn, ctx, n, chunksize, state, n_data, data_w, data_z, x_out, y_out, w_out, z_out, idx_out,
                                         state_out, has_uint32_out, uinteger_out))
        return rc;
    if (const int rc = check_healpix_order(fn, order)) return rc;
    const int64_t npix = (int64_t)12 << (2 * order);
    if (n_unmasked < 1 || n_unmasked > npix || !ipix_unmasked || !cdf)
        return fail(YAWHIP_ERR_INVALID, "%s: n_unmasked outside 1 .. 12 * 4^order, or ipix_unmasked / cdf is NULL", fn);
    for (int64_t j = 0; j < n_unmasked; ++j) {
        if (ipix_unmasked[j] < 0 || ipix_unmasked[j] >= npix)
            return fail(YAWHIP_ERR_INVALID, "%s: ipix_unmasked[%lld] is no pixel of order %d", fn, (long long)j, order);
        if (!(cdf[j] >= (j ? cdf[j - 1] : 0.0)))
            return fail(YAWHIP_ERR_INVALID, "%s: cdf[%lld] is negative, NaN or below its predecessor", fn, (long long)j);
    }
    if (cdf[n_unmasked - 1] != 1.0) return fail(YAWHIP_ERR_INVALID, "%s: the cdf must end in 1", fn);
    HIP_TRY(hipSetDevice(ctx->device));
    yawrand::HealpixDraw d;
    fill_draw(d, n, chunksize, state, has_uint32, uinteger, n_data, data_w, data_z, x_out, y_out, w_out, z_out, idx_out);
    d.order = order, d.n_unmasked = n_unmasked, d.ipix_unmasked = ipix_unmasked, d.cdf = cdf, d.pix_out = pix_out;
    yawrand::DrawEnd end;
    return finish_draw(fn, yawrand::draw_healpix(ctx->stream, d, end), end, state_out, has_uint32_out, uinteger_out);
}

int yawhip_host_group_columns(int64_t n, const void *keys, int32_t key_bytes, int64_t num_groups, int32_t n_cols,
                              const double *const *in, double *const *out, int64_t *sizes, int32_t n_threads) {
    if (n < 0 || num_groups <= 0 || n_cols < 0 || !sizes || (n > 0 && !keys) || (key_bytes != 4 && key_bytes != 8))
        return fail(YAWHIP_ERR_INVALID, "yawhip_host_group_columns: bad sizes or NULL arrays");
    for (int32_t c = 0; c < n_cols; ++c)
        if (n > 0 && (!in || !out || !in[c] || !out[c] || in[c] == out[c]))
            return fail(YAWHIP_ERR_INVALID, "yawhip_host_group_columns: column %d is NULL or aliases its output", c);
    if (n_threads <= 0) n_threads = (int32_t)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    try {
        return key_bytes == 4 ? group_columns(n, (const int32_t *)keys, num_groups, n_cols, in, out, sizes, n_threads)
                              : group_columns(n, (const int64_t *)keys, num_groups, n_cols, in, out, sizes, n_threads);
    } catch (const std::bad_alloc &) {
        return fail(YAWHIP_ERR_OOM, "yawhip_host_group_columns: out of host memory");
    } catch (const std::system_error &err) {
        return fail(YAWHIP_ERR_INVALID, "yawhip_host_group_columns: %s", err.what());
    }
}

int yawhip_host_scatter_rows(int64_t n_rows, int64_t row_len, double *out, int64_t n_cols, const int64_t *cols,
                             const double *vals, int64_t val_row_stride, int64_t val_col_stride, const double *col_factor) {
    if (n_rows < 0 || row_len < 0 || n_cols < 0 || (n_rows * row_len > 0 && !out) || (n_cols > 0 && (!cols || (n_rows > 0 && !vals))))
        return fail(YAWHIP_ERR_INVALID, "yawhip_host_scatter_rows: bad sizes or NULL arrays");
    for (int64_t j = 0; j < n_cols; ++j)
        if (cols[j] < 0 || cols[j] >= row_len) return fail(YAWHIP_ERR_INVALID, "yawhip_host_scatter_rows: column %lld out of range", (long long)cols[j]);
    memset(out, 0, sizeof(double) * (size_t)(n_rows * row_len));
    for (int64_t r = 0; r < n_rows; ++r) {
        double *dst = out + r * row_len;
        const double *src = vals + r * val_row_stride;
        if (col_factor)
            for (int64_t j = 0; j < n_cols; ++j) dst[cols[j]] = src[j * val_col_stride] * col_factor[j];
        else
            for (int64_t j = 0; j < n_cols; ++j) dst[cols[j]] = src[j * val_col_stride];
    }
    return YAWHIP_OK;
}

}  // extern "C"
