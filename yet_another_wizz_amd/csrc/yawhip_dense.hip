// yawhip_dense.hip -- the dense epilogue on top of the count call of yawhip_count.hip (count_enqueue / count_finish / run_single):
// yawhip_count_pairs_dense and yawhip_count_pairs_dense_batch recombine the fine bins of every scale (k_combine_scales, or
// numpy_sum on the host) and scatter the jobs into [scale][bin][patch i][patch j]; yawhip_count_pairs_rows_device leaves the
// rows of a sharded count on the device (k_scatter_rows). The two kernels are launched only from here.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <vector>

#include "yawhip_internal.h"

using namespace yawhip_detail;

namespace {

// ndarray.sum() of values v(0) .. v(n - 1), in numpy's order (see numpy_sum on the host side of yawhip_count_pairs_dense)
template <typename F>
__device__ double numpy_sum_dev(F v, int lo, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += v(lo + i);
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = v(lo + j);
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += v(lo + i + j);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += v(lo + i);
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_sum_dev(v, lo, n2) + numpy_sum_dev(v, lo + n2, n - n2);
}

// Per-scale recombination of the fine bins on the device (yawhip_count_pairs_dense): out[job][bin][scale] = sum over the
// scale's fine bins of count (or weighted sum) x separation weight -- the same products and the same order of additions as
// the host epilogue; what crosses PCIe afterwards is S values per (job, bin) instead of E - 1.
__global__ void k_combine_scales(const unsigned long long *__restrict__ counts, const double *__restrict__ sums, int weighted,
                                 int64_t n_jobs, int n_bins, int nf, int n_scales, const int32_t *__restrict__ slices,
                                 const double *__restrict__ factors, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_jobs * n_bins * n_scales) return;
    const int sc = (int)(i % n_scales), k = (int)((i / n_scales) % n_bins);
    const int64_t j = i / ((int64_t)n_scales * n_bins);
    const int lo = slices[2 * (k * n_scales + sc)], hi = slices[2 * (k * n_scales + sc) + 1];
    const int64_t base = (j * n_bins + k) * (int64_t)nf;
    const double *wk = factors ? factors + (int64_t)k * nf : nullptr;
    auto value = [&](int e) {
        const double v = weighted ? sums[base + e] : (double)counts[base + e];
        return wk ? v * wk[e] : v;
    };
    out[i] = hi > lo ? numpy_sum_dev(value, lo, hi - lo) : 0.0;
}

// rows of a call's result into their place in the full [rows][row] tensor (device-resident all-reduce of the process route)
__global__ void k_scatter_rows(const double *__restrict__ in, const int32_t *__restrict__ row_index, int64_t row, int64_t n,
                               double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / row;
    out[(int64_t)row_index[r] * row + (i - r * row)] = in[i];
}

// ndarray.sum() of a contiguous float64 vector, in numpy's order (pairwise summation: plain loop below 8 values, eight
// running sums up to 128, halves above): the reference sums the fine bins of a scale this way (trees.py:134-160), so
// separation-weighted counts of unweighted catalogues come out bit for bit as the reference's.
double numpy_sum(const double *a, int64_t n) {
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_sum(a, n2) + numpy_sum(a + n2, n - n2);
}

struct DenseState {
    CallState cs;
    bool enqueued = false;        // on the stream (false: counted by the blocking route at finish time)
    bool device_combine = false;  // the per-scale values were recombined on the device (k_combine_scales)
    bool weighted = false;
    int slot = 0;
    int64_t n_comb = 0;
    size_t h_comb_off = 0;
};

// the count a request asks for
CountArgs request_args(const yawhip_dense_request &r, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel) {
    return CountArgs{r.c1, r.c2, r.n_jobs, r.jobs, n_bins, n_edges, t, kernel};
}

int dense_check(const yawhip_ctx *ctx, const yawhip_dense_request &r, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                int32_t n_scales, const int32_t *slices) {
    const int rc = check_call(ctx, request_args(r, n_bins, n_edges, t, kernel));
    if (rc != YAWHIP_OK) return rc;
    if (n_scales <= 0 || !slices || !r.dense) return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_dense: bad sizes or NULL arrays");
    return YAWHIP_OK;
}

// Put one request on the context's stream, in the ACTIVE slot: the count, the recombination of several fine bins on the
// device (one device, E - 1 > 1: S values per (job, bin) come back instead of E - 1 -- separation weights: 51 -> 1), the copies
// into the slot's pinned buffers, and the slot's ev_done behind all of it. Nothing waits.
int dense_enqueue(yawhip_ctx *ctx, const yawhip_dense_request &r, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                  int32_t n_scales, const int32_t *slices, const double *fine_factors, DenseState &ds) {
    const int nf = n_edges - 1;
    ds.weighted = r.c1->w != nullptr || r.c2->w != nullptr;
    ds.slot = ctx->slot;
    ds.device_combine = nf > 1;
    int rc = count_enqueue(ctx, request_args(r, n_bins, n_edges, t, kernel), !ds.weighted, ds.weighted, nullptr, ds.cs,
                           /*fetch_results=*/!ds.device_combine);
    if (rc == SPLIT_JOBS) return YAWHIP_OK;  // counted in pieces by the blocking route when its turn comes (ds.enqueued stays false)
    if (rc != YAWHIP_OK) return rc;
    if (ds.device_combine) {
        ds.cs.word_wait = false;  // the recombination and its copy follow the tail: ev_done, recorded behind them, ends the wait
        ds.n_comb = (int64_t)r.n_jobs * n_bins * n_scales;
        const size_t b_slices = align16(sizeof(int32_t) * 2 * (size_t)n_bins * n_scales);
        const size_t b_fact = fine_factors ? align16(sizeof(double) * (size_t)n_bins * nf) : 0;
        HIP_TRY(ctx->comb.reserve(b_slices + b_fact + sizeof(double) * (size_t)std::max<int64_t>(ds.n_comb, 1)));
        memcpy(ctx->comb.h, slices, sizeof(int32_t) * 2 * (size_t)n_bins * n_scales);
        if (fine_factors) memcpy(ctx->comb.h + b_slices, fine_factors, sizeof(double) * (size_t)n_bins * nf);
        HIP_TRY(hipMemcpyAsync(ctx->comb.d, ctx->comb.h, b_slices + b_fact, hipMemcpyHostToDevice, ctx->stream));
        ds.h_comb_off = b_slices + b_fact;
        unsigned char *const comb_d = ctx->comb.d;
        double *d_comb = reinterpret_cast<double *>(comb_d + ds.h_comb_off);
        if (ds.cs.pending && ds.n_comb > 0) {
            hipLaunchKernelGGL(k_combine_scales, dim3((unsigned)((ds.n_comb + 255) / 256)), dim3(256), 0, ctx->stream,
                               ctx->d_counts, ctx->d_sums, ds.weighted ? 1 : 0, (int64_t)r.n_jobs, n_bins, nf, n_scales,
                               reinterpret_cast<const int32_t *>(comb_d),
                               fine_factors ? reinterpret_cast<const double *>(comb_d + b_slices) : nullptr, d_comb);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ctx->comb.h + ds.h_comb_off, d_comb, sizeof(double) * (size_t)ds.n_comb, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    HIP_TRY(hipEventRecord(ctx->ev_done, ctx->stream));
    ds.enqueued = true;
    return YAWHIP_OK;
}

// A request's result tensor cleared: unlinked slots and empty scales stay 0 (done while the device counts wherever the route
// allows: 1 MB, 0.04 ms at the headline).
void dense_clear(const yawhip_dense_request &r, int32_t n_bins, int32_t n_scales) {
    const size_t P = (size_t)r.c1->n_patches;
    memset(r.dense, 0, sizeof(double) * (size_t)n_scales * (size_t)n_bins * P * P);
}

// The host epilogue, O(jobs x B x S), of PatchLinkage.count_pairs (reference src/yaw/correlation/measurements.py:354-364), into
// the cleared tensor: halving of the doubly counted diagonal of an autocorrelation and the scatter into
// [scale][bin][patch i][patch j]. The values of every route:
//   comb != nullptr: [job][bin][scale], the per-scale sums of the fine bins (k_combine_scales, or the host's numpy_sum);
//   else one fine bin per (job, bin): numpy's sum of one element is the element, times its separation weight -- hs
//   (weighted), or hc: unweighted catalogues are counted in int64 and converted here (exact below 2^53, the reference's
//   .astype(float64), trees.py:353).
void dense_scatter(const yawhip_dense_request &r, int32_t n_bins, int32_t n_scales, const int32_t *slices, const double *fine_factors,
                   const double *comb, bool weighted, const int64_t *hc, const double *hs) {
    const int64_t P = r.c1->n_patches;
    const int32_t n_jobs = r.n_jobs;
    const int32_t *jobs = r.jobs;
    // position and factor of every job, once per call (two short loops over the job list: well under a microsecond)
    thread_local std::vector<int64_t> cell;
    thread_local std::vector<double> half;
    cell.resize((size_t)n_jobs);
    half.resize((size_t)n_jobs);
    for (int64_t j = 0; j < n_jobs; ++j) {
        cell[(size_t)j] = (int64_t)jobs[2 * j] * P + jobs[2 * j + 1];
        half[(size_t)j] = (r.halve_diagonal && jobs[2 * j] == jobs[2 * j + 1]) ? 0.5 : 1.0;
    }
    // Two passes. The first reads the values front to back, once -- slice by slice, a walk with a stride of one job's values
    // touched every line of the 110 KB block once per slice, 30 times in all: 0.65 us a slice at the headline, the first no more
    // than the others, 21 us against 10 -- and lays them out as rows [row][job] with their factors
    // applied, in the order of products the slices always had: (value x separation weight) x half. The second scatters slice by slice from a contiguous row: the stores of a (scale, bin) land in one [P, P] slice
    // (32 KB at the headline). (Job by job, every store of a job went to another slice, P * P * 8 bytes apart: one cache set for
    // all of them, 46 us at the headline.)
    // rows: [bin][scale] of comb, else [bin] -- one fine bin per (job, bin) is the value of every scale that takes it
    const size_t PP = (size_t)(P * P), nj = (size_t)n_jobs, n_rows = comb ? (size_t)n_bins * n_scales : (size_t)n_bins;
    thread_local std::vector<double> rows;
    rows.resize(n_rows * nj);
    double *const rw = rows.data();
    g_trace.mark("cells");
    auto gather = [&](auto value) {
        for (size_t j = 0; j < nj; ++j) {
            const double hj = half[j];
            for (size_t q = 0; q < n_rows; ++q) rw[q * nj + j] = value(j * n_rows + q, q) * hj;
        }
    };
    if (comb) {
        gather([=](size_t at, size_t) { return comb[at]; });
    } else if (weighted) {
        if (fine_factors) gather([=](size_t at, size_t k) { return hs[at] * fine_factors[k]; });
        else gather([=](size_t at, size_t) { return hs[at]; });
    } else {
        if (fine_factors) gather([=](size_t at, size_t k) { return (double)hc[at] * fine_factors[k]; });
        else gather([=](size_t at, size_t) { return (double)hc[at]; });
    }
    g_trace.mark("rows");
    for (int s_ = 0; s_ < n_scales; ++s_)
        for (int k = 0; k < n_bins; ++k) {
            if (!(slices[2 * ((int64_t)k * n_scales + s_) + 1] > slices[2 * ((int64_t)k * n_scales + s_)])) continue;  // (cleared)
            double *dst = r.dense + ((size_t)s_ * n_bins + (size_t)k) * PP;
            const double *row = rw + (comb ? (size_t)k * n_scales + s_ : (size_t)k) * nj;
            for (size_t j = 0; j < nj; ++j) dst[cell[j]] = row[j];
        }
    g_trace.mark("scattered");
    g_trace.flush();
}

// The blocking route of one request: several devices in the context (the library splits the job list), or a job list that
// has to be counted in pieces (weighted slabs beyond the budget). Per-job fine values on the host, then the epilogue.
int dense_blocking(yawhip_ctx *ctx, const yawhip_dense_request &r, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                   int32_t n_scales, const int32_t *slices, const double *fine_factors) {
    const yawhip_catalog *c1 = r.c1, *c2 = r.c2;
    const int32_t n_jobs = r.n_jobs;
    const int32_t *jobs = r.jobs;
    const int nf = n_edges - 1;
    const int64_t row = (int64_t)n_bins * nf;
    const bool weighted = c1->w != nullptr || c2->w != nullptr;
    // unweighted catalogues are counted in int64 and converted on the host: one kernel and half the device-to-host bytes less
    // than asking the device for both
    const size_t n_fine = (size_t)std::max<int64_t>((int64_t)n_jobs * row, 1);
    std::unique_ptr<double[]> fine_s(weighted ? new (std::nothrow) double[n_fine] : nullptr);
    std::unique_ptr<int64_t[]> fine_c(weighted ? nullptr : new (std::nothrow) int64_t[n_fine]);
    if (!fine_s && !fine_c) return fail(YAWHIP_ERR_OOM, "yawhip_count_pairs_dense: out of host memory");
    bool cleared = false;  // (on one device the tensor is cleared while the device counts)
    const std::function<void()> clear = [&]() {
        dense_clear(r, n_bins, n_scales);
        cleared = true;
    };
    const int rc = ctx->peers.empty() ? run_single(ctx, request_args(r, n_bins, n_edges, t, kernel), fine_c.get(), fine_s.get(), r.stats, &clear)
                                      : yawhip_count_pairs(ctx, c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel, fine_c.get(), fine_s.get(), r.stats);
    if (rc != YAWHIP_OK) return rc;
    g_trace.mark("finished");
    if (!cleared) clear();
    // Several fine bins: separation weights and the per-scale sums of the fine bins per job (reference
    // src/yaw/catalog/trees.py:358-362,134-160), into the [job][bin][scale] layout of k_combine_scales, with its products
    // (counts *= weights) and its order of additions
    std::vector<double> comb;
    if (nf > 1) {
        comb.resize((size_t)n_jobs * n_bins * n_scales);
        std::vector<double> scaled((size_t)nf);
        for (int64_t j = 0; j < n_jobs; ++j)
            for (int k = 0; k < n_bins; ++k) {
                const size_t at = ((size_t)j * n_bins + k) * nf;
                const double *wk = fine_factors ? fine_factors + (size_t)k * nf : nullptr;
                for (int e = 0; e < nf; ++e) {
                    const double v = weighted ? fine_s[at + e] : (double)fine_c[at + e];
                    scaled[(size_t)e] = wk ? v * wk[e] : v;
                }
                for (int s_ = 0; s_ < n_scales; ++s_) {
                    const int lo = slices[2 * ((int64_t)k * n_scales + s_)], hi = slices[2 * ((int64_t)k * n_scales + s_) + 1];
                    comb[((size_t)j * n_bins + k) * n_scales + s_] = hi > lo ? numpy_sum(scaled.data() + lo, hi - lo) : 0.0;
                }
            }
    }
    dense_scatter(r, n_bins, n_scales, slices, fine_factors, nf > 1 ? comb.data() : nullptr, weighted, fine_c.get(), fine_s.get());
    return YAWHIP_OK;
}

// Wait for a request's slot and write its result tensor (dense_scatter) from the slot's pinned buffers.
int dense_finish(yawhip_ctx *ctx, const yawhip_dense_request &r, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                 int32_t n_scales, const int32_t *slices, const double *fine_factors, DenseState &ds) {
    if (!ds.enqueued) return dense_blocking(ctx, r, n_bins, n_edges, t, kernel, n_scales, slices, fine_factors);
    dense_clear(r, n_bins, n_scales);
    const int rc = count_finish(ctx, ds.cs, nullptr, nullptr, r.stats, nullptr, 0, /*wait_done=*/true);
    if (rc != YAWHIP_OK) return rc;
    if (!ds.cs.pending) return YAWHIP_OK;
    dense_scatter(r, n_bins, n_scales, slices, fine_factors,
                  ds.device_combine ? reinterpret_cast<const double *>(ctx->comb.h + ds.h_comb_off) : nullptr, ds.weighted,
                  reinterpret_cast<const int64_t *>(ctx->out.h + ds.cs.o_counts), reinterpret_cast<const double *>(ctx->out.h + ds.cs.o_sums));
    return YAWHIP_OK;
}

}  // namespace

extern "C" {

int yawhip_count_pairs_rows_device(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                                   const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                                   int64_t n_rows_total, const int32_t *row_index, double **device_rows, yawhip_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!ctx || !c1 || !c2 || !device_rows) return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_rows_device: NULL argument");
    *device_rows = nullptr;
    if (!ctx->peers.empty()) return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_rows_device: single-device contexts only");
    const CountArgs args{c1, c2, n_jobs, jobs, n_bins, n_edges, t, kernel};
    const int rc_args = check_call(ctx, args);
    if (rc_args != YAWHIP_OK) return rc_args;
    if (n_rows_total < n_jobs || (n_jobs > 0 && !row_index))
        return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_rows_device: bad sizes or NULL arrays");
    const int64_t row = (int64_t)n_bins * (n_edges - 1);
    for (int j = 0; j < n_jobs; ++j)
        if (row_index[j] < 0 || row_index[j] >= n_rows_total)
            return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_rows_device: row index %d outside [0, %lld)", row_index[j], (long long)n_rows_total);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t n_full = (size_t)n_rows_total * (size_t)row + 1;  // + 1: the caller's status element
    HIP_TRY(reserve_call(ctx->d_full, n_full));
    HIP_TRY(reserve_call(ctx->d_rowidx, (size_t)std::max(n_jobs, 1)));
    CallState cs;
    // (the rows stay on the device: only the statistics counters are fetched)
    int rc = count_enqueue(ctx, args, false, true, nullptr, cs, /*fetch_results=*/false);
    if (rc == SPLIT_JOBS) {
        // a job list that is counted in pieces: through the host (rare: weighted slabs beyond the budget)
        std::vector<double> rows((size_t)n_jobs * (size_t)row), full(n_full, 0.0);
        rc = run_single(ctx, args, nullptr, rows.data(), stats);
        if (rc != YAWHIP_OK) return rc;
        place_rows(full.data(), (const double *)rows.data(), n_jobs, row, row_index);
        HIP_TRY(hipMemcpy(ctx->d_full.ptr, full.data(), sizeof(double) * n_full, hipMemcpyHostToDevice));
        *device_rows = ctx->d_full.ptr;
        return YAWHIP_OK;
    }
    if (rc != YAWHIP_OK) return rc;
    cs.word_wait = false;  // the rows are scattered behind the tail: the stream ends the wait
    HIP_TRY(hipMemsetAsync(ctx->d_full.ptr, 0, sizeof(double) * n_full, ctx->stream));
    if (cs.pending && n_jobs > 0) {
        HIP_TRY(hipMemcpyAsync(ctx->d_rowidx.ptr, row_index, sizeof(int32_t) * (size_t)n_jobs, hipMemcpyHostToDevice, ctx->stream));
        const int64_t n = (int64_t)n_jobs * row;
        hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_sums,
                           ctx->d_rowidx.ptr, row, n, ctx->d_full.ptr);
        HIP_TRY(hipGetLastError());
    }
    rc = count_finish(ctx, cs, nullptr, nullptr, stats);  // waits for the stream: the rows are in place when this returns
    if (rc != YAWHIP_OK) return rc;
    *device_rows = ctx->d_full.ptr;
    return YAWHIP_OK;
}

int yawhip_count_pairs_dense(yawhip_ctx *ctx, const yawhip_catalog *c1, const yawhip_catalog *c2, int32_t n_jobs,
                             const int32_t *jobs, int32_t n_bins, int32_t n_edges, const double *t, int32_t kernel,
                             int32_t n_scales, const int32_t *slices, const double *fine_factors, int32_t halve_diagonal,
                             double *dense, yawhip_stats *stats) {
    yawhip_dense_request req{c1, c2, n_jobs, halve_diagonal, jobs, dense, stats};
    return yawhip_count_pairs_dense_batch(ctx, 1, &req, n_bins, n_edges, t, kernel, n_scales, slices, fine_factors);
}

int yawhip_count_pairs_dense_batch(yawhip_ctx *ctx, int32_t n_requests, const yawhip_dense_request *requests, int32_t n_bins,
                                   int32_t n_edges, const double *t, int32_t kernel, int32_t n_scales, const int32_t *slices,
                                   const double *fine_factors) {
    if (!ctx || n_requests < 0 || (n_requests > 0 && !requests))
        return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_dense_batch: NULL argument");
    for (int i = 0; i < n_requests; ++i) {
        if (requests[i].stats) memset(requests[i].stats, 0, sizeof(yawhip_stats));
        const int rc = dense_check(ctx, requests[i], n_bins, n_edges, t, kernel, n_scales, slices);
        if (rc != YAWHIP_OK) return rc;
    }
    const int nf = n_edges - 1;
    if (n_bins > 0 && n_scales > 0 && slices)
        for (int64_t i = 0; i < (int64_t)n_bins * n_scales; ++i)
            if (slices[2 * i] < 0 || slices[2 * i + 1] > nf)
                return fail(YAWHIP_ERR_INVALID, "yawhip_count_pairs_dense: slice %lld outside [0, %d]", (long long)i, nf);
    if (n_requests == 0) return YAWHIP_OK;
    if (!ctx->peers.empty()) {  // several devices: every request is split over them by yawhip_count_pairs, one after the other
        for (int i = 0; i < n_requests; ++i) {
            const int rc = dense_blocking(ctx, requests[i], n_bins, n_edges, t, kernel, n_scales, slices, fine_factors);
            if (rc != YAWHIP_OK) return rc;
        }
        return YAWHIP_OK;
    }
    // One device: up to MAX_BATCH requests are on the stream at once, each in a slot of its own (tables, work items, partial
    // sums, result block, events). The host enqueues request k + 1 while the device counts request k, and writes the tensor of
    // request k (its epilogue) while the device counts the ones behind it; the device never waits for the host in between.
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<DenseState> st((size_t)n_requests);
    int rc_all = YAWHIP_OK, done = 0;
    auto finish_next = [&]() {
        hipError_t e = use_slot(ctx, done % MAX_BATCH);
        int rc = e == hipSuccess ? dense_finish(ctx, requests[done], n_bins, n_edges, t, kernel, n_scales, slices, fine_factors, st[(size_t)done])
                                 : fail(YAWHIP_ERR_HIP, "event creation failed: %s", hipGetErrorString(e));
        if (rc != YAWHIP_OK && rc_all == YAWHIP_OK) rc_all = rc;
        ++done;
    };
    int issued = 0;
    for (; issued < n_requests && rc_all == YAWHIP_OK; ++issued) {
        if (issued - done >= MAX_BATCH) finish_next();  // its slot is needed again
        if (rc_all != YAWHIP_OK) break;
        hipError_t e = use_slot(ctx, issued % MAX_BATCH);
        if (e != hipSuccess) { rc_all = fail(YAWHIP_ERR_HIP, "event creation failed: %s", hipGetErrorString(e)); break; }
        const int rc = dense_enqueue(ctx, requests[issued], n_bins, n_edges, t, kernel, n_scales, slices, fine_factors, st[(size_t)issued]);
        if (rc != YAWHIP_OK) { rc_all = rc; break; }
    }
    if (rc_all != YAWHIP_OK) {  // leave nothing in flight behind an error
        (void)hipStreamSynchronize(ctx->stream);
        (void)use_slot(ctx, 0);
        return rc_all;
    }
    while (done < issued) finish_next();
    (void)use_slot(ctx, 0);
    if (rc_all != YAWHIP_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc_all;
}

}  // extern "C"
