// libmcpc.so, the stateless reducers over recorded states: the entries of include/mcpc.h that take an `int device` and no engine --
// moments, covariances, histograms (1-D and joint), lagged autocovariances, rolling windows, linear probes, nearest-neighbour
// divergences, log marginal likelihoods, annealed-importance-sampling increments, Metropolis-adjusted Langevin proposals and
// decisions, resampling ancestors and their gather -- with their kernels.  A translation unit of its own: it sees nothing of the step kernels, the planner or the engine, and an edit to a reducer recompiles this unit alone.  What an entry refuses is read through
// mcpc_last_error (mcpc_api.hip) like every other error of the library: mcpc_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mcpc_host.h"
#include "mcpc_moments.h"
#include "mcpc_cov.h"
#include "mcpc_hist.h"
#include "mcpc_hist2d.h"
#include "mcpc_acov.h"
#include "mcpc_roll.h"
#include "mcpc_probe.h"
#include "mcpc_knn.h"
#include "mcpc_loglik.h"
#include "mcpc_ais.h"
#include "mcpc_mala.h"
#include "mcpc_hmc.h"
#include "mcpc_smc.h"

using namespace mcpc;

extern "C" {

namespace {
// The record window of the accumulate entries: records first, first + stride, ... (n of them) of a ring `rec` whose rows hold B x width
// floats.  The checks they share; `who`, the entry's name, opens every message.
int check_shape(const char* who, int32_t B, int32_t width) {
    if (B < 1) return fail(MCPC_EINVAL, "%s: B=%d, must be at least 1", who, B);
    if (width < 1) return fail(MCPC_EINVAL, "%s: width=%d, must be at least 1", who, width);
    return 0;
}
int check_window(const char* who, const void* rec, int32_t first, int32_t stride, int32_t n) {
    if (stride < 1) return fail(MCPC_EINVAL, "%s: stride=%d, must be at least 1", who, stride);
    if (first < 0) return fail(MCPC_EINVAL, "%s: first=%d, must not be negative", who, first);
    if (n < 0) return fail(MCPC_EINVAL, "%s: n=%d, must not be negative", who, n);
    if (n > 0 && !rec) return fail(MCPC_EINVAL, "%s: rec is null with n=%d", who, n);
    return 0;
}
int check_transform(const char* who, int32_t xf) {
    return xf != MCPC_MOM_IDENTITY && xf != MCPC_MOM_SIGMOID ? fail(MCPC_EINVAL, "%s: unknown transform %d", who, xf) : 0;
}
// The window itself: the row length E, the first record, the distance between two records.
// All offsets in 64 bits: (first + k * stride) * E passes 2^31 elements at the shapes the step kernels are built for.
struct RecWindow { int64_t E; const float* r0; int64_t row_step; };
RecWindow rec_window(const float* rec, int64_t E, int32_t first, int32_t stride, int32_t n) {
    return {E, n > 0 ? rec + (int64_t)first * E : rec, (int64_t)stride * E};
}
}  // namespace

int mcpc_moments_accumulate(int device, const float* rec, int64_t row_elems, int32_t first, int32_t stride, int32_t n, int32_t transform,
                            double* sum, double* sumsq, int accumulate, void* stream_) {
    if (!sum) return fail(MCPC_EINVAL, "moments: sum is null");
    if (row_elems < 1) return fail(MCPC_EINVAL, "moments: row_elems=%lld, must be at least 1", (long long)row_elems);
    if (const int rc = check_window("moments", rec, first, stride, n)) return rc;
    if (const int rc = check_transform("moments", transform)) return rc;
    if (n == 0 && accumulate) return MCPC_OK;                     // nothing to add
    HIP_TRY(hipSetDevice(device));
    const RecWindow w = rec_window(rec, row_elems, first, stride, n);
    const uintptr_t align = (uintptr_t)w.r0 | (uintptr_t)sum | (uintptr_t)sumsq;
    if (row_elems % 4 == 0 && align % 16 == 0)
        mom_dispatch<4>(transform, w.r0, w.E, w.row_step, n, sum, sumsq, accumulate, (hipStream_t)stream_);
    else
        mom_dispatch<1>(transform, w.r0, w.E, w.row_step, n, sum, sumsq, accumulate, (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

// shared argument checks of the two covariance entry points; fills the plan
static int cov_check_shape(int32_t B, const int32_t* widths, int32_t n_blocks, int32_t pool, CovPlan& plan) {
    if (n_blocks < 1 || n_blocks > kCovMaxBlocks) return fail(MCPC_EINVAL, "cov: n_blocks=%d outside 1..%d", n_blocks, kCovMaxBlocks);
    if (!widths) return fail(MCPC_EINVAL, "cov: widths is null");
    if (B < 1) return fail(MCPC_EINVAL, "cov: B=%d, must be at least 1", B);
    if (pool != 0 && pool != 1) return fail(MCPC_EINVAL, "cov: pool=%d, must be 0 or 1", pool);
    int64_t D = 0;
    for (int b = 0; b < n_blocks; ++b) {
        if (widths[b] < 1) return fail(MCPC_EINVAL, "cov: widths[%d]=%d, must be at least 1", b, widths[b]);
        D += (widths[b] + 15) / 16 * 16;
    }
    if (D > 32768) return fail(MCPC_EINVAL, "cov: %lld padded columns, at most 32768", (long long)D);
    plan = cov_plan(B, widths, n_blocks, pool);
    // one workgroup of 64 lanes per job, and a grid holds fewer than 2^32 threads
    if ((int64_t)plan.groups * plan.npairs >= (1LL << 26))
        return fail(MCPC_EINVAL, "cov: %lld jobs (chain groups x blocks of tile pairs), a launch holds fewer than %lld", (long long)plan.groups * plan.npairs, 1LL << 26);
    return MCPC_OK;
}

int64_t mcpc_cov_workspace_bytes(int32_t B, const int32_t* widths, int32_t n_blocks, int32_t pool) {
    CovPlan plan;
    if (cov_check_shape(B, widths, n_blocks, pool, plan)) return -1;
    return pool ? (int64_t)plan.groups * plan.Dpad * plan.Dpad * (int64_t)sizeof(double) : 0;
}

int mcpc_cov_accumulate(int device, const float* const* rec, const int32_t* widths, const int32_t* transforms, int32_t n_blocks, int32_t B,
                        int32_t first, int32_t stride, int32_t n, int32_t pool, double* outer, int accumulate, void* workspace,
                        int64_t workspace_bytes, void* stream_) {
    CovPlan plan;
    if (const int rc = cov_check_shape(B, widths, n_blocks, pool, plan)) return rc;
    if (!outer) return fail(MCPC_EINVAL, "cov: outer is null");
    if (const int rc = check_window("cov", rec, first, stride, n)) return rc;
    bool any_sig = false;
    for (int b = 0; b < n_blocks; ++b) {
        const int32_t xf = transforms ? transforms[b] : MCPC_MOM_IDENTITY;
        if (xf != MCPC_MOM_IDENTITY && xf != MCPC_MOM_SIGMOID) return fail(MCPC_EINVAL, "cov: unknown transform %d of block %d", xf, b);
        any_sig = any_sig || xf == MCPC_MOM_SIGMOID;
    }
    for (int b = 0; n > 0 && b < n_blocks; ++b)
        if (!rec[b]) return fail(MCPC_EINVAL, "cov: rec[%d] is null with n=%d", b, n);
    const int64_t need = pool ? (int64_t)plan.groups * plan.Dpad * plan.Dpad * (int64_t)sizeof(double) : 0;
    if (n > 0 && pool) {
        if (!workspace) return fail(MCPC_EINVAL, "cov: workspace is null with pool=1 (mcpc_cov_workspace_bytes: %lld bytes)", (long long)need);
        if (workspace_bytes < need)
            return fail(MCPC_EINVAL, "cov: workspace of %lld bytes is too small, %lld needed", (long long)workspace_bytes, (long long)need);
    }
    if (n == 0 && accumulate) return MCPC_OK;                     // nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(outer, 0, (size_t)(pool ? 1 : B) * plan.D * plan.D * sizeof(double), stream));
        return MCPC_OK;
    }
    CovParams P{};
    int32_t tile = 0, col = 0;
    for (int b = 0; b <= kCovMaxBlocks; ++b) {
        P.tile0[b] = tile; P.col0[b] = col;
        if (b < n_blocks) {
            P.rec[b] = rec[b]; P.width[b] = widths[b]; P.xf[b] = transforms ? transforms[b] : MCPC_MOM_IDENTITY;
            tile += (widths[b] + 15) / 16; col += widths[b];
        }
    }
    P.n_blocks = n_blocks; P.NT = plan.NT; P.NB = plan.NB; P.npairs = plan.npairs; P.D = plan.D; P.Dpad = plan.Dpad;
    P.B = B; P.first = first; P.stride = stride; P.n = n; P.gs = plan.gs; P.accumulate = accumulate ? 1 : 0;
    P.out = pool ? (double*)workspace : outer;
    const dim3 grid((unsigned)((int64_t)plan.groups * plan.npairs)), block(64);
    if (pool) {
        if (any_sig) hipLaunchKernelGGL((mcpc_cov_kernel<true, true>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((mcpc_cov_kernel<true, false>), grid, block, 0, stream, P);
        const int64_t total = (int64_t)plan.D * plan.D;
        hipLaunchKernelGGL(mcpc_cov_finish_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 2048)), dim3(256), 0, stream, P,
                           (const double*)workspace, plan.groups, outer);
    } else {
        if (any_sig) hipLaunchKernelGGL((mcpc_cov_kernel<false, true>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((mcpc_cov_kernel<false, false>), grid, block, 0, stream, P);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_hist_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n, int32_t transform,
                         const float* edges, int32_t n_bins, int32_t pool, int64_t* counts, int accumulate, void* stream_) {
    if (!counts) return fail(MCPC_EINVAL, "hist: counts is null");
    if (!edges) return fail(MCPC_EINVAL, "hist: edges is null");
    if (const int rc = check_shape("hist", B, width)) return rc;
    if (const int rc = check_window("hist", rec, first, stride, n)) return rc;
    if (n_bins < 1 || n_bins > MCPC_HIST_MAX_BINS) return fail(MCPC_EINVAL, "hist: n_bins=%d outside 1..%d", n_bins, MCPC_HIST_MAX_BINS);
    if (pool != 0 && pool != 1) return fail(MCPC_EINVAL, "hist: pool=%d, must be 0 or 1", pool);
    if (const int rc = check_transform("hist", transform)) return rc;
    for (int i = 0; i <= n_bins; ++i) {
        if (!std::isfinite(edges[i])) return fail(MCPC_EINVAL, "hist: edges[%d] is not finite", i);
        if (i > 0 && !(edges[i - 1] < edges[i]))
            return fail(MCPC_EINVAL, "hist: edges are not strictly ascending at %d (%.9g, then %.9g)", i, (double)edges[i - 1], (double)edges[i]);
    }
    if (n == 0 && accumulate) return MCPC_OK;                     // nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    const RecWindow w = rec_window(rec, (int64_t)B * width, first, stride, n);
    const int64_t E = w.E, ncol = n_bins + 3;
    const size_t out_bytes = (size_t)(pool ? (int64_t)width : E) * ncol * sizeof(int64_t);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(counts, 0, out_bytes, stream));
        return MCPC_OK;
    }
    const int kVec = (E % 4 == 0 && (uintptr_t)w.r0 % 16 == 0) ? 4 : 1;
    const HistPlan plan = hist_plan(E, width, pool, n, n_bins, kVec);
    HistParams P{};
    P.top = hist_key_table(edges, n_bins, P.key, kHistTable, &P.key_hi);
    P.n_bins = n_bins;
    P.TV = plan.TV; P.n = n; P.seg = plan.seg; P.width = width; P.pool = pool;
    P.exclusive = (!pool && plan.segments == 1) ? 1 : 0;
    P.accumulate = accumulate ? 1 : 0;
    P.E = E; P.row_step = w.row_step; P.tiles = plan.tiles; P.period = plan.period; P.splits = plan.splits;
    // workgroups that share a destination add into it with integer atomics: an overwriting call starts them from zero
    if (!P.exclusive && !accumulate) HIP_TRY(hipMemsetAsync(counts, 0, out_bytes, stream));
    if (kVec == 4) hist_launch<4>(transform, w.r0, P, plan, counts, stream);
    else hist_launch<1>(transform, w.r0, P, plan, counts, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_acov_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n, int32_t transform,
                         int32_t max_lag, int64_t n_seen, double* lagged, double* sum, float* window, float* head, void* stream_) {
    if (max_lag < 0 || max_lag > MCPC_ACOV_MAX_LAG) return fail(MCPC_EINVAL, "acov: max_lag=%d outside 0..%d", max_lag, MCPC_ACOV_MAX_LAG);
    if (!lagged) return fail(MCPC_EINVAL, "acov: lagged is null");
    if (!sum) return fail(MCPC_EINVAL, "acov: sum is null");
    if (max_lag > 0 && !window) return fail(MCPC_EINVAL, "acov: window is null with max_lag=%d", max_lag);
    if (max_lag > 0 && !head) return fail(MCPC_EINVAL, "acov: head is null with max_lag=%d", max_lag);
    if (const int rc = check_shape("acov", B, width)) return rc;
    if (const int rc = check_window("acov", rec, first, stride, n)) return rc;
    if (n_seen < 0) return fail(MCPC_EINVAL, "acov: n_seen=%lld, must not be negative", (long long)n_seen);
    if (const int rc = check_transform("acov", transform)) return rc;
    if (n == 0 && n_seen > 0) return MCPC_OK;                     // nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    const RecWindow w = rec_window(rec, (int64_t)B * width, first, stride, n);
    if (n == 0) {                                                 // a stream that starts empty
        HIP_TRY(hipMemsetAsync(lagged, 0, (size_t)w.E * (max_lag + 1) * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(sum, 0, (size_t)w.E * sizeof(double), stream));
        return MCPC_OK;
    }
    AcovParams P{};
    P.rec = w.r0; P.E = w.E; P.row_step = w.row_step; P.n_seen = n_seen; P.n = n; P.K = max_lag;
    P.lagged = lagged; P.sum = sum; P.window = window; P.head = head;
    acov_dispatch(transform, P, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

static int roll_check_shape(int32_t B, int32_t width, int32_t n) {
    if (const int rc = check_shape("roll", B, width)) return rc;
    if (n < 0) return fail(MCPC_EINVAL, "roll: n=%d, must not be negative", n);
    if (roll_groups((int64_t)B * width, 1) >= kRollMaxGroups)
        return fail(MCPC_EINVAL, "roll: B * width = %lld is more than one launch holds", (long long)B * width);
    return MCPC_OK;
}

int64_t mcpc_roll_workspace_bytes(int32_t B, int32_t width, int32_t n) {
    if (roll_check_shape(B, width, n)) return -1;
    // a chunk of n samples emits at most n rows, and the scalar form has the most workgroups
    return roll_groups((int64_t)B * width, 1) * (int64_t)n * 4 * (int64_t)sizeof(double);
}

int mcpc_roll_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n, int32_t transform,
                         int32_t window, int32_t every, int64_t n_seen, double* s1, double* s2, float* hist, double* out_elem,
                         double* out_pool, void* workspace, void* stream_) {
    if (window < 2) return fail(MCPC_EINVAL, "roll: window=%d, must be at least 2", window);
    if (every < 1) return fail(MCPC_EINVAL, "roll: every=%d, must be at least 1", every);
    if (!s1) return fail(MCPC_EINVAL, "roll: s1 is null");
    if (!s2) return fail(MCPC_EINVAL, "roll: s2 is null");
    if (!hist) return fail(MCPC_EINVAL, "roll: hist is null");
    if (!out_elem && !out_pool) return fail(MCPC_EINVAL, "roll: out_elem and out_pool are both null");
    if (const int rc = roll_check_shape(B, width, n)) return rc;
    if (const int rc = check_window("roll", rec, first, stride, n)) return rc;      // (n: checked with the shape already)
    if (n_seen < 0) return fail(MCPC_EINVAL, "roll: n_seen=%lld, must not be negative", (long long)n_seen);
    if (const int rc = check_transform("roll", transform)) return rc;
    RollParams P{};
    P.rows = roll_rows(n_seen, n, window, every, &P.emit0);
    if (out_pool && P.rows > 0 && !workspace)
        return fail(MCPC_EINVAL, "roll: workspace is null with out_pool set (mcpc_roll_workspace_bytes: %lld bytes)",
                    (long long)mcpc_roll_workspace_bytes(B, width, n));
    if (n == 0 && n_seen > 0) return MCPC_OK;                     // nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    const RecWindow w = rec_window(rec, (int64_t)B * width, first, stride, n);
    if (n == 0) {                                                 // a stream that starts empty
        HIP_TRY(hipMemsetAsync(s1, 0, (size_t)w.E * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(s2, 0, (size_t)w.E * sizeof(double), stream));
        return MCPC_OK;
    }
    P.rec = w.r0; P.E = w.E; P.row_step = w.row_step; P.n_seen = n_seen; P.n = n; P.W = window; P.every = every;
    P.slot0 = (int32_t)(n_seen % window);
    P.s1 = s1; P.s2 = s2; P.hist = hist; P.out_elem = out_elem; P.part = (double*)workspace;
    if (roll_vec(P) == 4) roll_launch<4>(transform, P, out_pool, stream);
    else roll_launch<1>(transform, P, out_pool, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_probe_accumulate(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n, const float* W,
                          const float* bias, int32_t n_classes, int32_t link, double* psum, double* psumsq, int64_t* votes, double* entsum,
                          int accumulate, void* stream_) {
    if (!W) return fail(MCPC_EINVAL, "probe: W is null");
    if (!psum) return fail(MCPC_EINVAL, "probe: psum is null");
    if (!votes) return fail(MCPC_EINVAL, "probe: votes is null");
    if (link != MCPC_PROBE_IDENTITY && link != MCPC_PROBE_SIGMOID && link != MCPC_PROBE_SOFTMAX)
        return fail(MCPC_EINVAL, "probe: unknown link %d", link);
    if (link == MCPC_PROBE_SOFTMAX && !entsum) return fail(MCPC_EINVAL, "probe: entsum is null with the softmax link");
    if (const int rc = check_shape("probe", B, width)) return rc;
    if (const int rc = check_window("probe", rec, first, stride, n)) return rc;
    if (n_classes < 1 || n_classes > MCPC_PROBE_MAX_CLASSES)
        return fail(MCPC_EINVAL, "probe: n_classes=%d outside 1..%d", n_classes, MCPC_PROBE_MAX_CLASSES);
    if (n == 0 && accumulate) return MCPC_OK;                     // nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(psum, 0, (size_t)B * n_classes * sizeof(double), stream));
        if (psumsq) HIP_TRY(hipMemsetAsync(psumsq, 0, (size_t)B * n_classes * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(votes, 0, (size_t)B * (n_classes + 1) * sizeof(int64_t), stream));
        if (link == MCPC_PROBE_SOFTMAX) HIP_TRY(hipMemsetAsync(entsum, 0, (size_t)B * sizeof(double), stream));
        return MCPC_OK;
    }
    ProbeParams P{};
    const RecWindow w = rec_window(rec, (int64_t)B * width, first, stride, n);
    P.rec = w.r0; P.W = W; P.bias = bias; P.row_step = w.row_step;
    P.B = B; P.width = width; P.n = n; P.C = n_classes; P.accumulate = accumulate ? 1 : 0;
    P.psum = psum; P.psumsq = psumsq; P.votes = votes; P.entsum = entsum;
    probe_dispatch(link, P, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_probe_records(int device, const float* rec, int32_t B, int32_t width, int32_t first, int32_t stride, int32_t n, const float* W,
                       const float* bias, int32_t n_classes, int32_t link, float* out, void* stream_) {
    if (!W) return fail(MCPC_EINVAL, "probe records: W is null");
    if (!out) return fail(MCPC_EINVAL, "probe records: out is null");
    if (link != MCPC_PROBE_IDENTITY && link != MCPC_PROBE_SIGMOID && link != MCPC_PROBE_SOFTMAX)
        return fail(MCPC_EINVAL, "probe records: unknown link %d", link);
    if (const int rc = check_shape("probe records", B, width)) return rc;
    if (const int rc = check_window("probe records", rec, first, stride, n)) return rc;
    if (n_classes < 1 || n_classes > MCPC_PROBE_MAX_CLASSES)
        return fail(MCPC_EINVAL, "probe records: n_classes=%d outside 1..%d", n_classes, MCPC_PROBE_MAX_CLASSES);
    if (n == 0) return MCPC_OK;                                   // no row to write
    HIP_TRY(hipSetDevice(device));
    ProbeParams P{};
    const RecWindow w = rec_window(rec, (int64_t)B * width, first, stride, n);
    P.rec = w.r0; P.W = W; P.bias = bias; P.row_step = w.row_step;
    P.B = B; P.width = width; P.n = n; P.C = n_classes; P.out = out;
    probe_dispatch<true>(link, P, (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_hist2d_accumulate(int device, const float* rec_x, int32_t width_x, const float* rec_y, int32_t width_y, int32_t B, int32_t first,
                           int32_t stride, int32_t n, int32_t transform_x, int32_t transform_y, const int32_t* pairs, int32_t n_pairs,
                           const float* edges_x, int32_t nx, const float* edges_y, int32_t ny, int32_t pool, int64_t* counts,
                           int accumulate, void* stream_) {
    if (!counts) return fail(MCPC_EINVAL, "hist2d: counts is null");
    if (!edges_x) return fail(MCPC_EINVAL, "hist2d: edges_x is null");
    if (!edges_y) return fail(MCPC_EINVAL, "hist2d: edges_y is null");
    if (!pairs) return fail(MCPC_EINVAL, "hist2d: pairs is null");
    if (B < 1) return fail(MCPC_EINVAL, "hist2d: B=%d, must be at least 1", B);
    if (width_x < 1) return fail(MCPC_EINVAL, "hist2d: width_x=%d, must be at least 1", width_x);
    if (width_y < 1) return fail(MCPC_EINVAL, "hist2d: width_y=%d, must be at least 1", width_y);
    if (const int rc = check_window("hist2d", rec_x, first, stride, n)) return rc;
    if (n > 0 && !rec_y) return fail(MCPC_EINVAL, "hist2d: rec_y is null with n=%d", n);
    if (n_pairs < 1 || n_pairs > MCPC_HIST2D_MAX_PAIRS)
        return fail(MCPC_EINVAL, "hist2d: n_pairs=%d outside 1..%d", n_pairs, MCPC_HIST2D_MAX_PAIRS);
    if (nx < 1 || nx > MCPC_HIST2D_MAX_BINS) return fail(MCPC_EINVAL, "hist2d: nx=%d outside 1..%d", nx, MCPC_HIST2D_MAX_BINS);
    if (ny < 1 || ny > MCPC_HIST2D_MAX_BINS) return fail(MCPC_EINVAL, "hist2d: ny=%d outside 1..%d", ny, MCPC_HIST2D_MAX_BINS);
    if ((nx + 3) * (ny + 3) > MCPC_HIST2D_MAX_CELLS)
        return fail(MCPC_EINVAL, "hist2d: (nx + 3) * (ny + 3) = %d cells, more than %d", (nx + 3) * (ny + 3), MCPC_HIST2D_MAX_CELLS);
    if (pool != 0 && pool != 1) return fail(MCPC_EINVAL, "hist2d: pool=%d, must be 0 or 1", pool);
    if (const int rc = check_transform("hist2d", transform_x)) return rc;
    if (const int rc = check_transform("hist2d", transform_y)) return rc;
    for (int i = 0; i < n_pairs; ++i) {
        if (pairs[2 * i] < 0 || pairs[2 * i] >= width_x)
            return fail(MCPC_EINVAL, "hist2d: pair %d: x column %d outside 0..%d", i, pairs[2 * i], width_x - 1);
        if (pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= width_y)
            return fail(MCPC_EINVAL, "hist2d: pair %d: y column %d outside 0..%d", i, pairs[2 * i + 1], width_y - 1);
    }
    for (int axis = 0; axis < 2; ++axis) {
        const float* edges = axis ? edges_y : edges_x;
        const char* name = axis ? "edges_y" : "edges_x";
        for (int i = 0; i <= (axis ? ny : nx); ++i) {
            if (!std::isfinite(edges[i])) return fail(MCPC_EINVAL, "hist2d: %s[%d] is not finite", name, i);
            if (i > 0 && !(edges[i - 1] < edges[i]))
                return fail(MCPC_EINVAL, "hist2d: %s are not strictly ascending at %d (%.9g, then %.9g)", name, i, (double)edges[i - 1],
                            (double)edges[i]);
        }
    }
    if (n == 0 && accumulate) return MCPC_OK;                     // nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    const Hist2dPlan plan = hist2d_plan(B, width_x, width_y, n_pairs, nx, ny, pool, n > 0 ? n : 1);
    const size_t out_bytes = (size_t)plan.slots * plan.cells * sizeof(int64_t);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(counts, 0, out_bytes, stream));
        return MCPC_OK;
    }
    const RecWindow wx = rec_window(rec_x, (int64_t)B * width_x, first, stride, n);
    const RecWindow wy = rec_window(rec_y, (int64_t)B * width_y, first, stride, n);
    Hist2dParams P{};
    P.top_x = hist_key_table(edges_x, nx, P.key_x, kHist2dTable, &P.hi_x);
    P.top_y = hist_key_table(edges_y, ny, P.key_y, kHist2dTable, &P.hi_y);
    P.nx = nx; P.ny = ny;
    for (int i = 0; i < n_pairs; ++i) { P.col[i][0] = pairs[2 * i]; P.col[i][1] = pairs[2 * i + 1]; }
    P.n_pairs = n_pairs; P.B = B; P.wx = width_x; P.wy = width_y; P.G = plan.G; P.GL = plan.GL; P.n = n; P.seg = plan.seg;
    P.chains_per = plan.chains_per; P.pool = pool;
    P.exclusive = (!pool && plan.segments == 1) ? 1 : 0;
    P.accumulate = accumulate ? 1 : 0;
    P.slots = plan.slots; P.groups = plan.groups; P.step_x = wx.row_step; P.step_y = wy.row_step;
    // workgroups that share a grid add into it with integer atomics: an overwriting call starts them from zero
    if (!P.exclusive && !accumulate) HIP_TRY(hipMemsetAsync(counts, 0, out_bytes, stream));
    hist2d_launch(transform_x, transform_y, wx.r0, wy.r0, P, plan, counts, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

static int knn_check_shape(int64_t nq, int64_t nr, int32_t d, int32_t k) {
    if (d < 1 || d > MCPC_KNN_MAX_DIM) return fail(MCPC_EINVAL, "knn: d=%d outside 1..%d", d, MCPC_KNN_MAX_DIM);
    if (k < 1 || k > MCPC_KNN_MAX_K) return fail(MCPC_EINVAL, "knn: k=%d outside 1..%d", k, MCPC_KNN_MAX_K);
    if (nq < 0 || nq > MCPC_KNN_MAX_ROWS) return fail(MCPC_EINVAL, "knn: nq=%lld outside 0..%lld", (long long)nq, (long long)MCPC_KNN_MAX_ROWS);
    if (nr < 0 || nr > MCPC_KNN_MAX_ROWS) return fail(MCPC_EINVAL, "knn: nr=%lld outside 0..%lld", (long long)nr, (long long)MCPC_KNN_MAX_ROWS);
    return MCPC_OK;
}

int64_t mcpc_knn_workspace_bytes(int64_t nq, int64_t nr, int32_t d, int32_t k) {
    if (knn_check_shape(nq, nr, d, k)) return -1;
    const KnnGeometry g = knn_geometry(nq, nr, d, k);
    return g.n_splits * nq * g.kt * (int64_t)sizeof(float);
}

int mcpc_knn_accumulate(int device, const float* q, int64_t nq, const float* ref, int64_t nr, int32_t d, int32_t k, float* best,
                        int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream_) {
    if (const int rc = knn_check_shape(nq, nr, d, k)) return rc;
    if (nq > 0 && !q) return fail(MCPC_EINVAL, "knn: q is null with nq=%lld", (long long)nq);
    if (nq > 0 && !best) return fail(MCPC_EINVAL, "knn: best is null with nq=%lld", (long long)nq);
    if (nr > 0 && !ref) return fail(MCPC_EINVAL, "knn: ref is null with nr=%lld", (long long)nr);
    const KnnGeometry g = knn_geometry(nq, nr, d, k);
    const int64_t need = g.n_splits * nq * g.kt * (int64_t)sizeof(float);
    if (need > 0) {
        if (!workspace) return fail(MCPC_EINVAL, "knn: workspace is null (mcpc_knn_workspace_bytes: %lld bytes)", (long long)need);
        if (workspace_bytes < need)
            return fail(MCPC_EINVAL, "knn: workspace of %lld bytes is too small, %lld needed", (long long)workspace_bytes, (long long)need);
    }
    if (nq == 0 || (nr == 0 && accumulate)) return MCPC_OK;      // nothing to write, or nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    KnnParams P{};
    P.q = q; P.ref = ref; P.nq = nq; P.nr = nr; P.d = d; P.k = k;
    P.tiles_per_split = g.tiles_per_split; P.n_tiles = g.n_tiles; P.n_splits = g.n_splits;
    P.part = (float*)workspace; P.best = best; P.accumulate = accumulate ? 1 : 0;
    knn_dispatch(g, P, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

static int loglik_check_shape(int64_t n_data, int64_t n_samp, int32_t width) {
    if (width < 1) return fail(MCPC_EINVAL, "loglik: width=%d, must be at least 1", width);
    if (n_data < 0 || n_data > MCPC_LOGLIK_MAX_ROWS)
        return fail(MCPC_EINVAL, "loglik: n_data=%lld outside 0..%lld", (long long)n_data, (long long)MCPC_LOGLIK_MAX_ROWS);
    if (n_samp < 0 || n_samp > MCPC_LOGLIK_MAX_ROWS)
        return fail(MCPC_EINVAL, "loglik: n_samp=%lld outside 0..%lld", (long long)n_samp, (long long)MCPC_LOGLIK_MAX_ROWS);
    return MCPC_OK;
}

int64_t mcpc_loglik_workspace_bytes(int64_t n_data, int64_t n_samp, int32_t width) {
    if (loglik_check_shape(n_data, n_samp, width)) return -1;
    return loglik_workspace_doubles(loglik_plan(n_data, n_samp, width), n_data, n_samp) * (int64_t)sizeof(double);
}

int mcpc_loglik_accumulate(int device, const float* y, int64_t n_data, const float* out, int64_t n_samp, int32_t width,
                           int32_t loss_kind, double loss_var, double clamp, double* state, int32_t accumulate, void* workspace,
                           int64_t workspace_bytes, void* stream_) {
    if (const int rc = loglik_check_shape(n_data, n_samp, width)) return rc;
    if (loss_kind != MCPC_LOSS_BERNOULLI && loss_kind != MCPC_LOSS_GAUSSIAN)
        return fail(MCPC_EINVAL, "loglik: loss_kind=%d, expected MCPC_LOSS_GAUSSIAN (%d) or MCPC_LOSS_BERNOULLI (%d)", loss_kind,
                    MCPC_LOSS_GAUSSIAN, MCPC_LOSS_BERNOULLI);
    if (loss_kind == MCPC_LOSS_GAUSSIAN && !(loss_var > 0.0)) return fail(MCPC_EINVAL, "loglik: loss_var=%g, must be positive", loss_var);
    if (!(clamp > 0.0)) return fail(MCPC_EINVAL, "loglik: clamp=%g, must be positive (+inf: none)", clamp);
    if (n_data > 0 && !y) return fail(MCPC_EINVAL, "loglik: y is null with n_data=%lld", (long long)n_data);
    if (n_data > 0 && !state) return fail(MCPC_EINVAL, "loglik: state is null with n_data=%lld", (long long)n_data);
    if (n_samp > 0 && !out) return fail(MCPC_EINVAL, "loglik: out is null with n_samp=%lld", (long long)n_samp);
    const LoglikPlan g = loglik_plan(n_data, n_samp, width);
    const int64_t need = loglik_workspace_doubles(g, n_data, n_samp) * (int64_t)sizeof(double);
    if (need > 0) {
        if (!workspace) return fail(MCPC_EINVAL, "loglik: workspace is null (mcpc_loglik_workspace_bytes: %lld bytes)", (long long)need);
        if (workspace_bytes < need)
            return fail(MCPC_EINVAL, "loglik: workspace of %lld bytes is too small, %lld needed", (long long)workspace_bytes, (long long)need);
    }
    if (n_data == 0 || (n_samp == 0 && accumulate)) return MCPC_OK;      // nothing to write, or nothing to add
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(device));
    LoglikParams P{};
    P.y = y; P.o = out; P.n_data = n_data; P.n_samp = n_samp; P.width = width;
    P.gauss = loss_kind == MCPC_LOSS_GAUSSIAN ? 1 : 0;
    P.accumulate = accumulate ? 1 : 0;
    P.vec = (width % 4 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)out % 16 == 0) ? 1 : 0;
    P.clamp = clamp;
    if (P.gauss) {
        P.half_inv_var = 0.5 / loss_var;
        P.cst = 0.5 * (double)width * log(2.0 * M_PI * loss_var);
    }
    P.tiles_per_group = g.tiles_per_group; P.n_stiles = g.n_stiles; P.groups = g.groups; P.ndpad = g.n_dtiles * 16;
    P.part = (double*)workspace;
    P.a = P.part + g.groups * P.ndpad * 4;
    P.b = P.a + n_data;
    P.state = state;
    loglik_dispatch(g, P, stream);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_ais_increment(int device, const float* x, int64_t rows, int32_t width, int32_t act, const float* W, const float* bias,
                       int32_t n_out, const float* y, int32_t loss_kind, double loss_var, int32_t mask_start, double a0, double c0,
                       double a1, double c1, double* logw, int32_t accumulate, void* stream_) {
    if (width < 1) return fail(MCPC_EINVAL, "ais: width=%d, must be at least 1", width);
    if (n_out < 1) return fail(MCPC_EINVAL, "ais: n_out=%d, must be at least 1", n_out);
    if (rows < 0 || rows > MCPC_AIS_MAX_ROWS)
        return fail(MCPC_EINVAL, "ais: rows=%lld outside 0..%lld", (long long)rows, (long long)MCPC_AIS_MAX_ROWS);
    if (mask_start < 0 || mask_start >= n_out) return fail(MCPC_EINVAL, "ais: mask_start=%d outside 0..%d", mask_start, n_out - 1);
    if (act != MCPC_ACT_IDENTITY && act != MCPC_ACT_RELU && act != MCPC_ACT_TANH) return fail(MCPC_EINVAL, "ais: unknown act %d", act);
    if (loss_kind != MCPC_LOSS_BERNOULLI && loss_kind != MCPC_LOSS_GAUSSIAN)
        return fail(MCPC_EINVAL, "ais: loss_kind=%d, expected MCPC_LOSS_GAUSSIAN (%d) or MCPC_LOSS_BERNOULLI (%d)", loss_kind,
                    MCPC_LOSS_GAUSSIAN, MCPC_LOSS_BERNOULLI);
    if (loss_kind == MCPC_LOSS_GAUSSIAN && !(loss_var > 0.0)) return fail(MCPC_EINVAL, "ais: loss_var=%g, must be positive", loss_var);
    if (std::isnan(loss_var) || std::isnan(a0) || std::isnan(c0) || std::isnan(a1) || std::isnan(c1))
        return fail(MCPC_EINVAL, "ais: a scalar is NaN (loss_var=%g a0=%g c0=%g a1=%g c1=%g)", loss_var, a0, c0, a1, c1);
    if (rows > 0 && !x) return fail(MCPC_EINVAL, "ais: x is null with rows=%lld", (long long)rows);
    if (rows > 0 && !W) return fail(MCPC_EINVAL, "ais: W is null with rows=%lld", (long long)rows);
    if (rows > 0 && !y) return fail(MCPC_EINVAL, "ais: y is null with rows=%lld", (long long)rows);
    if (rows > 0 && !logw) return fail(MCPC_EINVAL, "ais: logw is null with rows=%lld", (long long)rows);
    if (rows == 0) return MCPC_OK;                                // no row to write
    HIP_TRY(hipSetDevice(device));
    AisParams P{};
    P.x = x; P.W = W; P.bias = bias; P.y = y; P.logw = logw; P.rows = rows;
    P.width = width; P.n_out = n_out; P.mask_start = mask_start;
    P.gauss = loss_kind == MCPC_LOSS_GAUSSIAN ? 1 : 0;
    P.accumulate = accumulate ? 1 : 0;
    P.tile_begin = mask_start / 16;
    P.n_groups = ((n_out + 15) / 16 - P.tile_begin + kAisTiles - 1) / kAisTiles;
    P.a0 = a0; P.c0 = c0; P.a1 = a1; P.c1 = c1;
    P.half_inv_var = P.gauss ? 0.5 / loss_var : 0.0;
    ais_dispatch(act, P, (hipStream_t)stream_);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

namespace {
// what mcpc_mala_propose and mcpc_mala_accept share: the counts, the two scalars, the widths; `who` opens every message
int mala_check(const char* who, const int32_t* widths, int32_t n_layers, int64_t rows, double lr, double noise_var) {
    if (n_layers < 1 || n_layers > MCPC_MAX_LATENT)
        return fail(MCPC_EINVAL, "%s: n_layers=%d outside 1..%d", who, n_layers, MCPC_MAX_LATENT);
    if (rows < 0 || rows > MCPC_MALA_MAX_ROWS)
        return fail(MCPC_EINVAL, "%s: rows=%lld outside 0..%lld", who, (long long)rows, (long long)MCPC_MALA_MAX_ROWS);
    if (!(lr > 0.0) || !std::isfinite(lr)) return fail(MCPC_EINVAL, "%s: lr=%g, must be positive and finite", who, lr);
    if (!(noise_var > 0.0) || !std::isfinite(noise_var))
        return fail(MCPC_EINVAL, "%s: noise_var=%g, must be positive and finite", who, noise_var);
    if (!widths) return fail(MCPC_EINVAL, "%s: widths is null", who);
    for (int l = 0; l < n_layers; ++l)
        if (widths[l] < 1) return fail(MCPC_EINVAL, "%s: widths[%d]=%d, must be at least 1", who, l, widths[l]);
    return 0;
}
int mala_check_ptrs(const char* who, const char* name, const float* const* p, int32_t n_layers) {
    if (!p) return fail(MCPC_EINVAL, "%s: %s is null", who, name);
    for (int l = 0; l < n_layers; ++l)
        if (!p[l]) return fail(MCPC_EINVAL, "%s: %s[%d] is null", who, name, l);
    return 0;
}
void mala_scalars(MalaParams& P, const int32_t* widths, int32_t n_layers, int64_t rows, double lr, double noise_var, uint64_t seed,
                  uint64_t step, uint64_t chain_base) {
    for (int l = 0; l < n_layers; ++l) P.n[l] = widths[l];
    P.rows = rows; P.n_layers = n_layers;
    P.lr = (float)lr;
    P.s = (float)std::sqrt(noise_var * lr);                       // as mcpc_run rounds the step kernels' noise scale
    P.lr_d = lr;
    P.denom = (2.0 * noise_var) * lr;
    P.seed = seed; P.step = step; P.chain_base = chain_base;
}
}  // namespace

int mcpc_mala_propose(int device, const float* const* x, const float* const* g, const int32_t* widths, int32_t n_layers, int64_t rows,
                      double lr, double noise_var, uint64_t seed, uint64_t step, uint64_t chain_base, float* const* x_out,
                      void* stream_) {
    if (const int rc = mala_check("mala_propose", widths, n_layers, rows, lr, noise_var)) return rc;
    if (rows == 0) return MCPC_OK;                                // no row to write
    if (const int rc = mala_check_ptrs("mala_propose", "x", x, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("mala_propose", "g", g, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("mala_propose", "x_out", x_out, n_layers)) return rc;
    HIP_TRY(hipSetDevice(device));
    MalaParams P{};
    mala_scalars(P, widths, n_layers, rows, lr, noise_var, seed, step, chain_base);
    for (int l = 0; l < n_layers; ++l) {
        P.x[l] = const_cast<float*>(x[l]); P.g[l] = const_cast<float*>(g[l]); P.out[l] = x_out[l];
    }
    P.has_out = 1;
    hipLaunchKernelGGL(mcpc_mala_propose_kernel, mala_grid(rows), dim3(64 * kMalaWaves), 0, (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_mala_accept(int device, float* const* x, float* const* g, double* E, const float* const* x_prop, const float* const* g_prop,
                     const double* E_prop, const int32_t* widths, int32_t n_layers, int64_t rows, double lr, double noise_var,
                     uint64_t seed, uint64_t step, uint64_t chain_base, double* diag, int32_t* n_accepted, float* const* x_next,
                     void* stream_) {
    if (const int rc = mala_check("mala_accept", widths, n_layers, rows, lr, noise_var)) return rc;
    if (rows == 0) return MCPC_OK;                                // no row to decide
    if (const int rc = mala_check_ptrs("mala_accept", "x", x, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("mala_accept", "g", g, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("mala_accept", "x_prop", x_prop, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("mala_accept", "g_prop", g_prop, n_layers)) return rc;
    if (x_next)
        if (const int rc = mala_check_ptrs("mala_accept", "x_next", x_next, n_layers)) return rc;
    if (!E) return fail(MCPC_EINVAL, "mala_accept: E is null with rows=%lld", (long long)rows);
    if (!E_prop) return fail(MCPC_EINVAL, "mala_accept: E_prop is null with rows=%lld", (long long)rows);
    HIP_TRY(hipSetDevice(device));
    MalaParams P{};
    mala_scalars(P, widths, n_layers, rows, lr, noise_var, seed, step, chain_base);
    for (int l = 0; l < n_layers; ++l) {
        P.x[l] = x[l]; P.g[l] = g[l]; P.xp[l] = x_prop[l]; P.gp[l] = g_prop[l];
        if (x_next) P.out[l] = x_next[l];
    }
    P.E = E; P.Ep = E_prop; P.diag = diag; P.n_accepted = n_accepted;
    P.has_out = x_next ? 1 : 0;
    hipLaunchKernelGGL(mcpc_mala_accept_kernel, mala_grid(rows), dim3(64 * kMalaWaves), 0, (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

namespace {
// what the three mcpc_hmc entries share: MALA's checks (a unit-mass Hamiltonian has no noise scale: 2 stands in), then the scalars
int hmc_check(const char* who, const int32_t* widths, int32_t n_layers, int64_t rows, double lr) {
    if (rows > MCPC_HMC_MAX_ROWS)
        return fail(MCPC_EINVAL, "%s: rows=%lld outside 0..%lld", who, (long long)rows, (long long)MCPC_HMC_MAX_ROWS);
    return mala_check(who, widths, n_layers, rows, lr, 2.0);
}
void hmc_scalars(HmcParams& P, const int32_t* widths, int32_t n_layers, int64_t rows, double lr, uint64_t seed, uint64_t step,
                 uint64_t chain_base) {
    for (int l = 0; l < n_layers; ++l) P.n[l] = widths[l];
    P.rows = rows; P.n_layers = n_layers;
    P.eps = (float)std::sqrt(2.0 * lr);                           // formed in double, rounded once
    P.h = 0.5f * P.eps;                                           // exact
    P.seed = seed; P.step = step; P.chain_base = chain_base;
}
}  // namespace

int mcpc_hmc_begin(int device, const float* const* x, const float* const* g, const int32_t* widths, int32_t n_layers, int64_t rows,
                   double lr, uint64_t seed, uint64_t step, uint64_t chain_base, float* const* q_out, float* const* x_out, double* K0,
                   void* stream_) {
    if (const int rc = hmc_check("hmc_begin", widths, n_layers, rows, lr)) return rc;
    if (rows == 0) return MCPC_OK;                                // no row to write
    if (const int rc = mala_check_ptrs("hmc_begin", "x", x, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_begin", "g", g, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_begin", "q_out", q_out, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_begin", "x_out", x_out, n_layers)) return rc;
    if (!K0) return fail(MCPC_EINVAL, "hmc_begin: K0 is null with rows=%lld", (long long)rows);
    HIP_TRY(hipSetDevice(device));
    HmcParams P{};
    hmc_scalars(P, widths, n_layers, rows, lr, seed, step, chain_base);
    for (int l = 0; l < n_layers; ++l) {
        P.x[l] = const_cast<float*>(x[l]); P.g[l] = const_cast<float*>(g[l]); P.q[l] = q_out[l]; P.xt[l] = x_out[l];
    }
    P.K0 = K0;
    hipLaunchKernelGGL(mcpc_hmc_begin_kernel, mala_grid(rows), dim3(64 * kMalaWaves), 0, (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_hmc_leap(int device, float* const* x_t, float* const* q, const float* const* g_t, const int32_t* widths, int32_t n_layers,
                  int64_t rows, double lr, void* stream_) {
    if (const int rc = hmc_check("hmc_leap", widths, n_layers, rows, lr)) return rc;
    if (rows == 0) return MCPC_OK;                                // no row to move
    if (const int rc = mala_check_ptrs("hmc_leap", "x_t", x_t, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_leap", "q", q, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_leap", "g_t", g_t, n_layers)) return rc;
    HIP_TRY(hipSetDevice(device));
    HmcParams P{};
    hmc_scalars(P, widths, n_layers, rows, lr, 0, 0, 0);
    for (int l = 0; l < n_layers; ++l) { P.xt[l] = x_t[l]; P.q[l] = q[l]; P.gt[l] = g_t[l]; }
    hipLaunchKernelGGL(mcpc_hmc_leap_kernel, mala_grid(rows), dim3(64 * kMalaWaves), 0, (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_hmc_accept(int device, float* const* x, float* const* g, double* E, const float* const* x_t, const float* const* g_t,
                    const double* E_t, const float* const* q, const double* K0, const int32_t* widths, int32_t n_layers, int64_t rows,
                    double lr, uint64_t seed, uint64_t step, uint64_t chain_base, double* diag, int32_t* n_accepted, void* stream_) {
    if (const int rc = hmc_check("hmc_accept", widths, n_layers, rows, lr)) return rc;
    if (rows == 0) return MCPC_OK;                                // no row to decide
    if (const int rc = mala_check_ptrs("hmc_accept", "x", x, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_accept", "g", g, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_accept", "x_t", x_t, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_accept", "g_t", g_t, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("hmc_accept", "q", q, n_layers)) return rc;
    if (!E) return fail(MCPC_EINVAL, "hmc_accept: E is null with rows=%lld", (long long)rows);
    if (!E_t) return fail(MCPC_EINVAL, "hmc_accept: E_t is null with rows=%lld", (long long)rows);
    if (!K0) return fail(MCPC_EINVAL, "hmc_accept: K0 is null with rows=%lld", (long long)rows);
    HIP_TRY(hipSetDevice(device));
    HmcParams P{};
    hmc_scalars(P, widths, n_layers, rows, lr, seed, step, chain_base);
    for (int l = 0; l < n_layers; ++l) {
        P.x[l] = x[l]; P.g[l] = g[l]; P.xt[l] = const_cast<float*>(x_t[l]); P.gt[l] = g_t[l]; P.q[l] = const_cast<float*>(q[l]);
    }
    P.E = E; P.Et = E_t; P.K0 = const_cast<double*>(K0); P.diag = diag; P.n_accepted = n_accepted;
    hipLaunchKernelGGL(mcpc_hmc_accept_kernel, mala_grid(rows), dim3(64 * kMalaWaves), 0, (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_smc_ancestors(int device, double* logw, int64_t n_data, int32_t replicas, double threshold, uint64_t seed, uint64_t step,
                       uint64_t chain_base, int32_t* ancestors, double* diag, void* stream_) {
    if (replicas < 1 || replicas > MCPC_SMC_MAX_REPLICAS)
        return fail(MCPC_EINVAL, "smc_ancestors: replicas=%d outside 1..%d", replicas, MCPC_SMC_MAX_REPLICAS);
    if (n_data < 0 || n_data > MCPC_SMC_MAX_ROWS / replicas)
        return fail(MCPC_EINVAL, "smc_ancestors: n_data=%lld with replicas=%d: rows outside 0..%lld", (long long)n_data, replicas,
                    (long long)MCPC_SMC_MAX_ROWS);
    if (!(threshold >= 0.0 && threshold <= 1.0))
        return fail(MCPC_EINVAL, "smc_ancestors: threshold=%g outside [0, 1]", threshold);
    if (n_data == 0) return MCPC_OK;                              // no datum to resample
    if (!logw) return fail(MCPC_EINVAL, "smc_ancestors: logw is null with n_data=%lld", (long long)n_data);
    if (!ancestors) return fail(MCPC_EINVAL, "smc_ancestors: ancestors is null with n_data=%lld", (long long)n_data);
    HIP_TRY(hipSetDevice(device));
    SmcParams P{};
    P.logw = logw; P.ancestors = ancestors; P.diag = diag; P.n_data = n_data; P.replicas = replicas; P.threshold = threshold;
    P.seed = seed; P.step = step; P.chain_base = chain_base;
    hipLaunchKernelGGL(mcpc_smc_ancestors_kernel, dim3((unsigned)n_data), dim3(kSmcLanes), (size_t)replicas * sizeof(double),
                       (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_smc_gather(int device, const float* const* x, const int32_t* widths, int32_t n_layers, int64_t rows, const int32_t* ancestors,
                    float* const* x_out, int32_t* n_bad, void* stream_) {
    if (n_layers < 1 || n_layers > MCPC_MAX_LATENT)
        return fail(MCPC_EINVAL, "smc_gather: n_layers=%d outside 1..%d", n_layers, MCPC_MAX_LATENT);
    if (rows < 0 || rows > MCPC_SMC_MAX_ROWS)
        return fail(MCPC_EINVAL, "smc_gather: rows=%lld outside 0..%lld", (long long)rows, (long long)MCPC_SMC_MAX_ROWS);
    if (!widths) return fail(MCPC_EINVAL, "smc_gather: widths is null");
    for (int l = 0; l < n_layers; ++l)
        if (widths[l] < 1) return fail(MCPC_EINVAL, "smc_gather: widths[%d]=%d, must be at least 1", l, widths[l]);
    if (rows == 0) return MCPC_OK;                                // no row to write
    if (const int rc = mala_check_ptrs("smc_gather", "x", x, n_layers)) return rc;
    if (const int rc = mala_check_ptrs("smc_gather", "x_out", x_out, n_layers)) return rc;
    if (!ancestors) return fail(MCPC_EINVAL, "smc_gather: ancestors is null with rows=%lld", (long long)rows);
    HIP_TRY(hipSetDevice(device));
    SmcGatherParams P{};
    for (int l = 0; l < n_layers; ++l) { P.x[l] = x[l]; P.out[l] = x_out[l]; P.n[l] = widths[l]; }
    P.ancestors = ancestors; P.n_bad = n_bad; P.rows = rows; P.n_layers = n_layers;
    hipLaunchKernelGGL(mcpc_smc_gather_kernel, smc_gather_grid(rows), dim3(64 * kSmcWaves), 0, (hipStream_t)stream_, P);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

}  // extern "C"
