// Importance-sampled log marginal likelihood PER DATUM from read-outs of prior samples (include/mcpc.h: mcpc_loglik_accumulate): the hot
// path of the reference's get_marginal_likelihood (utils/training_evaluation.py), which forms softplus(o).sum(1) - data @ o.T in fp32,
// one [B, S] matrix per batch, and keeps one scalar.  Here, for datum i and sample s, with c = clamp(o):
//   Bernoulli  nll(i, s) = b_s - sum_j y_ij c_sj                                   b_s = sum_j softplus(c_sj)
//   Gaussian   nll(i, s) = (0.5 / var) (a_i + b_s - 2 sum_j y_ij c_sj) + 0.5 width log(2 pi var)     a_i = sum_j y_ij^2, b_s = sum_j c_sj^2
//   state[i]   = { m, s1, s2, cnt }: m = min_s nll, s1 = sum_s e^-(nll - m), s2 = sum_s e^-2(nll - m), cnt = samples taken
// so that log p(y_i) ~ log(s1 / cnt) - m and the effective sample size of the weights is s1^2 / s2.
//
// Everything is fp64.  The dot products run on v_mfma_f64_16x16x4_f64 with the operands converted from fp32 on load: an fp32 value and
// the product of two of them are exact in fp64 (a clamp that is no fp32 value rounds the product once), so the roundings are the
// additions.  a_i and b_s come from mcpc_loglik_prep_kernel: one wave per row, lane l sums columns l, l + 64, ... ascending, then a
// butterfly over the lanes -- one fixed order.  softplus(c) = max(c, 0) + log1p(exp(-|c|)), in fp64.
//
// A job is (16-datum tile, group of consecutive 16-sample tiles) and belongs to one wave (a workgroup of 64 lanes): no LDS, no barrier,
// no atomics, no wait on another wave.  The A operand is the samples, the B operand the data: lane (m = lane & 15, q = lane >> 4) holds
// D[sample q + 4 reg][datum m], i.e. a lane sees ONE datum and keeps that datum's online (m, s1, s2, cnt) over the samples it is handed;
// the four lanes of a datum are merged in ascending q at the end, and the wave writes the partial state of its 16 data into the
// caller's workspace ([group][padded datum][4]).  mcpc_loglik_finish_kernel, one lane per datum, merges the partials in ascending group
// order and then, when accumulating, the old state.  The grouping depends on (n_data, n_samp) alone and aims at kLoglikTargetJobs waves:
// at 10 000 x 5 000 x 784 a target of one wave per SIMD (1 024, as cov_plan's) took 3.59 ms, 4 096 took 2.52 ms and 8 192 takes 2.44 ms
// on one MI355X -- three waves are resident per SIMD and hide each other's waits, and the more jobs there are, the smaller the share of
// the last round of them.
//
// The width is walked in k-steps of 4, four at a time: lane (m, q) loads columns k0 + 4 q + (0..3) of its row with one 16-byte load
// (element-wise when the width is no multiple of 4 or a base is not 16-byte aligned) and MFMA j of the four contracts columns
// k0 + 4 q + j, q = 0..3 -- the same places on both operands, so sixteen columns are covered once each.  Two sample tiles share the
// data fragment.  The wave's 16 data rows are RE-READ FROM L2 per pair of sample tiles, not staged in LDS: a 16 x 16 x 4 fp64 MFMA
// occupies the matrix unit for 64 cycles, so a wave asks for 48 bytes per lane every 512 MFMA cycles, a small share of what L2 delivers,
// whereas 16 rows of 784 floats are 50 KB per wave and four waves of a compute unit would not fit its 160 KB of LDS.
//
// Bounds: rows beyond n_data / n_samp and columns beyond the width contribute exact zeros and READ NOTHING BEYOND THEIR BUFFER
// (mcpc_cov.h's rule): such a lane is pointed at element 0 of its own buffer and discards what it gets, which keeps the loads free of
// branches.  A sample beyond n_samp is excluded by its index, never by its value, and a datum beyond n_data is never written to
// state.  All offsets are 64-bit.
//
// Non-finite values: a (datum, sample) pair whose nll is not finite is neither taken nor counted.  A NaN in a sample's row reaches the
// MFMA results of that row alone, a NaN in a datum's row those of that column alone: nothing else changes, bit for bit.
//
// What is bitwise: two runs of the same call.  What holds within a bound only: the same samples chunked differently over calls, or in
// another order -- the running minimum rescales the sums at different points (tests/loglik_cases.py derives the bound).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpc.h"

namespace mcpc {

constexpr int kLoglikTargetJobs = 8192;     // groups are sized for about this many waves: 8 per SIMD of 256 CUs x 4 SIMDs, 3 of them resident
constexpr int kLoglikInFlight = 2;          // 16-column chunks whose fragments are loaded before the first is consumed

typedef double ll_d4 __attribute__((ext_vector_type(4)));

// The host's plan: depends on the shape alone (not on the device), so the workspace size is a function of the shape.
struct LoglikPlan {
    int64_t n_dtiles, n_stiles, tiles_per_group, groups;
};

inline LoglikPlan loglik_plan(int64_t n_data, int64_t n_samp, int32_t /*width*/) {
    LoglikPlan p{};
    p.n_dtiles = (n_data + 15) / 16;
    p.n_stiles = (n_samp + 15) / 16;
    if (p.n_dtiles == 0 || p.n_stiles == 0) { p.n_dtiles = p.n_stiles = 0; return p; }
    int64_t want = (kLoglikTargetJobs + p.n_dtiles - 1) / p.n_dtiles;
    if (want > p.n_stiles) want = p.n_stiles;
    p.tiles_per_group = (p.n_stiles + want - 1) / want;
    p.groups = (p.n_stiles + p.tiles_per_group - 1) / p.tiles_per_group;
    return p;
}

// workspace: part [groups][16 n_dtiles][4], then a [n_data], then b [n_samp], all fp64
inline int64_t loglik_workspace_doubles(const LoglikPlan& p, int64_t n_data, int64_t n_samp) {
    if (p.groups == 0) return 0;
    return p.groups * p.n_dtiles * 16 * 4 + n_data + n_samp;
}

struct LoglikParams {
    const float* y;         // [n_data][width]
    const float* o;         // [n_samp][width]
    int64_t n_data, n_samp;
    int32_t width, gauss, accumulate, vec;
    double clamp, half_inv_var, cst;    // Gaussian: 0.5 / var and 0.5 width log(2 pi var)
    int64_t tiles_per_group, n_stiles, groups, ndpad;
    double* part;           // workspace [groups][ndpad][4]
    double* a;              // workspace [n_data] (Gaussian only)
    double* b;              // workspace [n_samp]
    double* state;          // [n_data][4]
};

struct LoglikState {
    double m, s1, s2, cnt;
};

__device__ __forceinline__ LoglikState ll_empty() { return LoglikState{(double)INFINITY, 0.0, 0.0, 0.0}; }

// NaN stays NaN (fmin / fmax would replace it by the bound)
__device__ __forceinline__ double ll_clamp(double v, double cl) { return v < -cl ? -cl : (v > cl ? cl : v); }

__device__ __forceinline__ double ll_softplus(double c) { return (c > 0.0 ? c : 0.0) + log1p(exp(-fabs(c))); }

// The merge rule of include/mcpc.h.  An empty side has the factor 0; inf - inf is never formed.
__device__ __forceinline__ LoglikState ll_merge(const LoglikState& A, const LoglikState& B) {
    const double m = A.m < B.m ? A.m : B.m;
    if (!(m < (double)INFINITY)) return ll_empty();
    const double fA = A.m < (double)INFINITY ? exp(m - A.m) : 0.0;
    const double fB = B.m < (double)INFINITY ? exp(m - B.m) : 0.0;
    LoglikState r;
    r.m = m;
    r.s1 = A.s1 * fA + B.s1 * fB;
    r.s2 = A.s2 * (fA * fA) + B.s2 * (fB * fB);
    r.cnt = A.cnt + B.cnt;
    return r;
}

// one finite nll into a lane's online state: a single exp, of -|m - v| (m = +inf: exp(-inf) = 0)
__device__ __forceinline__ void ll_take(LoglikState& st, double v) {
    const bool lower = v < st.m;
    const double t = exp(lower ? v - st.m : st.m - v);
    const double t2 = t * t;
    st.s1 = lower ? st.s1 * t + 1.0 : st.s1 + t;
    st.s2 = lower ? st.s2 * t2 + 1.0 : st.s2 + t2;
    st.m = lower ? v : st.m;
    st.cnt += 1.0;
}

// a[i] = sum_j y_ij^2 (Gaussian), b[s] = sum_j softplus(c_sj) or sum_j c_sj^2: one wave per row, rows [0, n_data) of y then [0, n_samp) of o
__global__ __launch_bounds__(256) void mcpc_loglik_prep_kernel(const LoglikParams P) {
    const int lane = threadIdx.x & 63;
    const int64_t n_a = P.gauss ? P.n_data : 0;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_a + P.n_samp) return;                                  // wave-uniform
    const bool is_a = row < n_a;
    const float* src = is_a ? P.y + row * (int64_t)P.width : P.o + (row - n_a) * (int64_t)P.width;
    double s = 0.0;
    for (int32_t j = lane; j < P.width; j += 64) {
        double v = (double)src[j];
        if (!is_a) v = ll_clamp(v, P.clamp);
        s += (is_a || P.gauss) ? v * v : ll_softplus(v);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) {
        if (is_a) P.a[row] = s;
        else P.b[row - n_a] = s;
    }
}

// columns c .. c + 3 of a row.  row == nullptr or a column beyond the width: an exact zero, and the lane is pointed at the first
// element(s) of its own buffer (`safe`), whose value it discards -- no address outside the buffer is ever formed, and the loads stay
// free of branches (a branch per load would put a wait for it behind every one of them).
template <bool kVec>
__device__ __forceinline__ void ll_load4(const float* row, const float* safe, int32_t c, int32_t width, float (&v)[4]) {
    if (kVec) {                                                         // width % 4 == 0 and c % 4 == 0: c < width covers c + 3
        const bool ok = row && c < width;
        const float4 t = *reinterpret_cast<const float4*>(ok ? row + c : safe);
        v[0] = ok ? t.x : 0.0f; v[1] = ok ? t.y : 0.0f; v[2] = ok ? t.z : 0.0f; v[3] = ok ? t.w : 0.0f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = row && c + j < width;
            const float t = *(ok ? row + c + j : safe);
            v[j] = ok ? t : 0.0f;
        }
    }
}

struct LoglikFrag {
    float y[kLoglikInFlight][4], o0[kLoglikInFlight][4], o1[kLoglikInFlight][4];
};

template <bool kVec>
__global__ __launch_bounds__(64) void mcpc_loglik_kernel(const LoglikParams P) {
    const int lane = threadIdx.x, m = lane & 15, q = lane >> 4;
    // job -> (datum tile, group); wave-uniform
    const int64_t dt = (int64_t)blockIdx.x / P.groups, g = (int64_t)blockIdx.x % P.groups;
    const int64_t d0 = dt * 16;
    const int64_t t_begin = g * P.tiles_per_group;
    const int64_t t_end = t_begin + P.tiles_per_group < P.n_stiles ? t_begin + P.tiles_per_group : P.n_stiles;
    const int32_t width = P.width;
    const double cl = P.clamp;

    const bool datum_ok = d0 + m < P.n_data;
    const float* yrow = datum_ok ? P.y + (d0 + m) * (int64_t)width : nullptr;
    const double a_i = P.gauss ? P.a[datum_ok ? d0 + m : 0] : 0.0;
    LoglikState st = ll_empty();

    for (int64_t t = t_begin; t < t_end; t += 2) {
        // two sample tiles share the data fragment; the second may lie beyond the group's end
        const int64_t sA = t * 16 + m, sB = (t + 1) * 16 + m;
        const float* orow0 = sA < P.n_samp ? P.o + sA * (int64_t)width : nullptr;
        const float* orow1 = (t + 1 < t_end && sB < P.n_samp) ? P.o + sB * (int64_t)width : nullptr;
        // b_s of the eight samples this lane will see, asked for before the contraction (a sample beyond the end: b[0], not used)
        double b_s[2][4];
        bool s_ok[2][4];
#pragma unroll
        for (int ts = 0; ts < 2; ++ts)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t s = (t + ts) * 16 + q + 4 * reg;
                s_ok[ts][reg] = t + ts < t_end && s < P.n_samp && datum_ok;
                b_s[ts][reg] = P.b[s_ok[ts][reg] ? s : 0];
            }
        auto load = [&](int32_t k0, LoglikFrag& f) {
#pragma unroll
            for (int u = 0; u < kLoglikInFlight; ++u) {
                const int32_t c = k0 + 16 * u + 4 * q;
                ll_load4<kVec>(yrow, P.y, c, width, f.y[u]);
                ll_load4<kVec>(orow0, P.o, c, width, f.o0[u]);
                ll_load4<kVec>(orow1, P.o, c, width, f.o1[u]);
            }
        };
        ll_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        LoglikFrag next;
        load(0, next);
        for (int32_t k0 = 0; k0 < width; k0 += 16 * kLoglikInFlight) {
            const LoglikFrag cur = next;
            load(k0 + 16 * kLoglikInFlight, next);                       // the chunks after these, in flight under the MFMAs (past the width: zeros)
#pragma unroll
            for (int u = 0; u < kLoglikInFlight; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dy = (double)cur.y[u][j];
                    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ll_clamp((double)cur.o0[u][j], cl), dy, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ll_clamp((double)cur.o1[u][j], cl), dy, acc1, 0, 0, 0);
                }
        }
        // C/D layout of the f64 form: col (datum) = lane & 15, row (sample) = (lane >> 4) + 4 reg
#pragma unroll
        for (int ts = 0; ts < 2; ++ts)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const double dot = ts ? acc1[reg] : acc0[reg];
                const double v = P.gauss ? P.half_inv_var * (a_i + b_s[ts][reg] - 2.0 * dot) + P.cst : b_s[ts][reg] - dot;
                if (s_ok[ts][reg] && fabs(v) < (double)INFINITY) ll_take(st, v);     // false for NaN and both infinities
            }
    }

    // the four lanes of a datum, in ascending q, on lane q = 0
    LoglikState r = st;
#pragma unroll
    for (int qq = 1; qq < 4; ++qq) {
        LoglikState other;
        other.m = __shfl(st.m, m + 16 * qq, 64);
        other.s1 = __shfl(st.s1, m + 16 * qq, 64);
        other.s2 = __shfl(st.s2, m + 16 * qq, 64);
        other.cnt = __shfl(st.cnt, m + 16 * qq, 64);
        r = ll_merge(r, other);
    }
    if (q == 0) {
        double* p = P.part + (g * P.ndpad + d0 + m) * 4;                 // the workspace is padded to whole datum tiles
        p[0] = r.m; p[1] = r.s1; p[2] = r.s2; p[3] = r.cnt;
    }
}

// One lane per datum: the groups' partial states in ascending order, then the old state when accumulating.  groups = 0: the empty state.
__global__ __launch_bounds__(256) void mcpc_loglik_finish_kernel(const LoglikParams P) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n_data) return;
    LoglikState st = ll_empty();
    for (int64_t g = 0; g < P.groups; ++g) {
        const double* p = P.part + (g * P.ndpad + i) * 4;
        st = ll_merge(st, LoglikState{p[0], p[1], p[2], p[3]});
    }
    double* out = P.state + i * 4;
    if (P.accumulate) st = ll_merge(LoglikState{out[0], out[1], out[2], out[3]}, st);
    out[0] = st.m; out[1] = st.s1; out[2] = st.s2; out[3] = st.cnt;
}

inline void loglik_dispatch(const LoglikPlan& p, const LoglikParams& P, hipStream_t stream) {
    if (p.groups > 0) {
        const int64_t rows = (P.gauss ? P.n_data : 0) + P.n_samp;
        hipLaunchKernelGGL(mcpc_loglik_prep_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, P);
        const dim3 grid((unsigned)(p.n_dtiles * p.groups)), block(64);
        if (P.vec) hipLaunchKernelGGL(mcpc_loglik_kernel<true>, grid, block, 0, stream, P);
        else hipLaunchKernelGGL(mcpc_loglik_kernel<false>, grid, block, 0, stream, P);
    }
    hipLaunchKernelGGL(mcpc_loglik_finish_kernel, dim3((unsigned)((P.n_data + 255) / 256)), dim3(256), 0, stream, P);
}

}  // namespace mcpc
