// Resampling the replicas of annealed importance sampling (include/mcpc.h: mcpc_smc_ancestors, mcpc_smc_gather): the step that turns
// AIS into a sequential Monte Carlo sampler (Del Moral, Doucet & Jasra 2006).  Datum i owns rows i R .. i R + R - 1 of a chunk, with
// one fp64 log-weight each; when the effective sample size of those R weights falls below threshold * R the datum draws R ancestors
// by SYSTEMATIC resampling (one uniform per datum), every slot takes its ancestor's state, and all R log-weights become the log of
// the mean weight.  The state itself is moved by the gather kernel below; these kernels see log-weights and indices only.
//
// ANCESTORS, per datum, fp64, EVERY OPERATION ROUNDED SEPARATELY (nothing is contracted into an fma: `#pragma clang fp contract(off)`):
//     ok_j = isfinite(logw_j)    cnt = #ok    m = max_ok logw_j                 (cnt = 0: ess = NaN, identity ancestors, logw not written)
//     e_j  = ok_j ? exp(logw_j - m) : 0
//     c_j  = c_{j-1} + e_j       q_j = q_{j-1} + fl(e_j e_j)                    in replica order, SEQUENTIALLY: np.cumsum
//     S    = c_{R-1}             ess = fl(S S) / q_{R-1}
//     resample = ess < fl(threshold (double)R)                                   (false for a NaN)
//     u    = (w >> 8) 2^-24 + 2^-25,  w = word 0 of philox4x32_10(chain_base + i R, 0xFE << 24, step lo, step hi; key seed)
//     p_s  = fl(fl(fl((double)s + u) / (double)R) S)      a_s = #{j : c_j <= p_s}, clamped to the last j with e_j > 0
//     ancestors[i R + s] = i R + a_s          logw[i R + s] = m + log(S / cnt)   for all R slots
// u is exact in fp64 and inside (0, 1).  A datum that does not resample gets identity ancestors and its logw is NOT written.
// Layer 0xFE is outside every layer another consumer of the Philox stream uses: the normals of the step kernels and of
// mcpc_mala_propose take layers 0 .. MCPC_MAX_LATENT - 1, mcpc_sample_prior layers 0 .. MCPC_MAX_LATENT (the read-out's draw), and the
// uniform of mcpc_mala_accept layer 0xFF (mcpc_mala.h) and that of mcpc_hmc_accept layer 0xFD (mcpc_hmc.h), so no Philox word is
// consumed twice.
//
// One workgroup of 256 lanes serves one datum.  The exps run in parallel into LDS (R doubles: 32 KiB at MCPC_SMC_MAX_REPLICAS = 4096);
// m and cnt are a maximum and an integer count, which no order of evaluation changes; lane 0 then walks the two sums, overwriting e_j
// with c_j in place (eight loads in flight at a time); the slots then search c in parallel (a binary search: c is non-decreasing).
// The sequential walk is deliberate: it is the one order a restatement can reproduce (tests/smc_cases.py), and R <= 4096 bounds it.
// A datum's result depends on its own R log-weights, threshold, seed, step and chain_base + i R alone: not on n_data, the other data
// or the launch shape, and two runs are bitwise equal.  No atomics, no workspace.
// Bounds: lane t touches replicas t, t + 256, ... < R of datum blockIdx.x < n_data only; all offsets are 64-bit.
//
// GATHER, out of place: x_out_l[r] = x_l[ancestors[r]], bitwise, every layer in one launch; a workgroup is four waves, a wave one
// destination row, as in the MALA kernels.  An index outside 0 .. rows - 1 is never dereferenced: that row copies itself, and when
// n_bad is given it is incremented by one for the row -- the one atomic of this header, on a counter that exists for this purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_device.h"

namespace mcpc {

constexpr int kSmcLanes = 256;          // lanes of the workgroup that serves a datum
constexpr int kSmcWaves = 4;            // gather: waves (destination rows) of a workgroup
constexpr uint32_t kSmcLayer = 0xFEu;   // the layer index of the resampling uniform

struct SmcParams {
    double* logw;                       // [n_data * replicas]; overwritten for a resampled datum
    int32_t* ancestors;                 // [n_data * replicas]
    double* diag;                       // [n_data][4] or nullptr
    int64_t n_data;
    int32_t replicas;
    double threshold;
    uint64_t seed, step, chain_base;
};

struct SmcGatherParams {
    const float* x[MCPC_MAX_LATENT];
    float* out[MCPC_MAX_LATENT];
    int32_t n[MCPC_MAX_LATENT];
    const int32_t* ancestors;           // [rows]
    int32_t* n_bad;                     // one counter or nullptr
    int64_t rows;
    int32_t n_layers;
};

__global__ __launch_bounds__(kSmcLanes) void mcpc_smc_ancestors_kernel(const SmcParams P) {
    extern __shared__ double smc_c[];                                   // [R]: e_j, then c_j
    __shared__ double sh_m[kSmcLanes / 64];
    __shared__ int32_t sh_cnt[kSmcLanes / 64];
    __shared__ double sh_S, sh_q;
    __shared__ int32_t sh_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t R = P.replicas;
    const int64_t row0 = (int64_t)blockIdx.x * R;                       // (the grid is n_data workgroups)
    double* logw = P.logw + row0;
    int32_t* anc = P.ancestors + row0;

    // m and cnt: a maximum and a count, the same in any order
    double m = -INFINITY;
    int32_t cnt = 0;
    for (int32_t j = tid; j < R; j += kSmcLanes) {
        const double v = logw[j];
        if (isfinite(v)) { m = fmax(m, v); ++cnt; }
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        m = fmax(m, __shfl_xor(m, k, 64));
        cnt += __shfl_xor(cnt, k, 64);
    }
    if (lane == 0) { sh_m[wave] = m; sh_cnt[wave] = cnt; }
    __syncthreads();
    m = sh_m[0]; cnt = sh_cnt[0];
#pragma unroll
    for (int w = 1; w < kSmcLanes / 64; ++w) { m = fmax(m, sh_m[w]); cnt += sh_cnt[w]; }

    uint32_t w4[4];
    const uint32_t chain = (uint32_t)(P.chain_base + (uint64_t)row0);
    philox4x32_10(chain, kSmcLayer << 24, (uint32_t)P.step, (uint32_t)(P.step >> 32), (uint32_t)P.seed, (uint32_t)(P.seed >> 32), w4);
    const double u = (double)(w4[0] >> 8) * 0x1p-24 + 0x1p-25;           // exact: 24 bits and one more

    if (cnt == 0) {                                                     // workgroup-uniform
        for (int32_t s = tid; s < R; s += kSmcLanes) anc[s] = (int32_t)(row0 + s);
        if (tid == 0 && P.diag) {
            double* dg = P.diag + (int64_t)blockIdx.x * 4;
            dg[0] = NAN; dg[1] = 0.0; dg[2] = u; dg[3] = NAN;
        }
        return;
    }

    for (int32_t j = tid; j < R; j += kSmcLanes) {
        const double v = logw[j];
        smc_c[j] = isfinite(v) ? exp(v - m) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
#pragma clang fp contract(off)
        double c = 0.0, q = 0.0;
        int32_t last = 0;
        int32_t j = 0;
        for (; j + 8 <= R; j += 8) {
            double e[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = smc_c[j + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double ee = e[k] * e[k];
                c = c + e[k];
                q = q + ee;
                smc_c[j + k] = c;
                if (e[k] > 0.0) last = j + k;
            }
        }
        for (; j < R; ++j) {
            const double e = smc_c[j];
            const double ee = e * e;
            c = c + e;
            q = q + ee;
            smc_c[j] = c;
            if (e > 0.0) last = j;
        }
        sh_S = c; sh_q = q; sh_last = last;
    }
    __syncthreads();
    const double S = sh_S, q = sh_q;
    const int32_t last = sh_last;
    double ess, bar, neww;
    {
#pragma clang fp contract(off)
        const double ss = S * S;
        ess = ss / q;
        bar = P.threshold * (double)R;
        const double mean = S / (double)cnt;
        const double lg = log(mean);
        neww = m + lg;
    }
    const bool resample = ess < bar;                                    // false for a NaN
    if (tid == 0 && P.diag) {
        double* dg = P.diag + (int64_t)blockIdx.x * 4;
        dg[0] = ess; dg[1] = resample ? 1.0 : 0.0; dg[2] = u; dg[3] = neww;
    }
    if (!resample) {                                                    // workgroup-uniform
        for (int32_t s = tid; s < R; s += kSmcLanes) anc[s] = (int32_t)(row0 + s);
        return;
    }
    for (int32_t s = tid; s < R; s += kSmcLanes) {
        double p;
        {
#pragma clang fp contract(off)
            const double su = (double)s + u;
            const double f = su / (double)R;
            p = f * S;
        }
        int32_t lo = 0, hi = R;                                         // a = #{j : c_j <= p}: the first j with c_j > p
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (smc_c[mid] <= p) lo = mid + 1; else hi = mid;
        }
        const int32_t a = lo < last ? lo : last;
        anc[s] = (int32_t)(row0 + a);
        logw[s] = neww;
    }
}

__global__ __launch_bounds__(64 * kSmcWaves) void mcpc_smc_gather_kernel(const SmcGatherParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kSmcWaves + wave;
    if (r >= P.rows) return;                                            // wave-uniform; the kernel has no barrier
    int64_t a = (int64_t)P.ancestors[r];
    if (a < 0 || a >= P.rows) {                                         // never dereferenced: the row copies itself
        a = r;
        if (lane == 0 && P.n_bad) atomicAdd(P.n_bad, 1);
    }
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const float* src = P.x[l] + a * (int64_t)n;
        float* dst = P.out[l] + r * (int64_t)n;
        for (int32_t u = lane; u < n; u += 64) dst[u] = src[u];
    }
}

inline dim3 smc_gather_grid(int64_t rows) { return dim3((unsigned)((rows + kSmcWaves - 1) / kSmcWaves)); }

}  // namespace mcpc
