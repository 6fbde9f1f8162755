// Ksp  Ancestral samples of the generative model (include/mcpc.h: mcpc_sample_prior; DESIGN.md section 4 "Small kernels").
//
// The forward pass of mcpc_pred_err.h run as a GENERATOR.  A ROW is one sample with the global id g = sample_base + row.  Layer after
// layer the kernel forms the prediction mu_j = f(x_{j-1}) W_j^T + b_j exactly as mcpc_pe_kernel does -- mcpc_mu1_kernel for Linear 0, the
// tile of the layer-wise forward launch (4 waves, 64 rows x 128 units, lw_job_gemm as it is) on the engine's packed weights -- so that a
// prediction is bitwise what mcpc_prediction_errors writes as pred[j] for the same x_{j-1}; then, instead of comparing with a record,
//   x_j = mu_j + s_j z_j      s_j = (float)(1 / sqrt((double)ecoef_j)),   z_j = normals4(seed, step, layer j, chain (uint32)g, group u / 4):
//                             the step kernels' Philox + Box-Muller stream, what mcpc_philox_normals returns for chain_base = sample_base.
//                             t = s_j z and mu + t are two fp32 roundings, never one fma.
// THE PRIOR IS THE ENERGY'S: the layer energy c 0.5 (x - mu)^2 is the negative log density of N(mu, 1/c), which is what unclamped
// Langevin sampling converges to.  The reference's sample_pc (utils/training_evaluation.py) draws mean + randn whatever the coefficient;
// with the default ecoef = 1, s_j = 1 and the two agree.
// One launch per Linear and chunk (the layers are sequential by nature): the epilogue writes f(x_j), zero padded, as the next launch's
// B operand -- the scratch of mcpc_ce_prep_kernel, filled with the same act_f -- and the unpadded x_j where the caller wants it.  Padded
// units stay exactly zero (zero_padded4: the noise is masked there) and so do the rows of a partly live tile.
// The read-out launch writes o = f(x_{L-1}) W_L^T + b_L (bitwise pred_out) as
//   logits    o                                            sigmoid   bernoulli_mean(o) = sigmoid_f(o), the library's own
//   bernoulli (u < bernoulli_mean(o)) ? 1 : 0 with u = (r >> 8) 2^-24, r the raw Philox word of (seed, step, layer L, g, unit): the raw stream
//             of mcpc_philox_normals for layer L
//   gaussian  o + sd z_L, two roundings, sd = (float)sqrt(loss_var)
// No atomics, no sums: a value depends on (seed, step, g), the weights and the row's input alone -- not on the number of rows, the
// chunk, the split of [sample_base, sample_base + n) over calls, or the engine's form.
// Stores: as mcpc_pe_kernel's (pe_store4): 16-byte where the host found the destination fit for them, per element otherwise.
#pragma once

#include "mcpc_pred_err.h"

namespace mcpc {

enum : int { kSpLatent = 0, kSpLogits, kSpSigmoid, kSpBernoulli, kSpGaussian };     // what the epilogue of a launch makes of mu

struct SpParams {
    const float* fx_in;     // scratch: f(x_{j-1}) [chunk][npad_{j-1}]; unused for Linear 0
    float* fx_out;          // scratch: f(x_j)     [chunk][npad_j]; null where nothing reads it (the read-out, the last layer asked for)
    const void* Wf;         // forward fragments of Linear j >= 1
    const float* bias;      // padded bias of Linear j >= 1
    const float* mu1;       // Linear 0: mu_1 of the chunk's inputs [chunk][npad_0]
    const int* wexp;
    const LwJob* jobs;      // [gridDim.y]: the jobs of Linear j
    float* dst;             // the caller's destination of THIS chunk's first row, unpadded [rows][n], or null
    uint64_t seed, step;
    uint64_t g0;            // global id of the chunk's first row
    int kw;                 // padded width of the layer below (0 for Linear 0)
    int npad, n;            // padded and unpadded width of this layer
    int act;                // activation of this layer (latent launches)
    int rows;               // live rows of the chunk
    int mode;               // kSp*
    int vec;                // dst takes 16-byte stores
    float scale;            // s_j (latent), sd (gaussian)
};

// mu + s z in two roundings
__device__ __forceinline__ f32x4 sp_add_noise(f32x4 mu, float s, f32x4 z) {
#pragma clang fp contract(off)
    const f32x4 t = z * s;
    return mu + t;
}

__global__ __launch_bounds__(kLwThreads) void mcpc_sp_kernel(const SpParams R) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LwJob job = lw_load_job(R.jobs, blockIdx.y);
    const int j = job.layer;
    const int row0 = blockIdx.x * kLwChains;
    const int utw = job.ut0 + kLwUTW * wave;
    const int npad = R.npad, ntiles = npad / 16;
    int nt = ntiles - utw;
    nt = nt < 0 ? 0 : (nt > kLwUTW ? kLwUTW : nt);
    // the prediction: Linear j over f(x_{j-1}) (none for j == 0)
    f32x4 acc[kLwUTW][kLwCTT];
    const int kw = j > 0 ? R.kw : 0, nkb = (kw + kKB - 1) / kKB;
    lw_job_gemm(acc, j > 0 ? R.Wf : nullptr, nkb * kFragBlock, utw, ntiles, nkb, kw, j > 0 ? R.fx_in : nullptr, row0,
                j > 0 ? load_wexp(R.wexp, j) : 0, stage, sexp, tid, lane);
    const int c = lane & 15, q = lane >> 4;
    const int rows = R.rows, n = R.n, mode = R.mode, act = R.act;
    const float scale = R.scale;
    float* const dst = R.dst;
    float* const fxo = R.fx_out;
    const bool vec = R.vec != 0;
    const uint64_t seed = R.seed, step = R.step;
    f32x4 bias[kLwUTW];
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) bias[i] = (j > 0 && i < nt) ? ld4(R.bias + 16 * (utw + i) + 4 * q) : splat(0.f);
    // chain tile outermost: the two unit tiles of a row (adjacent in memory) are stored one after the other
#pragma unroll
    for (int ct = 0; ct < kLwCTT; ++ct) {
        const int row = row0 + 16 * ct + c;
        const bool live = row < rows;
        const uint32_t chain = (uint32_t)(R.g0 + (uint64_t)row);
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) {
            if (i >= nt) continue;
            const int u0 = 16 * (utw + i) + 4 * q;
            if (mode == kSpLatent) {
                const f32x4 mub = j > 0 ? bias[i] : ld4(R.mu1 + (size_t)row * npad + u0);
                const f32x4 mu = acc[i][ct] + mub;
                f32x4 x = splat(0.f);
                if (live) {
                    x = sp_add_noise(mu, scale, normals4(seed, step, (uint32_t)j, chain, (uint32_t)(u0 >> 2)));
                    zero_padded4(x, u0, n);
                    if (dst != nullptr) pe_store4(dst, row, n, u0, vec, x);
                }
                if (fxo != nullptr) {
                    f32x4 f;
                    f.x = act_f(act, x.x); f.y = act_f(act, x.y); f.z = act_f(act, x.z); f.w = act_f(act, x.w);
                    st4(fxo + (size_t)row * npad + u0, f);
                }
            } else if (live) {
                const f32x4 o = acc[i][ct] + bias[i];
                f32x4 v = o;
                if (mode == kSpSigmoid) {
                    v.x = bernoulli_mean(o.x); v.y = bernoulli_mean(o.y); v.z = bernoulli_mean(o.z); v.w = bernoulli_mean(o.w);
                } else if (mode == kSpBernoulli) {
                    uint32_t r[4];
                    philox4x32_10(chain, ((uint32_t)j << 24) | (uint32_t)(u0 >> 2), (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed,
                                  (uint32_t)(seed >> 32), r);
                    v.x = (float)(r[0] >> 8) * 0x1p-24f < bernoulli_mean(o.x) ? 1.f : 0.f;
                    v.y = (float)(r[1] >> 8) * 0x1p-24f < bernoulli_mean(o.y) ? 1.f : 0.f;
                    v.z = (float)(r[2] >> 8) * 0x1p-24f < bernoulli_mean(o.z) ? 1.f : 0.f;
                    v.w = (float)(r[3] >> 8) * 0x1p-24f < bernoulli_mean(o.w) ? 1.f : 0.f;
                } else if (mode == kSpGaussian) {
                    v = sp_add_noise(o, scale, normals4(seed, step, (uint32_t)j, chain, (uint32_t)(u0 >> 2)));
                }
                pe_store4(dst, row, n, u0, vec, v);
            }
        }
    }
}

}  // namespace mcpc
