// Kce  Per-chain energies of recorded states (include/mcpc.h: mcpc_chain_energies; DESIGN.md section Kce).
//
// A ROW is one chain at one recorded step.  For R rows with states x_1..x_L the evaluator forms every prediction
// mu_j = f(x_{j-1}) W_j^T + b_j (Linear 0: the constant mu_1 of the row's chain) and writes, per row, the read-out loss, the layer
// energies E_1..E_L and their sum `overall` -- what the step kernels add up over the chains of a step, kept apart per chain.
//
//   mcpc_ce_prep_kernel    a chunk of unpadded records [rows][n_l] -> padded x and f(x) rows [chunk][npad_l] in the evaluator's own scratch
//   mcpc_ce_kernel         grid (chunk / 64, jobs): the tile of the layer-wise forward launch -- 4 waves, 64 rows x 128 units, lw_job_gemm as
//                          it is, so a prediction is bitwise the step kernels' -- with an epilogue that keeps one fp32 sum PER CHAIN TILE and
//                          lane (the four units a lane holds of one row in the MFMA C layout, over the wave's unit tiles), then fp64: the four
//                          lanes of a row, the waves of the workgroup through LDS, one partial per (job, row)
//   mcpc_ce_finish_kernel  one thread per row: the jobs of a layer in ascending order, the layers in ascending order, the loss last
// No atomics; every sum has one fixed order in which only the row's own values appear: a row's result does not depend on its neighbours
// in the tile, on the number of rows or on how the caller chunks them.
// The per-element arithmetic is pc_error4 / pc_energy4 / MCPC_READOUT_LOSS4 of mcpc_step_math.h.
#pragma once
#include "mcpc_step_math.h"
#include "mcpc_lw_tile.h"       // the layer-wise forward tile (lw_job_gemm)

namespace mcpc {

constexpr int kCeDefaultRows = 16384;               // rows per scratch chunk when the caller leaves it to the library

struct CeParams {
    const float* x[kMaxLatent];         // scratch: x_l     [chunk][npad_l]
    const float* fx[kMaxLatent];        // scratch: f(x_l)  [chunk][npad_l]
    const void* Wf[kMaxLatent + 1];     // forward fragments of Linear j >= 1 (mcpc_pack_kernel)
    const float* bias[kMaxLatent + 1];  // padded bias of Linear j >= 1
    int npad[kMaxLatent + 1];           // padded widths; [L] = the read-out
    float ecoef[kMaxLatent];
    const float* mu1;                   // [B][npad_0], from the inputs of this call
    const float* y;                     // the bound target, padded [Bpad][npad_L]
    const int* wexp;
    const LwJob* jobs;                  // [gridDim.y]
    double* part;                       // [job][chunk]
    int job0;                           // index of jobs[0] in the whole table (= its row block of `part`)
    int L, B, n_out;
    int rows, chunk;                    // live rows of this chunk, padded rows (a multiple of kLwChains)
    int row_base;                       // index of the chunk's first row among all rows of the call (row -> chain: modulo B)
    int loss_kind, mask_start;
    float inv_var;
};

// layer l of rows [row0, row0 + rows) of the records -> rows 0 .. of the scratch, zero padded (f(0) = 0 for every activation)
__global__ __launch_bounds__(256) void mcpc_ce_prep_kernel(const float* __restrict__ rec, float* __restrict__ x, float* __restrict__ fx, int rows,
                                                           int chunk, int n, int npad, int act) {
    const size_t total4 = (size_t)chunk * (npad / 4);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total4; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / (npad / 4)), u0 = 4 * (int)(idx % (npad / 4));
        f32x4 v = splat(0.f);
        if (row < rows) v = ld_unpadded(rec, row, n, u0);
        f32x4 f;
        f.x = act_f(act, v.x); f.y = act_f(act, v.y); f.z = act_f(act, v.z); f.w = act_f(act, v.w);
        st4(x + 4 * idx, v);
        st4(fx + 4 * idx, f);
    }
}

__global__ __launch_bounds__(kLwThreads) void mcpc_ce_kernel(const CeParams Q) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    __shared__ double sred[kLwWaves][kLwChains];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LwJob job = lw_load_job(Q.jobs, blockIdx.y);
    const int j = job.layer, L = Q.L;
    const bool head = j == L;
    const int row0 = blockIdx.x * kLwChains;
    const int utw = job.ut0 + kLwUTW * wave;
    const int npad = Q.npad[j], ntiles = npad / 16;
    int nt = ntiles - utw;
    nt = nt < 0 ? 0 : (nt > kLwUTW ? kLwUTW : nt);
    // the prediction: Linear j over f(x_{j-1}) (none for j == 0)
    f32x4 acc[kLwUTW][kLwCTT];
    const int kw = j > 0 ? Q.npad[j - 1] : 0, nkb = (kw + kKB - 1) / kKB;
    lw_job_gemm(acc, j > 0 ? Q.Wf[j] : nullptr, nkb * kFragBlock, utw, ntiles, nkb, kw, j > 0 ? Q.fx[j - 1] : nullptr, row0,
                j > 0 ? load_wexp(Q.wexp, j) : 0, stage, sexp, tid, lane);
    const int c = lane & 15, q = lane >> 4;
    const int B = Q.B, rows = Q.rows;
    float sum[kLwCTT];                          // one per chain tile: the lane's four units of ONE row, over the wave's unit tiles
#pragma unroll
    for (int ct = 0; ct < kLwCTT; ++ct) sum[ct] = 0.f;
    if (head) {
        const int n = Q.n_out, mask_start = Q.mask_start, kind = Q.loss_kind;
        const float inv_var = Q.inv_var;
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) {
            if (i >= nt) continue;
            const int u0 = 16 * (utw + i) + 4 * q;
            const f32x4 bias = ld4(Q.bias[j] + u0);
#pragma unroll
            for (int ct = 0; ct < kLwCTT; ++ct) {
                const int row = row0 + 16 * ct + c;
                const bool live = row < rows;
                const int chain = live ? (Q.row_base + row) % B : 0;
                const f32x4 o = acc[i][ct] + bias;
                const f32x4 y = ld4(Q.y + (size_t)chain * npad + u0);
                f32x4 e;
                MCPC_READOUT_LOSS4(e, o, y, kind, true, inv_var, sum[ct], live && (u0 + r) >= mask_start && (u0 + r) < n, true);
                (void)e;
            }
        }
    } else {
        const float ecoef = Q.ecoef[j];
        const float* const xg = Q.x[j];
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) {
            if (i >= nt) continue;
            const int u0 = 16 * (utw + i) + 4 * q;
            const f32x4 bias = j > 0 ? ld4(Q.bias[j] + u0) : splat(0.f);
#pragma unroll
            for (int ct = 0; ct < kLwCTT; ++ct) {
                const int row = row0 + 16 * ct + c;
                const bool live = row < rows;
                const int chain = live ? (Q.row_base + row) % B : 0;
                const f32x4 x = ld4(xg + (size_t)row * npad + u0);
                const f32x4 mub = j > 0 ? bias : ld4(Q.mu1 + (size_t)chain * npad + u0);
                f32x4 d;
                (void)pc_error4(x, acc[i][ct] + mub, ecoef, d);
                sum[ct] += live ? pc_energy4(d, ecoef) : 0.0f;
            }
        }
    }
    // fp64 from here: the four lanes of a row (q = 0..3 hold its units 4q .. 4q + 3 of every tile), then the waves, ascending
#pragma unroll
    for (int ct = 0; ct < kLwCTT; ++ct) {
        double v = (double)sum[ct];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (q == 0) sred[wave][16 * ct + c] = v;
    }
    __syncthreads();
    if (tid < kLwChains) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kLwWaves; ++w) v += sred[w][tid];
        Q.part[(size_t)(Q.job0 + blockIdx.y) * Q.chunk + row0 + tid] = v;
    }
}

// (CeFinish -- the jobs of Linear j in the table, contiguous and ascending -- is kept by the engine: mcpc_types.h)
// out[row_base + row][:] = {loss, E_1..E_L, 0.., overall}
__global__ __launch_bounds__(256) void mcpc_ce_finish_kernel(const double* __restrict__ part, double* __restrict__ out, const CeFinish F, int L,
                                                             int with_loss, int rows, int chunk, size_t row_base) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    double* const o = out + (row_base + row) * kEnergyCols;
    double overall = 0.0;
#pragma unroll
    for (int l = 0; l < kMaxLatent; ++l) {
        double v = 0.0;
        if (l < L)
            for (int k = 0; k < F.count[l]; ++k) v += part[(size_t)(F.first[l] + k) * chunk + row];
        o[1 + l] = v;
        overall += v;
    }
    double loss = 0.0;
    if (with_loss)
        for (int k = 0; k < F.count[L]; ++k) loss += part[(size_t)(F.first[L] + k) * chunk + row];
    o[0] = loss;
    o[kEnergyCols - 1] = overall + loss;
}

// (the job table, ce_job_table, is built on the host: mcpc_plan.h)

}  // namespace mcpc
