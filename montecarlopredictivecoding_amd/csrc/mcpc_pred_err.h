// Kpe  Prediction errors and predictions of recorded states, per unit (include/mcpc.h: mcpc_prediction_errors; DESIGN.md section Kpe).
//
// The evaluator of mcpc_chain_energy.h with another epilogue.  A ROW is one chain at one recorded step; for the rows' states x_1..x_L the
// kernel forms the predictions mu_j = f(x_{j-1}) W_j^T + b_j exactly as mcpc_ce_kernel does -- mcpc_ce_prep_kernel's scratch, mcpc_mu1_kernel
// for Linear 0, the tile of the layer-wise forward launch (4 waves, 64 rows x 128 units, lw_job_gemm as it is), pc_error4 /
// MCPC_READOUT_LOSS4 of mcpc_step_math.h -- so a prediction is bitwise the step kernels' and bitwise what mcpc_chain_energies squares.
// Instead of summing, every lane stores the four units it holds of each row:
//   err[l][row][u]  = x - mu     the d of pc_error4, NOT scaled by ecoef          pred[l][row][u] = mu
//   err_out[row][u] = e          the read-out error the step kernels propagate,   pred_out[row][u] = o   (the logits)
//                                exactly 0 outside [mask_start, n_out)
// DERIVED RECORDS: unpadded fp32 [rows][n_l], the layout mcpc_run writes rec_x[l] / rec_out in, so that every stateless reducer of the
// library (moments, covariance, histogram, autocovariance, rolling) takes them as it takes a record.
// No atomics, no sums: a value depends on its own row alone.  Nothing is stored for rows >= rows of a partly live tile or units >= n_l.
// Stores: in the MFMA C layout a lane holds units 16 t + 4 q .. + 3 of row c (c = lane & 15, q = lane >> 4), so one store instruction
// writes 16 rows x 64 contiguous bytes; the wave's two unit tiles of a row are adjacent (128 B) and are stored back to back.  Rows are
// only 4-byte aligned in general: 16-byte stores where n_l % 4 == 0 and the base is 16-byte aligned (decided on the host, per
// destination), per-element predicated stores otherwise.
#pragma once

#include <vector>

#include "mcpc_chain_energy.h"

namespace mcpc {

struct PeParams {
    CeParams ce;                        // the evaluator's operands (part / job0 unused)
    float* err[kMaxLatent + 1];         // destinations of THIS chunk's first row, or null; [L] = the read-out
    float* pred[kMaxLatent + 1];
    int n[kMaxLatent + 1];              // unpadded widths; [L] = n_out
    unsigned vec_err, vec_pred;         // bit j: destination j takes 16-byte stores
};

// the four units u0 .. u0 + 3 of `row` of an unpadded [rows][n] tensor
__device__ __forceinline__ void pe_store4(float* base, int row, int n, int u0, bool vec, f32x4 v) {
    if (vec) {
        if (u0 < n) st4(base + (size_t)row * n + u0, v);       // n % 4 == 0: the quad is inside the row or beyond it
    } else {
        st_unpadded(base, row, n, u0, v);
    }
}

__global__ __launch_bounds__(kLwThreads) void mcpc_pe_kernel(const PeParams R) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    const CeParams& Q = R.ce;
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
    const int B = Q.B, rows = Q.rows, n = R.n[j];
    float* const eg = R.err[j];
    float* const pg = R.pred[j];
    const bool evec = (R.vec_err >> j) & 1u, pvec = (R.vec_pred >> j) & 1u;
    f32x4 bias[kLwUTW];
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) bias[i] = (j > 0 && i < nt) ? ld4(Q.bias[j] + 16 * (utw + i) + 4 * q) : splat(0.f);
    // chain tile outermost: the two unit tiles of a row (adjacent in memory) are stored one after the other
#pragma unroll
    for (int ct = 0; ct < kLwCTT; ++ct) {
        const int row = row0 + 16 * ct + c;
        const bool live = row < rows;
        const int chain = live ? (Q.row_base + row) % B : 0;
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) {
            if (i >= nt) continue;
            const int u0 = 16 * (utw + i) + 4 * q;
            if (head) {
                const f32x4 o = acc[i][ct] + bias[i];
                if (pg != nullptr && live) pe_store4(pg, row, n, u0, pvec, o);
                if (eg != nullptr) {
                    const int mask_start = Q.mask_start, kind = Q.loss_kind;
                    const float inv_var = Q.inv_var;
                    const f32x4 y = ld4(Q.y + (size_t)chain * npad + u0);
                    float lsum = 0.f;
                    f32x4 e;
                    MCPC_READOUT_LOSS4(e, o, y, kind, false, inv_var, lsum, live && (u0 + r) >= mask_start && (u0 + r) < n, true);
                    (void)lsum;
                    if (live) pe_store4(eg, row, n, u0, evec, e);
                }
            } else {
                const f32x4 x = ld4(Q.x[j] + (size_t)row * npad + u0);
                const f32x4 mub = j > 0 ? bias[i] : ld4(Q.mu1 + (size_t)chain * npad + u0);
                const f32x4 mu = acc[i][ct] + mub;
                f32x4 d;
                (void)pc_error4(x, mu, Q.ecoef[j], d);
                if (live) {
                    if (eg != nullptr) pe_store4(eg, row, n, u0, evec, d);
                    if (pg != nullptr) pe_store4(pg, row, n, u0, pvec, mu);
                }
            }
        }
    }
}

// The job table (host): ce_job_table's jobs of the Linears marked in `want` (bit j; bit L = the read-out), in that table's order.
inline void pe_job_table(const std::vector<LwJob>& all, unsigned want, std::vector<LwJob>& jobs) {
    jobs.clear();
    for (const LwJob& jb : all)
        if ((want >> jb.layer) & 1u) jobs.push_back(jb);
}

// the latent layers whose recorded state the wanted Linears read (bit l): Linear j reads x_j (its own state, j < L) and f(x_{j-1})
inline unsigned pe_layers_read(unsigned want, int L) {
    unsigned need = 0;
    for (int j = 0; j <= L; ++j) {
        if (!((want >> j) & 1u)) continue;
        if (j < L) need |= 1u << j;
        if (j > 0) need |= 1u << (j - 1);
    }
    return need;
}

}  // namespace mcpc
