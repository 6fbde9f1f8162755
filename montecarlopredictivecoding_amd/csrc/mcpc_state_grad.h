// Ksg  Gradient of the free energy, and the energies, of handed-over states (include/mcpc.h: mcpc_state_gradients; DESIGN.md section Ksg).
//
// A ROW is one chain at one handed-over state, as in mcpc_chain_energy.h: x[l] is [n_rec][B][n_l] fp32, unpadded, the row's chain is
// row mod B.  For every row the pair of tile launches is one layer-wise step with update_x = 0 (mcpc_steps_lw.h) on the CALLER's tensors:
// nothing of the engine's state, Adam moments, Philox position or records is read or written.
//
//   mcpc_grad_prep_kernel  ONE launch per chunk for all layers: unpadded rows [rows][n_l] -> padded x and f(x) rows [chunk][npad_l] in the
//                          evaluators' scratch (what mcpc_ce_prep_kernel does per layer, over a by-value table of the layers)
//   mcpc_grad_fwd_kernel   grid (chunk / 64, jobs of ce_job_table: the read-out first): the forward tile of the layer-wise launch,
//                          lw_job_gemm as it is; epilogue pc_error4 / MCPC_READOUT_LOSS4, e_l (l >= 1) and e_o stored as padded rows in
//                          the evaluators' error scratch.  When the energies are asked for, the per-(job, row) fp64 partials of
//                          mcpc_ce_kernel, sum for sum: mcpc_ce_finish_kernel serves unchanged
//   mcpc_grad_bwd_kernel   grid (chunk / 64, backward jobs of lw_job_table): the back-projection e_{l+1} W_{l+1} on the Wb fragments,
//                          g = x_grad4(x, e, back, sign), stored unpadded to the caller's grad[l]
// No atomics; no sum that holds another row's value; nothing is stored for rows >= rows or units >= n_l.  Stores to the caller follow
// Kpe's rule (pe_store4): 16-byte stores where n_l % 4 == 0 and the destination is 16-byte aligned, decided on the host per destination.
#pragma once
#include "mcpc_pred_err.h"      // CeParams, the tile, pe_store4

namespace mcpc {

struct SgPrep {
    const float* rec[kMaxLatent];       // the chunk's first row of the caller's x[l]
    float* x[kMaxLatent];               // scratch: x_l     [chunk][npad_l]
    float* fx[kMaxLatent];              // scratch: f(x_l)  [chunk][npad_l]
    unsigned end4[kMaxLatent];          // quads of layers 0 .. l of this launch (a running total: layer l owns [end4[l-1], end4[l]))
    int n[kMaxLatent], npad[kMaxLatent], act[kMaxLatent];
    int L, rows;
};

struct SgParams {
    CeParams ce;                        // the evaluators' operands; ce.part == nullptr: no energies
    const void* Wb[kMaxLatent + 1];     // backward fragments of Linear j >= 1 (mcpc_pack_kernel)
    float* err[kMaxLatent];             // scratch: e_l, l >= 1  [chunk][npad_l]
    float* err_o;                       // scratch: e_o          [chunk][out_pad]
    float* grad[kMaxLatent];            // destinations of THIS chunk's first row
    const LwJob* bjobs;                 // [gridDim.y] of the backward launch
    int n[kMaxLatent], act[kMaxLatent];
    unsigned vec_grad;                  // bit l: grad[l] takes 16-byte stores
    int has_head;
};

__global__ __launch_bounds__(256) void mcpc_grad_prep_kernel(const SgPrep T) {
    const unsigned total4 = T.end4[T.L - 1];
    for (unsigned idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total4; idx += gridDim.x * blockDim.x) {
        int l = 0;
#pragma unroll
        for (int k = 0; k < kMaxLatent - 1; ++k) l += (k < T.L - 1 && idx >= T.end4[k]) ? 1 : 0;
        const unsigned loc = idx - (l > 0 ? T.end4[l - 1] : 0u);
        const int q = T.npad[l] / 4;
        const int row = (int)(loc / q), u0 = 4 * (int)(loc % q);
        const int act = T.act[l];
        f32x4 v = splat(0.f);
        if (row < T.rows) v = ld_unpadded(T.rec[l], row, T.n[l], u0);
        f32x4 f;
        f.x = act_f(act, v.x); f.y = act_f(act, v.y); f.z = act_f(act, v.z); f.w = act_f(act, v.w);
        st4(T.x[l] + 4 * (size_t)loc, v);
        st4(T.fx[l] + 4 * (size_t)loc, f);
    }
}

__global__ __launch_bounds__(kLwThreads) void mcpc_grad_fwd_kernel(const SgParams R) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    __shared__ double sred[kLwWaves][kLwChains];
    const CeParams& Q = R.ce;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LwJob job = lw_load_job(Q.jobs, blockIdx.y);
    const int j = job.layer, L = Q.L;
    const bool head = j == L;
    const int kind = Q.loss_kind;
    const bool do_energy = Q.part != nullptr;
    const int row0 = blockIdx.x * kLwChains;
    const int utw = job.ut0 + kLwUTW * wave;
    const int npad = Q.npad[j], ntiles = npad / 16;
    int nt = ntiles - utw;
    nt = nt < 0 ? 0 : (nt > kLwUTW ? kLwUTW : nt);
    // the prediction: Linear j over f(x_{j-1}) (none for j == 0, none for a read-out without a loss: its error is zero)
    f32x4 acc[kLwUTW][kLwCTT];
    const bool gemm = j > 0 && !(head && kind == MCPC_LOSS_NONE);
    const int kw = gemm ? Q.npad[j - 1] : 0, nkb = (kw + kKB - 1) / kKB;
    lw_job_gemm(acc, gemm ? Q.Wf[j] : nullptr, nkb * kFragBlock, utw, ntiles, nkb, kw, gemm ? Q.fx[j - 1] : nullptr, row0,
                gemm ? load_wexp(Q.wexp, j) : 0, stage, sexp, tid, lane);
    const int c = lane & 15, q = lane >> 4;
    const int B = Q.B, rows = Q.rows;
    float sum[kLwCTT];                          // one per chain tile: the lane's four units of ONE row, over the wave's unit tiles
#pragma unroll
    for (int ct = 0; ct < kLwCTT; ++ct) sum[ct] = 0.f;
    if (head) {
        const int n = Q.n_out, mask_start = Q.mask_start;
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
                f32x4 e = splat(0.f);
                if (kind != MCPC_LOSS_NONE) {
                    const f32x4 y = ld4(Q.y + (size_t)chain * npad + u0);
                    MCPC_READOUT_LOSS4(e, o, y, kind, do_energy, inv_var, sum[ct], live && (u0 + r) >= mask_start && (u0 + r) < n, true);
                }
                st4(R.err_o + (size_t)row * npad + u0, e);
            }
        }
    } else {
        const float ecoef = Q.ecoef[j];
        const float* const xg = Q.x[j];
        float* const eg = R.err[j];
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
                const f32x4 e = pc_error4(x, acc[i][ct] + mub, ecoef, d);
                if (j > 0) st4(eg + (size_t)row * npad + u0, e);
                sum[ct] += live ? pc_energy4(d, ecoef) : 0.0f;
            }
        }
    }
    if (!do_energy) return;                     // (uniform: no barrier is left behind)
    // fp64 from here, as mcpc_ce_kernel: the four lanes of a row, then the waves, ascending
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

template <int ACT>
__device__ __forceinline__ void sg_bwd_store(const SgParams& R, int l, float sign, int utw, int nt, int row0, int lane,
                                             const f32x4 (&acc)[kLwUTW][kLwCTT]) {
    const CeParams& Q = R.ce;
    const int c = lane & 15, q = lane >> 4;
    const int npad = Q.npad[l], n = R.n[l], B = Q.B, rows = Q.rows;
    const float ecoef = Q.ecoef[l];
    const float* const xg = Q.x[l];
    const float* const eg = R.err[l];
    float* const gg = R.grad[l];
    const bool vec = (R.vec_grad >> l) & 1u;
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
            const size_t at = (size_t)row * npad + u0;
            const f32x4 x = ld4(xg + at), back = acc[i][ct];
            const f32x4 e = l > 0 ? ld4(eg + at) : (x - ld4(Q.mu1 + (size_t)chain * npad + u0)) * ecoef;
            const f32x4 g = x_grad4<ACT>(x, e, back, sign);
            if (live) pe_store4(gg, row, n, u0, vec, g);
        }
    }
}

__global__ __launch_bounds__(kLwThreads) void mcpc_grad_bwd_kernel(const SgParams R) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    const CeParams& Q = R.ce;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LwJob job = lw_load_job(R.bjobs, blockIdx.y);
    const int l = job.layer, L = Q.L;
    const int row0 = blockIdx.x * kLwChains;
    const int utw = job.ut0 + kLwUTW * wave;
    const int ntiles = Q.npad[l] / 16;
    int nt = ntiles - utw;
    nt = nt < 0 ? 0 : (nt > kLwUTW ? kLwUTW : nt);
    // the back-projection: e_{l+1} W_{l+1} (the read-out's error for the last latent layer; none without a read-out)
    const bool last = l == L - 1;
    const bool has_gemm = !last || R.has_head;
    const int kw = has_gemm ? Q.npad[l + 1] : 0, nkb = (kw + kKB - 1) / kKB;
    const void* const A = has_gemm ? R.Wb[l + 1] : nullptr;
    const float* const Bg = !has_gemm ? nullptr : (last ? R.err_o : R.err[l + 1]);
    const float sign = !has_gemm ? 0.0f : (last ? 1.0f : -1.0f);
    f32x4 acc[kLwUTW][kLwCTT];
    lw_job_gemm(acc, A, nkb * kFragBlock, utw, ntiles, nkb, kw, Bg, row0, has_gemm ? load_wexp(Q.wexp, l + 1) : 0, stage, sexp, tid, lane);
    const int act = R.act[l];
    if (act == MCPC_ACT_RELU) sg_bwd_store<MCPC_ACT_RELU>(R, l, sign, utw, nt, row0, lane, acc);
    else if (act == MCPC_ACT_TANH) sg_bwd_store<MCPC_ACT_TANH>(R, l, sign, utw, nt, row0, lane, acc);
    else sg_bwd_store<MCPC_ACT_IDENTITY>(R, l, sign, utw, nt, row0, lane, acc);
}

// ---- host: the sizes of the error scratch and the prep launch's table (plain functions: no device work) -----------------------------------
// floats of the error rows e_l (l >= 1; [L]: the read-out's, 0 without one) for chunks of `chunk` rows
inline void sg_err_floats(int L, const int* npad, int out_pad, int chunk, size_t (&floats)[kMaxLatent + 1]) {
    for (int l = 0; l <= kMaxLatent; ++l) floats[l] = 0;
    for (int l = 1; l < L; ++l) floats[l] = (size_t)chunk * npad[l];
    floats[kMaxLatent] = (size_t)chunk * out_pad;
}
// the running quad totals of a chunk of `padded` rows; false when they pass 32 bits (the chunk is then prepared layer by layer)
inline bool sg_prep_ends(int L, const int* npad, int padded, unsigned (&end4)[kMaxLatent]) {
    unsigned long long t = 0;
    for (int l = 0; l < kMaxLatent; ++l) {
        if (l < L) t += (unsigned long long)padded * (npad[l] / 4);
        end4[l] = (unsigned)t;
    }
    return t < (1ull << 32);
}

}  // namespace mcpc
