// K1w  Layer-wise step kernels: networks too wide for the LDS plans of K1 / K1u.
//
// The state of ALL chains lives in global memory and one Langevin step is TWO launches over (Linear, chain tile, unit tile) output tiles:
//   mcpc_lw_fwd_kernel   every prediction of the step at once: mu_j = f(x_{j-1}) W_j^T + b_j as a tiled GEMM, epilogue e_j = c_j (x_j - mu_j)
//                        (read-out: output, loss, e_o = dloss/dout), energy partials, Hebbian spill, trajectory records; errors -> global memory.
//                        Linear 0's prediction is the constant mu_1 (mcpc_mu1_kernel): its tiles have no GEMM.
//   mcpc_lw_bwd_kernel   every x update at once: g_l = e_l - f'(x_l) (e_{l+1} W_{l+1}) as a tiled GEMM on the transposed fragments, epilogue = the
//                        x update with every optimiser and noise mode behind uniform branches, in place (an element of x_l is read and written by one thread only), and
//                        f(x_l) of the new state for the next forward launch.
// Given x_t all predictions are independent of each other, and given the errors all back-projections are: the two launch boundaries are the
// only synchronisation (no grid barrier, no spin-wait, no cooperative launch).
//
// The tile and its GEMM (lw_job_gemm) are the evaluators' too: mcpc_lw_tile.h.
#pragma once
#include "mcpc_kernels.h"
#include "mcpc_lw_tile.h"

namespace mcpc {

struct LwParams {
    KParams P;                     // what the LDS-resident kernels take: layers, read-out, optimiser, noise, records (LDS offsets unused)
    float* fx[kMaxLatent];         // f(x_l)   [Bpad][npad_l]: written by the backward launch, B operand of the forward launch
    float* err[kMaxLatent];        // e_l      [Bpad][npad_l], l >= 1: written by the forward launch, B operand of the backward launch
    float* err_o;                  // e_o      [Bpad][out_pad]
    const LwJob* jobs;             // [gridDim.y]
    int t;                         // step of the call
    int slot;                      // spill slot of this step (-1: the step does not accumulate)
    int rec_idx;                   // record index of this step (-1: not recorded)
    int do_energy, erow;           // energies of this step go to row erow of the partial table
};

// ---- forward epilogues: prediction errors and the read-out's loss error go to global memory ------------------------------------------------
template <int ACT>
__device__ __forceinline__ float lw_fwd_latent(const LwParams& Q, int l, int utw, int nt, int chain0, int lane, const f32x4 (&acc)[kLwUTW][kLwCTT],
                                               float& amx, float& emx) {
    const KParams& P = Q.P;
    const KLayer& Ly = P.layer[l];
    const int c = lane & 15, q = lane >> 4;
    const int npad = Ly.npad, n = Ly.n, B = P.B, Bpad = P.Bpad, slot = Q.slot;
    const float ecoef = Ly.ecoef;
    float* const eg = Q.err[l];
    float* const rec = (Q.rec_idx >= 0 && Ly.rec != nullptr) ? Ly.rec + (size_t)Q.rec_idx * B * n : nullptr;
    float esum = 0.f;
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) {
        if (i >= nt) continue;
        const int u0 = 16 * (utw + i) + 4 * q;
        // (l == 0: the prediction is the constant mu_1 row; l >= 1: GEMM + bias)
        const f32x4 bias = l > 0 ? ld4(Ly.bias + u0) : splat(0.f);
#pragma unroll
        for (int ct = 0; ct < kLwCTT; ++ct) {
            const int chain = chain0 + 16 * ct + c;
            const bool live = chain < B;
            const size_t row = (size_t)chain * npad + u0;
            const f32x4 x = ld4(Ly.x + row);
            const f32x4 mub = l > 0 ? bias : ld4(P.mu1 + row);
            f32x4 d;                                              // x - mu
            const f32x4 e = pc_error4(x, acc[i][ct] + mub, ecoef, d);
            if (l > 0) st4(eg + row, e);
            if (slot >= 0) {
                const f32x4 z = splat(0.f);
                const f32x4 fx = act4<ACT>(x);
                const size_t srow = (size_t)slot * Bpad + chain;
                st4s(Ly.spill_a + spill_offset(Ly.spill_a_tm, srow, u0, npad), live ? fx : z);
                amx = absmax4(amx, live ? fx : z);
                if (l > 0) {
                    st4s(Ly.spill_e + spill_offset(Ly.spill_e_tm, srow, u0, npad), live ? e : z);
                    emx = absmax4(emx, live ? e : z);
                } else if (live) {        // Linear 0 sees a constant input: only sum_t e_1 is needed
                    float* sp = Ly.spill_e + row;
                    st4(sp, ld4(sp) + e);
                }
            }
            if (rec != nullptr && live) st_unpadded(rec, chain, n, u0, x);
            esum += live ? pc_energy4(d, ecoef) : 0.0f;
        }
    }
    return esum;
}

__device__ __forceinline__ float lw_fwd_head(const LwParams& Q, int utw, int nt, int chain0, int lane, const f32x4 (&acc)[kLwUTW][kLwCTT], float& omx) {
    const KParams& P = Q.P;
    const KHead& H = P.head;
    const int c = lane & 15, q = lane >> 4;
    const int npad = H.npad, n = H.n, B = P.B, Bpad = P.Bpad, mask_start = H.mask_start, kind = H.loss_kind, slot = Q.slot;
    const float inv_var = H.inv_var;
    const bool do_energy = Q.do_energy != 0;
    float* const rec = (Q.rec_idx >= 0 && H.rec_out != nullptr) ? H.rec_out + (size_t)Q.rec_idx * B * n : nullptr;
    float lsum = 0.f;
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) {
        if (i >= nt) continue;
        const int u0 = 16 * (utw + i) + 4 * q;
        const f32x4 bias = ld4(H.bias + u0);
#pragma unroll
        for (int ct = 0; ct < kLwCTT; ++ct) {
            const int chain = chain0 + 16 * ct + c;
            const bool live = chain < B;
            const size_t row = (size_t)chain * npad + u0;
            const f32x4 o = acc[i][ct] + bias;
            f32x4 e = splat(0.f);
            if (kind != MCPC_LOSS_NONE) {
                const f32x4 y = ld4(H.y + row);
                MCPC_READOUT_LOSS4(e, o, y, kind, do_energy, inv_var, lsum, live && (u0 + r) >= mask_start && (u0 + r) < n, true);
            }
            st4(Q.err_o + row, e);
            if (slot >= 0) { st4s(H.spill_e + spill_offset(H.spill_tm, (size_t)slot * Bpad + chain, u0, npad), e); omx = absmax4(omx, e); }
            if (rec != nullptr && live) st_unpadded(rec, chain, n, u0, o);
        }
    }
    return lsum;
}

__global__ __launch_bounds__(kLwThreads) void mcpc_lw_fwd_kernel(const LwParams Q) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    __shared__ float sred[kLwWaves];
    __shared__ unsigned smax[2];
    const KParams& P = Q.P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LwJob job = lw_load_job(Q.jobs, blockIdx.y);
    const int j = job.layer, L = P.L;
    const bool head = j == L;
    const int chain0 = blockIdx.x * kLwChains;
    const int utw = job.ut0 + kLwUTW * wave;
    const int ntiles = head ? P.head.ntiles : P.layer[j].ntiles;
    int nt = ntiles - utw;
    nt = nt < 0 ? 0 : (nt > kLwUTW ? kLwUTW : nt);
    if (tid < 2) smax[tid] = 0u;
    // the GEMM: Linear j over f(x_{j-1}) (none for j == 0)
    f32x4 acc[kLwUTW][kLwCTT];
    const int kw = j > 0 ? P.layer[j - 1].npad : 0, nkb = (kw + kKB - 1) / kKB;
    const void* const A = j == 0 ? nullptr : (head ? (const void*)P.head.Wf : (const void*)P.layer[j].Wf);
    lw_job_gemm(acc, A, nkb * kFragBlock, utw, ntiles, nkb, kw, j > 0 ? Q.fx[j - 1] : nullptr, chain0, j > 0 ? load_wexp(P.wexp, j) : 0,
                stage, sexp, tid, lane);
    float esum = 0.f, mx0 = 0.f, mx1 = 0.f;
    if (head) {
        esum = lw_fwd_head(Q, utw, nt, chain0, lane, acc, mx1);
    } else {
        const int act = P.layer[j].act;
        if (act == MCPC_ACT_RELU) esum = lw_fwd_latent<MCPC_ACT_RELU>(Q, j, utw, nt, chain0, lane, acc, mx0, mx1);
        else if (act == MCPC_ACT_TANH) esum = lw_fwd_latent<MCPC_ACT_TANH>(Q, j, utw, nt, chain0, lane, acc, mx0, mx1);
        else esum = lw_fwd_latent<MCPC_ACT_IDENTITY>(Q, j, utw, nt, chain0, lane, acc, mx0, mx1);
    }
    const bool spills = Q.slot >= 0 && P.spillmax != nullptr;
    if (Q.do_energy) { esum = wave_sum(esum); if (lane == 0) sred[wave] = esum; }
    __syncthreads();                  // (smax is zero for every wave from here on; sred is complete behind the next barrier)
    if (spills) {
        mx0 = wave_max(mx0); mx1 = wave_max(mx1);
        if (lane == 0) { atomicMax(&smax[0], __float_as_uint(mx0)); atomicMax(&smax[1], __float_as_uint(mx1)); }
    }
    __syncthreads();
    if (tid == 0) {
        if (Q.do_energy) {
            // one slot per workgroup of this launch: its own Linear's column, zeros in the others (mcpc_energy_reduce_kernel sums the slots)
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < kLwWaves; ++w) v += (double)sred[w];
            const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x, nwg = (size_t)gridDim.x * gridDim.y;
            double* const o = P.epart + ((size_t)Q.erow * nwg + wg) * (kMaxLatent + 1);
            const int col = head ? kMaxLatent : j;
#pragma unroll
            for (int k = 0; k <= kMaxLatent; ++k) o[k] = k == col ? v : 0.0;
        }
        if (spills) {
            // order-free: integer maxima of bit patterns (non-negative floats order like them)
            if (head) { if (smax[1]) atomicMax(P.spillmax + kSpillIdEo, smax[1]); }
            else {
                if (smax[0]) atomicMax(P.spillmax + spill_id_a(j), smax[0]);
                if (j > 0 && smax[1]) atomicMax(P.spillmax + spill_id_e(j), smax[1]);
            }
        }
    }
}

// ---- backward epilogue: the x update on global rows (every optimiser and noise mode), f(x_new) for the next forward launch -------- -----------------------------
template <int ACT>
__device__ __forceinline__ void lw_bwd_update(const LwParams& Q, int l, float sign, int utw, int nt, int chain0, int lane,
                                              const f32x4 (&acc)[kLwUTW][kLwCTT]) {
    const KParams& P = Q.P;
    const KLayer& Ly = P.layer[l];
    const int c = lane & 15, q = lane >> 4;
    const int npad = Ly.npad, n = Ly.n, B = P.B;
    const float lr = P.lr, nscale = P.noise_scale, ecoef = Ly.ecoef;
    const uint64_t seed = P.seed, step = P.step_base + (uint64_t)Q.t, chain_base = P.chain_base;
    const float* const eg = Q.err[l];
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) {
        if (i >= nt) continue;
        const int u0 = 16 * (utw + i) + 4 * q;
#pragma unroll
        for (int ct = 0; ct < kLwCTT; ++ct) {
            const int chain = chain0 + 16 * ct + c;
            const bool live = chain < B;
            const size_t row = (size_t)chain * npad + u0;
            const f32x4 x = ld4(Ly.x + row), back = acc[i][ct];
            const f32x4 e = l > 0 ? ld4(eg + row) : (x - ld4(P.mu1 + row)) * ecoef;
            const f32x4 g = x_grad4<ACT>(x, e, back, sign);
            if (!P.update_x) {          // gradients only: x and f(x) stay
                if (live && Ly.xgrad != nullptr) st_unpadded(Ly.xgrad, chain, n, u0, g);
                continue;
            }
            f32x4 xn;
            if (P.xopt == MCPC_XOPT_SGD) {
                xn = x - g * lr;
            } else {
                const size_t mrow = tile_major_offset(chain, u0, npad);                    // (the moments are tile-major)
                f32x4 m = ld4s(Ly.m + mrow), v = ld4s(Ly.v + mrow);
                adam_moments4(m, v, g, P.omb1, P.beta2, P.omb2);
                st4s(Ly.m + mrow, m);
                st4s(Ly.v + mrow, v);
                xn = adam_x4(x, m, v, P.adam_coef[0], P.adam_coef[1], P.eps);              // (the host passes this step's pair)
            }
            if (P.noise_mode == MCPC_NOISE_PHILOX) {
                xn = xn + normals4(seed, step, (uint32_t)l, (uint32_t)(chain_base + (uint64_t)chain), (uint32_t)(u0 >> 2)) * nscale;
            } else if (P.noise_mode == MCPC_NOISE_EXTERNAL && live) {
                xn = xn + ld_unpadded(Ly.ext_noise, chain, n, u0) * nscale;                // (the host passes this step's image)
            }
            zero_padded4(xn, u0, n);
            st4(Ly.x + row, xn);
            st4(Q.fx[l] + row, act4<ACT>(xn));
        }
    }
}

__global__ __launch_bounds__(kLwThreads) void mcpc_lw_bwd_kernel(const LwParams Q) {
    __shared__ __attribute__((aligned(16))) float stage[kLwStageFloats];
    __shared__ int sexp[kLwChains];
    const KParams& P = Q.P;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LwJob job = lw_load_job(Q.jobs, blockIdx.y);
    const int l = job.layer, L = P.L;
    const int chain0 = blockIdx.x * kLwChains;
    const int utw = job.ut0 + kLwUTW * wave;
    const int ntiles = P.layer[l].ntiles;
    int nt = ntiles - utw;
    nt = nt < 0 ? 0 : (nt > kLwUTW ? kLwUTW : nt);
    // the back-projection: e_{l+1} W_{l+1} (the read-out's error for the last latent layer; none without a read-out)
    const bool last = l == L - 1;
    const bool has_gemm = !last || P.has_head;
    const int kw = !has_gemm ? 0 : (last ? P.head.npad : P.layer[l + 1].npad), nkb = (kw + kKB - 1) / kKB;
    const void* const A = !has_gemm ? nullptr : (last ? (const void*)P.head.Wb : (const void*)P.layer[l + 1].Wb);
    const float* const Bg = !has_gemm ? nullptr : (last ? Q.err_o : Q.err[l + 1]);
    const float sign = !has_gemm ? 0.0f : (last ? 1.0f : -1.0f);
    f32x4 acc[kLwUTW][kLwCTT];
    lw_job_gemm(acc, A, nkb * kFragBlock, utw, ntiles, nkb, kw, Bg, chain0, has_gemm ? load_wexp(P.wexp, l + 1) : 0, stage, sexp, tid, lane);
    const int act = P.layer[l].act;
    if (act == MCPC_ACT_RELU) lw_bwd_update<MCPC_ACT_RELU>(Q, l, sign, utw, nt, chain0, lane, acc);
    else if (act == MCPC_ACT_TANH) lw_bwd_update<MCPC_ACT_TANH>(Q, l, sign, utw, nt, chain0, lane, acc);
    else lw_bwd_update<MCPC_ACT_IDENTITY>(Q, l, sign, utw, nt, chain0, lane, acc);
}

// f(x_l) of the state a run starts from (mcpc_load_state may have replaced it since the last run): one launch per layer and run; from
// there on the backward launches keep it current
__global__ void mcpc_lw_act_kernel(const float* __restrict__ x, float* __restrict__ fx, size_t total4, int act) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total4; idx += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = ld4(x + 4 * idx);
        f32x4 f;
        f.x = act_f(act, v.x); f.y = act_f(act, v.y); f.z = act_f(act, v.z); f.w = act_f(act, v.w);
        st4(fx + 4 * idx, f);
    }
}

}  // namespace mcpc

