// K1  mcpc_steps_kernel   fused Langevin / PC inference steps, persistent over n_steps, in the first form: every wave runs GEMM and
//                         epilogue of its tiles, a workgroup barrier closes a table entry.
//                         one workgroup = 16 chains (one MFMA column tile), all layers, weights streamed from L2 in
//                         MFMA-fragment order, state in HBM/L2 (padded), activations/errors in LDS.
//                         replaces reference pc_trainer.py:733-918 + utils/model.py:35-44 per step.
// The fallback of the in-place kernel (mcpc_steps_ws2.h) where no in-place plan fits; instantiated and launched by mcpc_steps_lw.hip.
#pragma once
#include "mcpc_kernels.h"

namespace mcpc {

#ifndef MCPC_BARRIER_WAVES_PER_EU
#define MCPC_BARRIER_WAVES_PER_EU 1      // one workgroup per CU, no spilled VGPRs (256 + 112 AGPRs): 129 us per step at cfg-M; 2 (two workgroups
                                         // per CU, one's GEMMs covering the other's epilogues, 72 VGPRs spilled to scratch): 147 us (round 4)
#endif
template <int CTT, int NW>       // CTT: part of the symbol, always 1 (one MFMA column tile of 16 chains); handed on only to the epilogues that still take it
__global__ __launch_bounds__(NW * 64, MCPC_BARRIER_WAVES_PER_EU) void mcpc_steps_kernel(const KParams P) {
    static_assert(CTT == 1, "part of the symbol: one chain tile per workgroup");
    constexpr int NTW = 16 / NW;     // unit tiles per wave per phase (a phase hands out 16 tiles)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chain0 = blockIdx.x * 16;
    const int L = P.L;
    // fused fast paths of the x update (wave-uniform, fixed for the launch)
    const int upd_mode = (P.update_x && P.xopt == MCPC_XOPT_SGD)
                             ? (P.noise_mode == MCPC_NOISE_PHILOX ? 2 : (P.noise_mode == MCPC_NOISE_NONE ? 1 : 0)) : 0;
    const bool y_bounded = P.has_head && *P.head.y_bounded != 0;      // (headb_fixed_exp)
    // every float of the plan starts a launch as zero (row tails and padding columns are never written afterwards)
    for (int i = tid; i < P.lds_floats / 4; i += NW * 64) st4(lds + 4 * i, splat(0.f));
    __syncthreads();
    if (P.stagger_cycles > 0 && blockIdx.x >= 256) {
        // two workgroups share a CU: start the second one out of phase so that its GEMMs overlap the
        // first one's epilogues / barriers instead of competing for the matrix pipe in lockstep
        const unsigned long long t_end = __builtin_amdgcn_s_memtime() + (unsigned long long)P.stagger_cycles;
        while (__builtin_amdgcn_s_memtime() < t_end) __builtin_amdgcn_s_sleep(32);
    }
    STAMP_DECL
    // software pipeline over phases: descriptor + first two weight k-blocks of the upcoming phase
    KPhase ph_next = load_phase(P.phases, 0);
    int nt_next, aoff_next[NTW];
    frag_t pre0_next[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) pre0_next[i] = frag_zero();
    prefetch_first_blocks<NW, NTW>(ph_next, wave, lane, nt_next, aoff_next, pre0_next);

    for (int s = 0; s < P.n_steps; ++s) {
        const int t = P.t0 + s;
        const bool do_energy = (P.energy_mode == MCPC_ENERGY_ALL) ||
                               (P.energy_mode == MCPC_ENERGY_LAST && t == P.T - 1);
        const int slot = (t >= P.acc_begin && t < P.acc_end) ? (t - P.spill_t0) : -1;
        int rec_idx = -1;
        if (P.rec_count > 0 && t >= P.rec_begin) {
            const int k = (t - P.rec_begin) / P.rec_stride;
            if (k < P.rec_count && P.rec_begin + k * P.rec_stride == t) rec_idx = k;
        }
        // per-wave energy partials of this step; two copies alternate so that a wave running ahead
        // into the next step never touches slots a slower wave is still reading
        float* red = lds + P.lds_red + (s & 1) * (kMaxLatent + 1) * NW;
        if (do_energy && lane <= kMaxLatent) red[lane * NW + wave] = 0.f;

        f32x4 accb[NTW];
#pragma unroll
        for (int i = 0; i < NTW; ++i) accb[i] = splat(0.f);
        int accb_run = kRunNone, accb_aexp = 0;            // the units accb is in (mcpc_gemm_f16.h: GemmScale)

#pragma unroll 1
        for (int p = 0; p < P.n_phases; ++p) {
            const KPhase ph = ph_next;
            const int nt = nt_next;
            int aoff[NTW];
            frag_t pre0[NTW];
#pragma unroll
            for (int i = 0; i < NTW; ++i) { aoff[i] = aoff_next[i]; pre0[i] = pre0_next[i]; }
            // descriptor of the phase after this one (wraps into the next step)
            const bool has_next = (p + 1 < P.n_phases) || (s + 1 < P.n_steps);
            if (has_next) ph_next = load_phase(P.phases, p + 1 < P.n_phases ? p + 1 : 0);
            if (ph.type == PH_ENERGY) {
                if (do_energy) {
                    __syncthreads();   // uniform branch: publishes every wave's red[] entries of this step
                    if (tid <= kMaxLatent) {
                        double v = 0.0;
                        const bool used = (tid < L) || (tid == kMaxLatent && P.has_head);
                        if (used) {
#pragma unroll
                            for (int w = 0; w < NW; ++w) v += (double)red[tid * NW + w];
                        }
                        const int erow = (P.energy_mode == MCPC_ENERGY_ALL) ? t : 0;
                        P.epart[((size_t)erow * gridDim.x + blockIdx.x) * (kMaxLatent + 1) + tid] = v;
                    }
                }
                if (has_next) prefetch_first_blocks<NW, NTW>(ph_next, wave, lane, nt_next, aoff_next, pre0_next);
                STAMP(12);
                continue;
            }
            f32x4 acc[NTW], pa[NTW], pb[NTW];
            const KLayer& Ly = P.layer[ph.layer];
            // ---- accumulators; the epilogue's operands are requested by `prologue`, which the GEMM
            //      invokes after its last fragment load (or which runs directly when there is no GEMM)
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                acc[i] = (ph.flags & PHF_ACC_FROM_B) ? accb[i] : splat(0.f);
                pa[i] = splat(0.f); pb[i] = splat(0.f);
            }
            STAMP_T(0, ph.type);
            // ---- GEMM ------------------------------------------------------------------------------------
            // operands of the epilogue (x, targets: streamed; bias, E: L2/LDS) are requested ahead of the GEMM.
            // (Requesting them after the GEMM's last fragment load was measured slower on MI355X.)
            if (ph.type != PH_HEADB) issue_epilogue_loads<CTT, NW, NTW>(P, ph, lds, nt, wave, lane, chain0, pa, pb);
            if (nt > 0 && ph.nkb > 0) {
                // HEADB phases add up in accb over the chunks of the read-out, in scaled units (accb_run / accb_aexp); every other GEMM is fresh
                const int hb_exp = ph.type == PH_HEADB ? headb_fixed_exp(P.head.loss_kind, y_bounded) : kScaleAuto;
                GemmScale gs{load_wexp(P.wexp, ph.a_lin), ph.type == PH_HEADB ? GS_ACCUM : GS_FRESH, hb_exp, accb_run,
                             ph.type == PH_HEADB ? (P.head.npad <= kShortK * kKB ? 1 : 0) : -1, hb_exp == kScaleAuto ? 1 : 0};
                gemm_tiles<NTW, NW>(acc, ph.A, aoff, nt, ph.nkb, ph.kw, lds + ph.b_lds, ph.ldb, lane, pre0, lds + P.lds_zero, gs);
                if (ph.type == PH_HEADB) { accb_run = gs.run; accb_aexp = gs.a_exp; }
            } else if ((ph.flags & PHF_ACC_FROM_B) && ph.type != PH_HEADB && accb_run != kRunNone) {
                gemm_unscale<NTW>(acc, accb_aexp, accb_run);       // the complete back-projection of the read-out error, handed to BWD_{L-1}
            }
            // the next phase's first weight fragments travel while this phase's epilogue runs
            if (has_next) prefetch_first_blocks<NW, NTW>(ph_next, wave, lane, nt_next, aoff_next, pre0_next);
            if (ph.flags & PHF_ACC_TO_B) {
#pragma unroll
                for (int i = 0; i < NTW; ++i) accb[i] = acc[i];
            }
            STAMP_T(1, ph.type);
            // ---- epilogue --------------------------------------------------------------------------------
            if (ph.type == PH_FWD) {
                float esum;
                if (Ly.act == MCPC_ACT_RELU) esum = fwd_epilogue<CTT, NW, NTW, MCPC_ACT_RELU>(P, ph, lds, nt, wave, lane, chain0, acc, pa, pb, slot, rec_idx);
                else if (Ly.act == MCPC_ACT_TANH) esum = fwd_epilogue<CTT, NW, NTW, MCPC_ACT_TANH>(P, ph, lds, nt, wave, lane, chain0, acc, pa, pb, slot, rec_idx);
                else esum = fwd_epilogue<CTT, NW, NTW, MCPC_ACT_IDENTITY>(P, ph, lds, nt, wave, lane, chain0, acc, pa, pb, slot, rec_idx);
                if (do_energy) { esum = wave_sum(esum); if (lane == 0) red[ph.layer * NW + wave] += esum; }
            } else if (ph.type == PH_HEADF) {
                float lsum = headf_epilogue<CTT, NW, NTW>(P, ph, lds, nt, wave, lane, chain0, acc, pa, pb, slot, rec_idx, do_energy);
                if (do_energy) { lsum = wave_sum(lsum); if (lane == 0) red[kMaxLatent * NW + wave] += lsum; }
            } else if (ph.type == PH_BWD) {
                if (Ly.act == MCPC_ACT_RELU) bwd_epilogue_mode<CTT, NW, NTW, MCPC_ACT_RELU>(P, ph, nt, wave, lane, chain0, acc, pa, pb, s, t, upd_mode);
                else if (Ly.act == MCPC_ACT_TANH) bwd_epilogue_mode<CTT, NW, NTW, MCPC_ACT_TANH>(P, ph, nt, wave, lane, chain0, acc, pa, pb, s, t, upd_mode);
                else bwd_epilogue_mode<CTT, NW, NTW, MCPC_ACT_IDENTITY>(P, ph, nt, wave, lane, chain0, acc, pa, pb, s, t, upd_mode);
            }
            STAMP_T(2, ph.type);
            if (ph.flags & PHF_SYNC) __syncthreads();
            STAMP(13);
        }
        // no barrier at the end of a step: the first barrier of the next step (after the top-layer
        // pass, which only writes FX_0 and the other copy of red[]) orders this step's readers of
        // E_l / e_o before their next writers.
    }
    spill_max_publish(P.spillmax, lds + P.lds_spillmax, lane);     // what this workgroup spilled at most, per tensor (every wave, when it is through)
#ifdef MCPC_STAMPS
    if (lane == 0)
        for (int i = 0; i < 16; ++i) P.dbg[((size_t)blockIdx.x * NW + wave) * 16 + i] = st_sum[i];
#endif
}

}  // namespace mcpc
