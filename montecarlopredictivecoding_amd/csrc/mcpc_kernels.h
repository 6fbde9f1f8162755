// MCPC kernels for gfx950 (MI355X).  See DESIGN.md for the data layout and the per-kernel rooflines.
//
// K1  mcpc_steps_kernel   fused Langevin / PC inference steps, persistent over n_steps:
//                         one workgroup = 16 chains (one MFMA column tile), all layers, weights streamed from L2 in
//                         MFMA-fragment order, state in HBM/L2 (padded), activations/errors in LDS.
//                         replaces reference pc_trainer.py:733-918 + utils/model.py:35-44 per step.
// and the small kernels around it: weight packing, target images, padding, mu_1, Linear 0's Hebbian sums, energy reduction, gradient
// export, the normals.  (K3, the Hebbian flush of the Linears j >= 1, is a translation unit of its own: mcpc_hebbian.h, mcpc_flush.hip.)
// The parameter structs, table entries and tile shapes these kernels and the host agree on are in mcpc_types.h; the other step-kernel
// forms (mcpc_steps_ws2.h, mcpc_steps_u.h, mcpc_steps_lw.h) build on this header.  Non-template kernels are defined here, so ONE
// translation unit includes it: mcpc_api.hip.
#pragma once
#include "mcpc_types.h"
#include "mcpc_step_math.h"
#include "mcpc_gemm_f16.h"

namespace mcpc {

// Request the operands of a phase's epilogue (x, targets: streamed from HBM/MALL; mu1, bias from L2; E from LDS)
// into pa/pb, ahead of the phase's GEMM.  Branch-free on purpose: the entry type only selects ADDRESSES, every slot
// issues the same three loads (one streamed, one cached, one LDS).  With a load inside an `if` hipcc joins the
// branches behind an `s_waitcnt vmcnt(0)`, which serialised the slots at full HBM latency each.
// CTT, here and in the epilogues below, is always 1 (one MFMA column tile of 16 chains per workgroup; two were measured and dropped in
// rounds 4 and 5).  The parameter and a one-trip `ct` loop are left in the functions whose compiled code changes without the loop
// (profiles/ctt_removal_asm.txt); everything else knows one tile only.
template <int CTT, int NW, int NTW>
__device__ __forceinline__ void issue_epilogue_loads(const KParams& P, const KPhase& ph, const float* lds, int nt, int wave,
                                                     int lane, int chain0, f32x4 (&pa)[NTW], f32x4 (&pb)[NTW]) {
    const KLayer& Ly = P.layer[ph.layer];
    const int c = lane & 15, q = lane >> 4;
    const bool is_head = ph.type == PH_HEADF, is_bwd = ph.type == PH_BWD;
    const bool mu1 = (ph.flags & PHF_MU1) != 0 || (is_bwd && ph.layer == 0);
    const bool has_y = is_head && P.head.loss_kind != MCPC_LOSS_NONE;
    // streamed operand: x_l (FWD, BWD) or the target (HEADF with a loss; without one any valid row of x)
    const float* const baseA = has_y ? P.head.y : Ly.x;
    const int strideA = has_y ? P.head.npad : Ly.npad;
    // cached operand: mu1 rows (top layer), else the bias of the Linear that produced the accumulators
    const float* const baseB = mu1 ? P.mu1 : (is_head ? P.head.bias : Ly.bias);
    const int strideB = mu1 ? Ly.npad : 0;
    const int tile_last = ph.tile0 + (ph.ntiles > 0 ? ph.ntiles - 1 : 0);   // entries without tiles (ENERGY) still load valid rows
    const float ecoef = Ly.ecoef;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        int ut = ph.tile0 + wave + NW * i;                     // slots past nt re-read the entry's last tile (never used)
        ut = ut > tile_last ? tile_last : ut;
        const int u0 = 16 * ut + 4 * q;
        const int uA = (is_head && !has_y) ? 0 : u0;
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const int cl = 16 * ct + c;
            const f32x4 va = ld4s(baseA + (size_t)(chain0 + cl) * strideA + uA);
            const f32x4 vg = ld4(baseB + (size_t)(chain0 + cl) * strideB + u0);
            const f32x4 ve = ld4(lds + Ly.lds_e + cl * Ly.ld + (is_bwd ? u0 : 4 * q));
            pa[i] = va;
            pb[i] = is_bwd ? (mu1 ? (va - vg) * ecoef : ve) : vg;
        }
    }
}

// ---- GEMM core ------------------------------------------------------------------------------------------------------------
// fp32 products on the fp16 matrix pipe with per-row power-of-two scaling (mcpc_gemm_f16.h): frag_t, kKB (k-depth of a fragment block),
// kFragBlock (16-byte units per tile and block), frag_zero, load_frag, gemm_tiles, GemmScale, prefetch_first_blocks.  The B operand is read
// from fp32 LDS rows.  (Rounds 1-2 ran v_mfma_f32_16x16x4_f32 here, rounds 3-4 six bf16 MFMAs per product: git history)

// the weights' exponent of a phase's Linear, through the constant address space (a wave-uniform s_load like the phase descriptors)
__device__ __forceinline__ int load_wexp(const int* wexp, int lin) {
    typedef __attribute__((address_space(4))) const int cint;
    return ((cint*)wexp)[lin];
}
// B exponent of the read-out error rows: a Bernoulli read-out's sigma(o) - y is bounded by 1 for targets in [0, 1], by 3 for targets in
// [-1, 2] (3 x 2^13 < 65 504: both fp16 pieces stay finite) -> a FIXED exponent, independent of how the read-out is cut into chunks.
// `bounded` is what mcpc_bind_target found (KHead::y_bounded): the reference's BCEWithLogitsLoss (utils/model.py:17-22) takes ANY target and
// stays finite, so a target outside that range (un-normalised 0..255 pixels) must not meet a constant scale -- it takes the exponent of
// the rows themselves like every unbounded read-out error (round 6, ADVICE r5: e 2^13 overflowed fp16 to Inf from |y| ~ 8 on, silently).
__device__ __forceinline__ int headb_fixed_exp(int loss_kind, bool bounded) { return loss_kind == MCPC_LOSS_BERNOULLI && bounded ? 13 : kScaleAuto; }
// unified-wave kernel: with that constant exponent the read-out's epilogue can write the error rows already split into the fp16 planes the
// back-projection reads -- once per value instead of once per k-block, wave and step (the long contractions only: a short one keeps its
// fourth product and its own code path)
__device__ __forceinline__ bool headf_planes(int loss_kind, bool bounded, int out_pad) { return loss_kind == MCPC_LOSS_BERNOULLI && bounded && out_pad > kShortK * kKB; }

// ---- row exponents kept by the producers (in-place kernel, lean epilogues) ------------------------------------------------------------
// The GEMM core scales every chain row of its LDS operand by a power of two taken from the row's largest |value| (mcpc_gemm_f16.h).
// Scanning the row for it in front of the GEMM (gemm_row_exp) sits on the step's critical path -- the row is complete only when the
// GEMM may start -- and cost 2.8 of 30 us per step at cfg-M (profiles/r05_k1_bounds.txt).  The epilogue waves that WRITE the rows know
// the values: each lane keeps the maximum of what it stores of its chain's row in an entry and adds it with ONE ds_max_u32 to the
// row's word of the operand, as (generation << 8) | biased exponent: a newer generation of the operand (the step it is written in;
// the entry for a ring slot, which is reused inside a step) supersedes the older one without a reset, the same generation's writers
// -- the four epilogue waves, several entries of a wide layer -- combine to the row's maximum.  The word is complete when the
// consumer's dependency on the producing entries is (the atomic precedes the wave's progress-counter store in LDS order), and it is
// protected against the next generation's writers exactly as the rows are.  The exponent is the one gemm_row_exp computes (the field of
// the maximum is the maximum of the fields; v_max skips NaN in both), so kernel forms with and without it agree bitwise.
// (the ids of the words -- kRowExpIds, rowexp_fx / rowexp_e / rowexp_ring -- are the planner's too: mcpc_types.h)
__device__ __forceinline__ void rowexp_track(float* lds_rowexp, int id, int row, float lane_max, unsigned gen) {
    atomicMax(reinterpret_cast<unsigned*>(lds_rowexp) + 16 * id + row, (gen << 8) | (__float_as_uint(lane_max) >> 23));
}
__device__ __forceinline__ int rowexp_read(const float* lds_rowexp, int id, int row) {
    return scale_exp_for_field((int)(reinterpret_cast<const unsigned*>(lds_rowexp)[16 * id + row] & 0xffu));
}

// guarded scalar store of a C-layout quad into an unpadded [B][n] tensor row
__device__ __forceinline__ void st_unpadded(float* base, int chain, int n, int u0, f32x4 v) {
    float* p = base + (size_t)chain * n + u0;
    if (u0 + 0 < n) p[0] = v.x;
    if (u0 + 1 < n) p[1] = v.y;
    if (u0 + 2 < n) p[2] = v.z;
    if (u0 + 3 < n) p[3] = v.w;
}
__device__ __forceinline__ f32x4 ld_unpadded(const float* base, int chain, int n, int u0) {
    const float* p = base + (size_t)chain * n + u0;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (u0 + 0 < n) v.x = p[0];
    if (u0 + 1 < n) v.y = p[1];
    if (u0 + 2 < n) v.z = p[2];
    if (u0 + 3 < n) v.w = p[3];
    return v;
}

#ifdef MCPC_STAMPS
// Diagnostic build (never shipped): s_memtime deltas per phase type, summed per wave (guide section 7,
// "In-kernel stamps"); read the SHARES, the fences change the absolute time.
#define STAMP_DECL unsigned long long st_sum[16] = {0}; unsigned long long st_last = mcpc_stamp();
#define STAMP(i) do { const unsigned long long st_now = mcpc_stamp(); st_sum[i] += st_now - st_last; st_last = st_now; } while (0)
__device__ __forceinline__ unsigned long long mcpc_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
// static slot per phase type (a runtime-indexed st_sum[] would live in scratch and distort the shares)
#define STAMP_T(b, ty) do { if ((ty) == 0) STAMP(b); else if ((ty) == 1) STAMP(3 + b); else if ((ty) == 2) STAMP(6 + b); else STAMP(9 + b); } while (0)
#else
#define STAMP_DECL
#define STAMP(i) do {} while (0)
#define STAMP_T(b, ty) do {} while (0)
#endif

// ---- FWD epilogue: prediction errors, energies, activations to LDS, spills, trajectory records -------
template <int CTT, int NW, int NTW, int ACT, bool WRITE_FX = true>
__device__ __forceinline__ float fwd_epilogue(const KParams& P, const KPhase& ph, float* lds, int nt, int wave, int lane,
                                              int chain0, const f32x4 (&acc)[NTW], const f32x4 (&pa)[NTW],
                                              const f32x4 (&pb)[NTW], int slot, int rec_idx) {
    const KLayer& Ly = P.layer[ph.layer];
    const int c = lane & 15, q = lane >> 4;
    const int l = ph.layer, npad = Ly.npad, n = Ly.n, ld = Ly.ld, B = P.B, Bpad = P.Bpad;
    const float ecoef = Ly.ecoef;
    float* const fx_lds = lds + Ly.lds_a;
    float* const e_lds = lds + Ly.lds_e;
    float* const spill_a = Ly.spill_a;
    float* const spill_e = Ly.spill_e;
    float* const rec = (rec_idx >= 0 && Ly.rec != nullptr) ? Ly.rec + (size_t)rec_idx * B * n : nullptr;
    float esum = 0.f;
    float amx = 0.f, emx = 0.f;            // largest |value| this call spills of A_l / E_l (spill_track)
    // unrolled over the wave's tiles: independent quads give the scheduler ILP to cover the
    // transcendental / LDS / global latencies of a single wave (a rolled loop serialises them)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i >= nt) continue;
        const f32x4 a = acc[i], xa = pa[i], xb = pb[i];
        const int u0 = 16 * (ph.tile0 + wave + NW * i) + 4 * q;
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const int cl = 16 * ct + c, chain = chain0 + cl;
            const bool live = chain < B;
            const f32x4 x = xa;
            f32x4 d;                                              // x - mu
            const f32x4 e = pc_error4(x, a + xb, ecoef, d);
            const f32x4 fx = act4<ACT>(x);
            if constexpr (WRITE_FX) st4(fx_lds + cl * ld + u0, fx);   // in-place variant: FX_l is written by the x update
            if (l > 0) st4(e_lds + cl * ld + u0, e);
            if (slot >= 0) {
                const f32x4 z = splat(0.f);
                const size_t srow = (size_t)slot * Bpad + chain;
                st4s(spill_a + spill_offset(Ly.spill_a_tm, srow, u0, npad), live ? fx : z);
                amx = absmax4(amx, live ? fx : z);
                if (l > 0) {
                    st4s(spill_e + spill_offset(Ly.spill_e_tm, srow, u0, npad), live ? e : z);
                    emx = absmax4(emx, live ? e : z);
                } else if (live) {    // Linear 0 sees a constant input: only sum_t e_1 is needed
                    float* sp = spill_e + (size_t)chain * npad + u0;
                    st4s(sp, ld4s(sp) + e);
                }
            }
            if (rec != nullptr && live) st_unpadded(rec, chain, n, u0, x);
            esum += live ? pc_energy4(d, ecoef) : 0.0f;
        }
    }
    if (slot >= 0) {
        spill_track(lds + P.lds_spillmax, spill_id_a(l), amx, lane);
        if (l > 0) spill_track(lds + P.lds_spillmax, spill_id_e(l), emx, lane);
    }
    return esum;
}

// ---- HEADF epilogue: read-out, loss error e_o into the LDS chunk, loss value, spills, output records ----
template <int CTT, int NW, int NTW>
__device__ __forceinline__ float headf_epilogue(const KParams& P, const KPhase& ph, float* lds, int nt, int wave, int lane,
                                                int chain0, const f32x4 (&acc)[NTW], const f32x4 (&pa)[NTW],
                                                const f32x4 (&pb)[NTW], int slot, int rec_idx, bool do_energy) {
    const KHead& H = P.head;
    const int c = lane & 15, q = lane >> 4;
    const int npad = H.npad, n = H.n, ld = ph.out_ld, B = P.B, Bpad = P.Bpad, mask_start = H.mask_start, kind = H.loss_kind;
    const float inv_var = H.inv_var;
    float* const eo_lds = lds + ph.out_lds;
    float* const spill = H.spill_e;
    float* const rec = (rec_idx >= 0 && H.rec_out != nullptr) ? H.rec_out + (size_t)rec_idx * B * n : nullptr;
    float lsum = 0.f;
    float omx = 0.f;                       // largest |value| this call spills of E_o (spill_track)
    // unrolled over the wave's tiles: independent quads give the scheduler ILP to cover the
    // transcendental / LDS / global latencies of a single wave (a rolled loop serialises them)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i >= nt) continue;
        const f32x4 a = acc[i], xa = pa[i], xb = pb[i];
        const int ut = ph.tile0 + wave + NW * i;
        const int u0 = 16 * ut + 4 * q;
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const int cl = 16 * ct + c, chain = chain0 + cl;
            const bool live = chain < B;
            const f32x4 o = a + xb;
            f32x4 e = splat(0.f);
            if (kind != MCPC_LOSS_NONE) {
                const f32x4 y = xa;
                MCPC_READOUT_LOSS4(e, o, y, kind, do_energy, inv_var, lsum, live && (u0 + r) >= mask_start && (u0 + r) < n, true);
            }
            st4(eo_lds + cl * ld + (u0 - 16 * ph.tile0), e);
            if (slot >= 0) { st4s(spill + spill_offset(H.spill_tm, (size_t)slot * Bpad + chain, u0, npad), e); omx = absmax4(omx, e); }
            if (rec != nullptr && live) st_unpadded(rec, chain, n, u0, o);
        }
    }
    if (slot >= 0) spill_track(lds + P.lds_spillmax, kSpillIdEo, omx, lane);
    return lsum;
}

// ---- BWD epilogue: x update of the phase's layer --------------------------------------------------------
//   g = e + sign * f'(x) * back ;  MODE 1: SGD, no noise   MODE 2: SGD + fused Philox kick   MODE 0: everything
//   else (Adam, external noise, gradients-only) behind wave-uniform branches.
template <int CTT, int NW, int NTW, int ACT, int MODE, bool FXOUT = false>
__device__ __forceinline__ void bwd_epilogue(const KParams& P, const KPhase& ph, int nt, int wave, int lane, int chain0,
                                             const f32x4 (&acc)[NTW], const f32x4 (&pa)[NTW],
                                             const f32x4 (&pb)[NTW], int s, int t, float* lds = nullptr) {
    const KLayer& Ly = P.layer[ph.layer];
    const int c = lane & 15, q = lane >> 4;
    const int l = ph.layer, npad = Ly.npad, n = Ly.n, B = P.B;
    const float sign = ph.sign, lr = P.lr, nscale = P.noise_scale;
    float* const xptr = Ly.x;
    const uint64_t seed = P.seed, step = P.step_base + (uint64_t)t, chain_base = P.chain_base;
    // unrolled over the wave's tiles: independent quads give the scheduler ILP to cover the
    // transcendental / LDS / global latencies of a single wave (a rolled loop serialises them)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i >= nt) continue;
        const f32x4 a = acc[i], xa = pa[i], xb = pb[i];
        const int u0 = 16 * (ph.tile0 + wave + NW * i) + 4 * q;
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const int chain = chain0 + 16 * ct + c;
            const size_t row = (size_t)chain * npad + u0;
            const f32x4 x = xa, e = xb, back = a;
            const f32x4 g = x_grad4<ACT>(x, e, back, sign);
            f32x4 xn;
            if constexpr (MODE == 0) {
                const bool live = chain < B;
                if (!P.update_x) {
                    if (live && Ly.xgrad != nullptr) st_unpadded(Ly.xgrad, chain, n, u0, g);
                    // x stays: put f(x) back where the back-projection was handed over
                    if constexpr (FXOUT) st4(lds + Ly.lds_a + (16 * ct + c) * Ly.ld + u0, act4<ACT>(x));
                    continue;
                }
                if (P.xopt == MCPC_XOPT_SGD) {
                    xn = x - g * lr;
                } else {
                    const size_t mrow = tile_major_offset(chain, u0, npad);      // (tile-major: see tile_major_offset)
                    f32x4 m = ld4s(Ly.m + mrow), v = ld4s(Ly.v + mrow);
                    adam_moments4(m, v, g, P.omb1, P.beta2, P.omb2);
                    st4s(Ly.m + mrow, m);
                    st4s(Ly.v + mrow, v);
                    xn = adam_x4(x, m, v, P.adam_coef[2 * s], P.adam_coef[2 * s + 1], P.eps);
                }
                if (P.noise_mode == MCPC_NOISE_PHILOX) {
                    xn = xn + normals4(seed, step, (uint32_t)l, (uint32_t)(chain_base + (uint64_t)chain), (uint32_t)(u0 >> 2)) * nscale;
                } else if (P.noise_mode == MCPC_NOISE_EXTERNAL && live) {
                    xn = xn + ld_unpadded(Ly.ext_noise + (size_t)s * B * n, chain, n, u0) * nscale;
                }
            } else {
                xn = x - g * lr;
                if constexpr (MODE == 2)
                    xn = xn + normals4(seed, step, (uint32_t)l, (uint32_t)(chain_base + (uint64_t)chain), (uint32_t)(u0 >> 2)) * nscale;
            }
            zero_padded4(xn, u0, n);
            st4s(xptr + row, xn);
            // in-place variant: the next step's GEMMs read f(x_new) from FX_l
            if constexpr (FXOUT) st4(lds + Ly.lds_a + (16 * ct + c) * Ly.ld + u0, act4<ACT>(xn));
        }
    }
}

template <int CTT, int NW, int NTW, int ACT, bool FXOUT = false>
__device__ __forceinline__ void bwd_epilogue_mode(const KParams& P, const KPhase& ph, int nt, int wave, int lane, int chain0,
                                                  const f32x4 (&acc)[NTW], const f32x4 (&pa)[NTW],
                                                  const f32x4 (&pb)[NTW], int s, int t, int mode, float* lds = nullptr) {
    if (mode == 2) bwd_epilogue<CTT, NW, NTW, ACT, 2, FXOUT>(P, ph, nt, wave, lane, chain0, acc, pa, pb, s, t, lds);
    else if (mode == 1) bwd_epilogue<CTT, NW, NTW, ACT, 1, FXOUT>(P, ph, nt, wave, lane, chain0, acc, pa, pb, s, t, lds);
    else bwd_epilogue<CTT, NW, NTW, ACT, 0, FXOUT>(P, ph, nt, wave, lane, chain0, acc, pa, pb, s, t, lds);
}

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

// ------------------------------------------------------------------------------------------------
// Weight packing into MFMA fragment order (run once per parameter change).
// f16 core (mcpc_gemm_f16.h): every weight, scaled by the Linear's power of two, is split into two fp16 pieces, stored as two planes per
// (tile, 32-deep block):
//   forward : Wf[ut][kb][plane][lane] (16 B) = W[16ut + (lane&15)][32kb + 8(lane>>4) + j], j = 0..7
//   backward: Wb[it][ub][plane][lane] (16 B) = W[32ub + 8(lane>>4) + j][16it + (lane&15)], j = 0..7
// in_blocks = ceil(16 in_tiles / 32), out_blocks = ceil(16 out_tiles / 32); elements beyond the matrix are zeros.
// max |W| of a Linear -> the exponent its packed fp16 planes are scaled by (mcpc_gemm_f16.h: scale_exp_for_max).  One block.
__global__ __launch_bounds__(1024) void mcpc_wexp_kernel(const float* __restrict__ W, size_t n, int* __restrict__ wexp_slot) {
    __shared__ float part[16];
    float mx = 0.f;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, fabsf(W[i]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) mx = fmaxf(mx, part[w]);
        *wexp_slot = scale_exp_for_max(mx);
    }
}

__global__ void mcpc_pack_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                 float* __restrict__ Wf_, float* __restrict__ Wb_, float* __restrict__ bias_pad,
                                 int n_out, int n_in, int out_tiles, int in_tiles, const int* __restrict__ wexp_slot) {
    u32x4* const Wf = reinterpret_cast<u32x4*>(Wf_);
    u32x4* const Wb = reinterpret_cast<u32x4*>(Wb_);
    const float ws = pow2i(*wexp_slot);                    // (written by mcpc_wexp_kernel on the same stream)
    const int in_blocks = (16 * in_tiles + kKB - 1) / kKB, out_blocks = (16 * out_tiles + kKB - 1) / kKB;
    const size_t n_fwd = (size_t)out_tiles * in_blocks * 64, n_bwd = (size_t)in_tiles * out_blocks * 64;
    const size_t total = n_fwd > n_bwd ? n_fwd : n_bwd;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int lane = idx & 63, m = lane & 15, g = lane >> 4;
        const size_t blk = idx >> 6;
        if (idx < n_fwd) {   // blk = ut * in_blocks + kb
            const int ut = blk / in_blocks, kb = blk % in_blocks;
            const int u = 16 * ut + m;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kKB * kb + 8 * g + j;
                v[j] = (u < n_out && k < n_in) ? W[(size_t)u * n_in + k] : 0.f;
            }
            const frag_t f = split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, ws);
            Wf[blk * kFragBlock + lane] = f.h; Wf[blk * kFragBlock + 64 + lane] = f.m;
        }
        if (idx < n_bwd) {   // blk = it * out_blocks + ub
            const int it = blk / out_blocks, ub = blk % out_blocks;
            const int i = 16 * it + m;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int u = kKB * ub + 8 * g + j;
                v[j] = (u < n_out && i < n_in) ? W[(size_t)u * n_in + i] : 0.f;
            }
            const frag_t f = split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, ws);
            Wb[blk * kFragBlock + lane] = f.h; Wb[blk * kFragBlock + 64 + lane] = f.m;
        }
    }
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < out_tiles * 16) bias_pad[gid] = (bias != nullptr && gid < n_out) ? bias[gid] : 0.f;
}

// Bit-pack a padded target image [Bpad][npad] whose values are all exactly 0.0f / 1.0f (binarised MNIST, the Bernoulli
// read-out's usual target): 98 B per chain instead of 3 136 B re-read from HBM in every step.  *flag is cleared by the first
// value that is neither; the step kernel then reads the fp32 image as before.  flag[2] is cleared by the first value outside [-1, 2]
// (headb_fixed_exp: the read-out error's constant fp16 scale holds for bounded targets only).  One thread per 32-unit word.
__global__ void mcpc_pack_target_bits_kernel(const float* __restrict__ ypad, uint32_t* __restrict__ bits, int* __restrict__ flag,
                                             int Bpad, int npad, int ywords) {
    const size_t total = (size_t)Bpad * ywords;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / ywords, w = idx % ywords;
        uint32_t word = 0;
        bool ok = true, bounded = true;
        for (int j = 0; j < 32; ++j) {
            const int u = 32 * w + j;
            if (u >= npad) break;
            const float v = ypad[(size_t)row * npad + u];
            const uint32_t pat = __float_as_uint(v);
            if (pat == 0x3F800000u) word |= 1u << j;
            else if (pat != 0u) ok = false;
            if (!(v >= -1.0f && v <= 2.0f)) bounded = false;          // (NaN: not bounded)
        }
        bits[idx] = word;
        if (!ok) flag[0] = 0;
        if (!bounded) flag[2] = 0;          // (flag[1] is the constant 0 of tuning no_ybits)
    }
}

// tile-major copy of a padded image [Bpad][npad] (tile_major_offset: the 16 chains x 16 units of a wave access contiguous)
__global__ void mcpc_tile_major_kernel(const float* __restrict__ src, float* __restrict__ dst, int Bpad, int npad) {
    const size_t total = (size_t)Bpad * npad / 4;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / (npad / 4), u0 = 4 * (int)(idx % (npad / 4));
        *reinterpret_cast<f32x4*>(dst + tile_major_offset(row, u0, npad)) = *reinterpret_cast<const f32x4*>(src + (size_t)row * npad + u0);
    }
}

// dst[Bpad][npad] <- src[B][n] (zero padded)      /     dst[B][n] <- src[Bpad][npad]
__global__ void mcpc_pad_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int n, int Bpad, int npad) {
    const size_t total = (size_t)Bpad * npad;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / npad, col = idx % npad;
        dst[idx] = (src != nullptr && row < B && col < n) ? src[(size_t)row * n + col] : 0.f;
    }
}
// export of Adam's moments: the engine keeps them tile-major (tile_major_offset), the caller gets [B][n]
__global__ void mcpc_unpad_adam_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int n, int npad) {
    const size_t total = (size_t)B * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / n, col = idx % n;
        dst[idx] = src[tile_major_offset(row, col & ~3, npad) + (col & 3)];
    }
}

__global__ void mcpc_unpad_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int n, int npad) {
    const size_t total = (size_t)B * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / n, col = idx % n;
        dst[idx] = src[(size_t)row * npad + col];
    }
}

// mu1[Bpad][npad] = inputs W0^T + b0 (inputs may be null = zeros).  Tiny (n_in*n_1 per chain).
__global__ void mcpc_mu1_kernel(const float* __restrict__ inputs, const float* __restrict__ W0,
                                const float* __restrict__ b0, float* __restrict__ mu1,
                                int B, int n_in, int n1, int Bpad, int npad) {
    const size_t total = (size_t)Bpad * npad;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = idx / npad, u = idx % npad;
        float acc = 0.f;
        if (u < n1) {
            if (b0 != nullptr) acc = b0[u];
            if (inputs != nullptr && row < B) {
                float dot = 0.f;
                for (int k = 0; k < n_in; ++k) dot = fmaf(inputs[(size_t)row * n_in + k], W0[(size_t)u * n_in + k], dot);
                acc += dot;
            }
        }
        mu1[idx] = acc;
    }
}

// Linear 0 (constant input): G_W0[u][k] -= sum_chain esum[chain][u] * inputs[chain][k];  G_b0[u] -= sum_chain esum[chain][u].
// One block per (unit u, column k) -- blockIdx.y == n_in is the bias -- 256 threads stride over the chains, partial sums
// meet in a fixed-order LDS tree: bitwise reproducible.  (One thread per output looping over 6000 chains took 2.3 ms.)
__global__ __launch_bounds__(256) void mcpc_dw0_kernel(const float* __restrict__ esum, const float* __restrict__ inputs,
                                                       float* __restrict__ gW, float* __restrict__ gb, int B, int n1, int npad1,
                                                       int n_in, int gw_ld) {
    __shared__ float part[256];
    const int u = blockIdx.x, k = blockIdx.y;
    const bool is_bias = inputs == nullptr || k == n_in;
    float s = 0.f;
    for (int ch = threadIdx.x; ch < B; ch += 256) {
        const float ev = esum[(size_t)ch * npad1 + u];
        s = is_bias ? s + ev : fmaf(ev, inputs[(size_t)ch * n_in + k], s);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (is_bias) gb[u] -= part[0];
        else gW[(size_t)u * gw_ld + k] -= part[0];
    }
}

// energies_out[row][:] = {loss, E_1..E_L, 0.., overall} from per-workgroup partials: one wave per row, lane i sums the
// slots i, i+64, ... of every column, then a butterfly over the lanes -- fixed order, fp64, bitwise reproducible.
__global__ __launch_bounds__(256) void mcpc_energy_reduce_kernel(const double* __restrict__ epart, double* __restrict__ out, int rows,
                                                                 int nwg, int L) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    double col[kMaxLatent + 1];
#pragma unroll
    for (int l = 0; l <= kMaxLatent; ++l) col[l] = 0.0;
    for (int w = lane; w < nwg; w += 64) {
        const double* p = epart + ((size_t)row * nwg + w) * (kMaxLatent + 1);
#pragma unroll
        for (int l = 0; l <= kMaxLatent; ++l) col[l] += p[l];
    }
#pragma unroll
    for (int l = 0; l <= kMaxLatent; ++l)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) col[l] += __shfl_xor(col[l], off, 64);
    if (lane == 0) {
        double* o = out + (size_t)row * kEnergyCols;
        double overall = 0.0;
#pragma unroll
        for (int l = 0; l < kMaxLatent; ++l) { o[1 + l] = col[l]; overall += col[l]; }
        o[0] = col[kMaxLatent];
        o[kEnergyCols - 1] = overall + col[kMaxLatent];
    }
}

// out[scale * G] with un-padding: dst[u][i] (=|+=) scale * G[u][i_pad]
__global__ void mcpc_export_grad_kernel(const float* __restrict__ G, float* __restrict__ dst, int n_out, int n_in, int ld,
                                        float scale, int accumulate) {
    const size_t total = (size_t)n_out * n_in;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int u = idx / n_in, i = idx % n_in;
        const float v = scale * G[(size_t)u * ld + i];
        dst[idx] = accumulate ? dst[idx] + v : v;
    }
}

__global__ void mcpc_philox_kernel(uint64_t seed, uint64_t step, int layer, uint64_t chain_base, int batch, int n_units,
                                   float* __restrict__ out, int raw) {
    const int groups = (n_units + 3) / 4;
    const size_t total = (size_t)batch * groups;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int chain = idx / groups, g = idx % groups;
        float v[4];
        if (raw) {
            uint32_t r[4];
            philox4x32_10((uint32_t)(chain_base + chain), ((uint32_t)layer << 24) | (uint32_t)g, (uint32_t)step,
                          (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
            for (int k = 0; k < 4; ++k) v[k] = __uint_as_float(r[k]);
        } else {
            const f32x4 z = normals4(seed, step, (uint32_t)layer, (uint32_t)(chain_base + chain), (uint32_t)g);
            v[0] = z.x; v[1] = z.y; v[2] = z.z; v[3] = z.w;
        }
        for (int k = 0; k < 4; ++k)
            if (4 * g + k < n_units) out[(size_t)chain * n_units + 4 * g + k] = v[k];
    }
}

// box_muller on bits the caller chooses (diagnostic: the transform's whole domain is 2^24 radii x 2^24 angles)
__global__ void mcpc_box_muller_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n,
                                       float* __restrict__ z0, float* __restrict__ z1) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x)
        box_muller(a[idx], b[idx], z0[idx], z1[idx]);
}

}  // namespace mcpc
