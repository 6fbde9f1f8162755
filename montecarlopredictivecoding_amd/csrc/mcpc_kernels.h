// What the step kernels of every form share (see DESIGN.md for the data layout and the per-kernel rooflines): the request of an epilogue's
// operands, the generic epilogues (FWD, HEADF, BWD with every optimiser and noise mode behind wave-uniform branches), the row-exponent
// words, guarded stores into unpadded tensors and the in-kernel stamps of the diagnostic build.  Device functions and macros only -- no
// __global__ kernel is defined here, so any unit that holds a step kernel or an evaluator may include it.  The kernels themselves:
//   mcpc_steps_barrier.h   K1 in its first form, mcpc_steps_kernel (a workgroup barrier per table entry)     -> mcpc_steps_lw.hip
//   mcpc_steps_ws2.h       the in-place kernel                                                   -> mcpc_steps_ws2.hip, mcpc_steps_ws2_spec.hip
//   mcpc_steps_u.h         the unified-wave kernel                                               -> mcpc_steps_u.hip
//   mcpc_steps_lw.h        the layer-wise kernels (their tile: mcpc_lw_tile.h)                   -> mcpc_steps_lw.hip
//   mcpc_engine_kernels.h  weight packing, target images, padding, mu_1, gradient export, normals -> mcpc_api.hip
//   mcpc_run_kernels.h     Linear 0's Hebbian sums, the energy reduction                          -> mcpc_run.hip
// (K3, the Hebbian flush of the Linears j >= 1: mcpc_hebbian.h, mcpc_flush.hip.)
// The parameter structs, table entries and tile shapes the kernels and the host agree on are in mcpc_types.h.
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

}  // namespace mcpc
