// Lean epilogues of the in-place step kernel's E waves for the paths every script of the reference runs per step:
// SGD on x with or without the fused Philox kick, fused x update, workgroup fully inside the batch.
//
// Why they exist (measured, round 2): on gfx950 the fp32 MFMA and the VALU never co-execute
// (SQ_VALU_MFMA_COEXEC_CYCLES = 0 for this kernel), so every VALU instruction an E wave issues is taken out of its
// partner's MFMA stream -- the step kernel's time is MFMA cycles + VALU cycles + what neither fills.  With the GEMMs
// switched off the E waves alone needed 35 us of a 94 us step.  The generic epilogues (mcpc_kernels.h) spend much of
// their instruction count on things these paths do not need:
//   * 64-bit per-lane addresses for every access   -> wave-uniform base (SGPR pair) + one 32-bit byte offset per lane:
//     a row offset computed once per entry (v_mul_u32_u24), one v_add per tile;
//   * per-element `live` / padding / mask predicates -> padded units and partial loss masks are handled by a wave-uniform branch on
//     the one tile that has them; padding CHAINS (the last workgroup of a batch that is not a multiple of 16) cost one per-lane mask:
//     they evolve like any chain, and their energy terms are dropped by a select, their spills ANDed with 0, their records skipped
//     (LeanLane::livem) -- until round 3 such a workgroup took the generic epilogues and every launch waited for it (+17 %
//     per step at 7000 chains);
//   * three loads per slot whatever the entry type   -> each entry type requests exactly its operands.
// The arithmetic per element is mcpc_step_math.h's, like the generic epilogues': trajectories stay bitwise those of the
// other kernel forms and schedules (tests/test_gpu_fullsize.py, tests/test_gpu_rounds.py; bench.py self_check).
//
// XL (KParams::xl, 16-chain plans whose LDS has the room -- 45 KB more at cfg-M): the state rows x_l of the workgroup's chains, the
// biases, the mu_1 rows and the bit-packed target rows are copied to LDS when the launch starts (ws2_fill_fx / ws2_fill_constants);
// the epilogues read them there, the x update writes the new state there, and the rows go back to global memory once, after the
// step loop (lean_store_x).  An E wave then issues NO global load inside the step loop.  Why that matters: a wave's vector memory
// operations retire in order, so every operand load of an entry also waited for the Hebbian spill stores of the entry before it --
// 12.5 us of a 96 us step in the Hebbian stretches of cfg-M (timing build without the stores: 78.5 us against 88.5 per step of a
// learning call), and the x store / x loads of every step besides.
#pragma once
#include "mcpc_kernels.h"       // the barrier kernel's epilogues, row-exponent words, stamps
#include "mcpc_steps_ws.h"      // progress counters and hand-off fences

namespace mcpc {

typedef const char __attribute__((address_space(1)))* gbytes_t;
typedef char __attribute__((address_space(1)))* gbytes_w_t;

__device__ __forceinline__ f32x4 gld4(const float* base, uint32_t boff) {
    return *reinterpret_cast<const gf32x4*>((gbytes_t)base + boff);
}
__device__ __forceinline__ f32x4 gld4s(const float* base, uint32_t boff) {
    return __builtin_nontemporal_load(reinterpret_cast<const gf32x4*>((gbytes_t)base + boff));
}
__device__ __forceinline__ void gst4s(float* base, uint32_t boff, f32x4 v) {
    __builtin_nontemporal_store(v, reinterpret_cast<gf32x4*>((gbytes_w_t)base + boff));
}
__device__ __forceinline__ uint32_t mul24(uint32_t a, uint32_t b) { return __umul24(a, b); }

// Hebbian spill store through a buffer descriptor (wave-uniform base, 32-bit lane offset, selectable cache policy).  The data is
// read next by another kernel on other CUs, and 44 MB of it per step flow through L2s of 4 MB that hold the 3.3 MB of packed
// weights every GEMM wave streams.  Round 2 (epilogue loads still queued behind these stores in the wave's vector-memory order):
// plain write-back stores were 0.4 us per step faster than any other policy.  Round 3 (no global loads left in the epilogue waves,
// XL): system-scope stores -- sc1, with or without sc0 / nt -- take the learning call of cfg-M from 80.4-81.1 to 77.6-78.0 us
// per step, nt alone or sc0 nt do not; not issuing the stores at all: 71.7.  A shard of 256 chains, whose spill never leaves the
// L2, loses 6 % with them (24.4 -> 25.8 us per step of a learning call): `sys` (KParams::spill_sys, wave-uniform) chooses.
// Round 5 (the step kernel 1.3 x faster, the same stores per step): measured again, one gpurun call, learning call at 6000 / 4096 chains,
// us per step -- write-back 59.1-60.2 / 40.1-40.3, sc1 57.0-57.2 / 38.2-38.4, sc0 sc1 56.6-57.4 / 37.8, sc1 nt 55.9-56.2 / 37.8-38.2, sc0 sc1 nt
// (round 3's choice) 56.6 / 38.2-38.6, and a plain GLOBAL nontemporal store (no buffer descriptor) **55.1-55.5 / 37.3-37.4**: the default now.
#ifndef MCPC_SPILL_AUX
#define MCPC_SPILL_AUX -1          // < 0: global nontemporal store; else the gfx950 cache-policy bits of a buffer store: 1 = sc0, 2 = nt, 16 = sc1; 0 = plain write-back
#endif
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void spill_st4(float* base, uint32_t image_bytes, uint32_t boff, f32x4 v, bool sys = true) {
#ifdef MCPC_EXP_NOSPILL        // timing experiment only (wrong Hebbian sums): the spill stores are not issued
    (void)base; (void)image_bytes; (void)boff; (void)v; (void)sys;
#elif MCPC_SPILL_AUX < 0
    if (sys) {
        gst4s(base, boff, v); (void)image_bytes;
    } else {          // (a small shard's spill stays in the L2: plain write-back stores)
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)image_bytes, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rsrc, (int)boff, 0, 0);
    }
#else
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)image_bytes, 0x00020000);
    if (sys) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rsrc, (int)boff, 0, MCPC_SPILL_AUX);
    else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rsrc, (int)boff, 0, 0);
#endif
}

// ---- compile-time run mode of the in-place step kernel (mcpc_steps_ws2.h) -------------------------------------------------------------
// What a launch decides once -- optimizer and noise, XL, row words, whether it accumulates, the read-out's loss and target form, the
// activations -- is a run-time value of KParams in the generic kernel, re-tested in every workgroup, table entry and tile loop; the
// compiler keeps the union of all paths alive (294 spilled SGPRs).  A field of Ws2Mode fixes one such decision at
// compile time; kModeDyn leaves it to the run-time test, which then compiles to exactly the generic kernel's code for that decision.
// ws2_select_mode (mcpc_run.hip) returns a specialised mode only when every launched workgroup would have decided the same.
constexpr int kModeDyn = -1;
enum { WS2_UPD_SGD = 1, WS2_UPD_SGD_PHILOX = 2, WS2_UPD_ADAM = 3 };     // lean epilogues with the fused update: SGD, SGD + Philox kick, Adam without noise
enum { WS2_SPILL_OFF = 0, WS2_SPILL_SYS = 1 };                          // no step of the launch accumulates / every step does, its stores at system scope
enum { WS2_HEAD_NONE = 0, WS2_HEAD_BERNOULLI_BITS = 1 };                // no loss / Bernoulli read-out whose 0/1 target is read bit-packed (bounded: headb_fixed_exp)
template <int UPD_ = kModeDyn, int XL_ = kModeDyn, int ROWEXP_ = kModeDyn, int SPILL_ = kModeDyn, int HEAD_ = kModeDyn, int ACT_ = kModeDyn>
struct Ws2Mode {
    static constexpr int UPD = UPD_, XL = XL_, ROWEXP = ROWEXP_, SPILL = SPILL_, HEAD = HEAD_, ACT = ACT_;      // ACT: the activation of every latent layer
    static constexpr bool generic = UPD == kModeDyn && XL == kModeDyn && ROWEXP == kModeDyn && SPILL == kModeDyn && HEAD == kModeDyn && ACT == kModeDyn;
    static_assert(XL == kModeDyn || UPD != kModeDyn, "XL is a property of the lean epilogues");
    static_assert(ROWEXP == kModeDyn || UPD != kModeDyn, "row words are kept by the lean epilogues");
    // `slot` of a step (>= 0: the step spills into that ring slot)
    static __device__ __forceinline__ bool spills(int slot) { if constexpr (SPILL == kModeDyn) return slot >= 0; else return SPILL != WS2_SPILL_OFF; }
    static __device__ __forceinline__ bool spill_sys(const KParams& P) { if constexpr (SPILL == kModeDyn) return P.spill_sys != 0; else return SPILL == WS2_SPILL_SYS; }
    static __device__ __forceinline__ int loss_kind(const KHead& H) {
        if constexpr (HEAD == kModeDyn) return H.loss_kind; else return HEAD == WS2_HEAD_BERNOULLI_BITS ? MCPC_LOSS_BERNOULLI : MCPC_LOSS_NONE;
    }
    static __device__ __forceinline__ int act(int a) { if constexpr (ACT == kModeDyn) return a; else return ACT; }
    static __device__ __forceinline__ bool has_rx(const float* rx) { if constexpr (ROWEXP == kModeDyn) return rx != nullptr; else return ROWEXP != 0; }
};
using Ws2Generic = Ws2Mode<>;

// per-lane constants of an E wave, fixed for the launch
struct LeanLane {
    int c, q;
    uint32_t chain;            // global row (chain) of this lane
    uint32_t lrow;             // c: row inside the workgroup's LDS images
    uint32_t livem;            // ~0u / 0u: the chain lies inside the batch / is a padding chain
};
__device__ __forceinline__ f32x4 mask4(f32x4 v, uint32_t m) {
    f32x4 r;
    r.x = __uint_as_float(__float_as_uint(v.x) & m); r.y = __uint_as_float(__float_as_uint(v.y) & m);
    r.z = __uint_as_float(__float_as_uint(v.z) & m); r.w = __uint_as_float(__float_as_uint(v.w) & m);
    return r;
}

// tiles of this wave in an entry: tile(i) = tile0 + kk + NW i, i < nt
// CTT is always 1 (mcpc_kernels.h: issue_epilogue_loads): the one-trip `ct` loops left below are those the compiled code depends on

// ---- FWD entry (layer l): e_l = c_l (x_l - mu_l), energies, E_l -> LDS, Hebbian spills ------------------------------
// mu_l = acc (from G, in LDS at out_lds) + bias for l >= 1; the constant mu_1 row for l == 0 (no GEMM).
// e0acc: Linear 0 sees a constant input, so only sum_t e_1 is needed for its Hebbian sums; when the top layer has at most
// one tile per wave (n_1 <= 64) the running sum is held in registers for the whole launch (lean_load_e0 / lean_flush_e0)
// instead of a global read-modify-write in every step.
// REG (unified-wave kernel, mcpc_steps_u.h): the wave computed the block itself -- it arrives in registers (racc[i], zeros when the entry has
// no GEMM), nothing is waited for and nothing is read from out_lds.
template <int CTT, int NW, int NTW, int ACT, bool XL = false, bool REG = false, class M = Ws2Generic>
__device__ __forceinline__ float lean_fwd(const KParams& P, const KPhase& ph, float* lds, int nt, int kk, const LeanLane& L,
                                          int slot, int rec_idx, const int* prog_g, int need, int* err, int& dead,
                                          f32x4& e0acc, bool e0_in_regs, float* rx = nullptr, unsigned row_gen = 0u,
                                          const f32x4* racc = nullptr) {
    if (nt <= 0) return 0.f;                  // (a layer with fewer tiles than waves: nothing to load, nothing to wait for)
    const int tstep = REG ? ph.rot : NW;      // tile(i) = tile0 + kk + tstep i: the unified-wave kernel's rows carry their own stride (kk = 0)
    const KLayer& Ly = P.layer[ph.layer];
    const int l = ph.layer;
    const bool has_gemm = (ph.flags & PHF_WS_GEMM) && ph.nkb > 0;
    const uint32_t npad4 = 4u * (uint32_t)Ly.npad;
    uint32_t rowb, lrowb, orowb;
#pragma unroll
    for (int ct = 0; ct < CTT; ++ct) {
        rowb = mul24(L.chain, npad4) + 16u * L.q;
        lrowb = mul24(L.lrow, 4u * (uint32_t)Ly.ld) + 16u * L.q;
        orowb = mul24(L.lrow, 4u * (uint32_t)ph.out_ld) + 16u * L.q;
    }
    f32x4 xv[NTW], bv[NTW];
    const float* const bsrc = l == 0 ? P.mu1 : Ly.bias;                  // mu1: a row per chain; bias: one row
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const uint32_t tb = 64u * (uint32_t)(ph.tile0 + kk + tstep * (i < nt ? i : 0));     // unused slots repeat slot 0
        if constexpr (XL) {
            xv[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds + Ly.lds_x) + lrowb + tb);
            bv[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds + Ly.lds_bias) + (l == 0 ? lrowb : 16u * L.q) + tb);
            (void)bsrc;
        } else {
#if defined(MCPC_EXP_NOX) || defined(MCPC_EXP_NOELOAD)       // timing experiment only (wrong results): the state is neither loaded nor stored
        xv[i] = splat(0.5f);
#else
        xv[i] = gld4s(Ly.x, rowb + tb);
#endif
#ifdef MCPC_EXP_NOELOAD   // timing experiment only (wrong results): no operand loads at all in the E waves
        bv[i] = splat(0.25f); (void)bsrc;
#else
        bv[i] = gld4(bsrc, (l == 0 ? rowb : 16u * L.q) + tb);
#endif
        }
    }
    f32x4 av[NTW];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) av[i] = racc[i];
        (void)has_gemm; (void)prog_g; (void)need; (void)err; (void)dead; (void)orowb;
    } else if (has_gemm) {
        ws_wait_one(prog_g, need, err, dead);
        const char* const src = reinterpret_cast<const char*>(lds + ph.out_lds);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const uint32_t tb = 64u * (uint32_t)(ph.tile0 + kk + tstep * (i < nt ? i : 0));
            av[i] = *reinterpret_cast<const f32x4*>(src + orowb + tb);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NTW; ++i) av[i] = splat(0.f);
    }
    const float ecoef = Ly.ecoef;
    char* const e_lds = reinterpret_cast<char*>(lds + Ly.lds_e);
    float* const spill_a = M::spills(slot) ? Ly.spill_a + (size_t)slot * P.Bpad * Ly.npad : nullptr;
    float* const spill_e = M::spills(slot) ? (l > 0 ? Ly.spill_e + (size_t)slot * P.Bpad * Ly.npad : Ly.spill_e) : nullptr;
    float* const rec = (rec_idx >= 0 && Ly.rec != nullptr) ? Ly.rec + (size_t)rec_idx * P.B * Ly.n : nullptr;
    const uint32_t img_bytes = (uint32_t)P.Bpad * npad4;               // one [Bpad][npad] image (lean_ok: < 4 GiB)
    const bool sys = M::spill_sys(P);
    float esum = 0.f;
    float amx = 0.f, emx = 0.f;            // largest |value| this call spills of A_l / E_l (mcpc_kernels.h: spill_track)
    float rmx = 0.f;                       // largest |value| this lane writes of its chain's E_l row (rowexp_track)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i >= nt) continue;
        const int tile = ph.tile0 + kk + tstep * i;
        const uint32_t tb = 64u * (uint32_t)tile;
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const f32x4 x = xv[i];
            f32x4 d;                                                      // x - mu
            const f32x4 e = pc_error4(x, av[i] + bv[i], ecoef, d);
            if (l > 0) { *reinterpret_cast<f32x4*>(e_lds + lrowb + tb) = e; rmx = absmax4(rmx, e); }
            if (M::spills(slot)) {
#ifdef MCPC_EXP_SPILL_LINEAR      // timing experiment only (rows permuted inside the workgroup's block): one contiguous KiB per store
                const uint32_t sb = mul24(L.chain - (uint32_t)L.c, npad4) + 1024u * (uint32_t)tile + 16u * (uint32_t)(L.c + 16 * L.q);
#else
                const uint32_t sb = rowb + tb;
#endif
                // tile-major image: (chain's row tile, unit tile) is one contiguous KiB, lane (c, q) its float4 number c + 16 q
                const uint32_t sb_tm = mul24(L.chain - (uint32_t)L.c, npad4) + 1024u * (uint32_t)tile + 16u * (uint32_t)(L.c + 16 * L.q);
                spill_st4(spill_a, img_bytes, Ly.spill_a_tm ? sb_tm : sb, mask4(act4<ACT>(x), L.livem), sys);
                amx = absmax4(amx, mask4(act4<ACT>(x), L.livem));
                if (l > 0) { spill_st4(spill_e, img_bytes, Ly.spill_e_tm ? sb_tm : sb, mask4(e, L.livem), sys); emx = absmax4(emx, mask4(e, L.livem)); }
                else if (e0_in_regs) e0acc = e0acc + e;                          // (one tile per wave: i == 0 only)
                else gst4s(spill_e, rowb + tb, gld4s(spill_e, rowb + tb) + e);   // Linear 0: only sum_t e_1 is needed
            }
            if (rec != nullptr && L.livem) st_unpadded(rec, (int)L.chain, Ly.n, 16 * tile + 4 * L.q, x);
            esum += L.livem ? pc_energy4(d, ecoef) : 0.f;                  // (a select, not a product: whatever a padding chain holds)
        }
    }
    if (M::spills(slot)) {
        spill_track(lds + P.lds_spillmax, spill_id_a(l), amx, L.c + 16 * L.q);
        if (l > 0) spill_track(lds + P.lds_spillmax, spill_id_e(l), emx, L.c + 16 * L.q);
    }
    if (M::has_rx(rx) && ph.o_row >= 0) rowexp_track(rx, ph.o_row, L.c, rmx, row_gen);
    return esum;
}

// The running sum e0sum[chain][unit] of this wave's tile (wave kk owns tile kk of the top layer) is READ into the registers
// before the step loop and WRITTEN back after it: every chain's sum is then one sequential fp32 chain over its steps, whatever the
// launches a call is cut into (plain segments, the cycles of the round schedule) -- adding a launch's partial sum to the global
// value instead made the result depend on where the launches end.
__device__ __forceinline__ void lean_load_e0(const KParams& P, int kk, const LeanLane& L, f32x4& e0acc) {
    const KLayer& Ly = P.layer[0];
    if (kk >= Ly.ntiles) return;
    const uint32_t npad4 = 4u * (uint32_t)Ly.npad;
    e0acc = gld4s(Ly.spill_e, mul24(L.chain, npad4) + 16u * L.q + 64u * (uint32_t)kk);
}
__device__ __forceinline__ void lean_flush_e0(const KParams& P, int kk, const LeanLane& L, const f32x4& e0acc) {
    const KLayer& Ly = P.layer[0];
    if (kk >= Ly.ntiles) return;
    const uint32_t npad4 = 4u * (uint32_t)Ly.npad;
    gst4s(Ly.spill_e, mul24(L.chain, npad4) + 16u * L.q + 64u * (uint32_t)kk, e0acc);
}

// XL: after the step loop every E wave writes the state rows of its tiles back (the tiles its BWD entries updated: tile = kk + NW i
// of every layer; FWD and BWD entries of a layer hand out tiles alike, rot == 0, chunk starts multiples of NW)
template <int CTT, int NW>
__device__ __forceinline__ void lean_store_x(const KParams& P, const float* lds, int kk, const LeanLane& L) {
    for (int l = 0; l < P.L; ++l) {
        const KLayer& Ly = P.layer[l];
        const uint32_t npad4 = 4u * (uint32_t)Ly.npad;
        for (int tile = kk; tile < Ly.ntiles; tile += NW) {
#pragma unroll
            for (int ct = 0; ct < CTT; ++ct) {
                const uint32_t lb = mul24(L.lrow, 4u * (uint32_t)Ly.ld) + 16u * L.q + 64u * (uint32_t)tile;
                gst4s(Ly.x, mul24(L.chain, npad4) + 16u * L.q + 64u * (uint32_t)tile,
                      *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds + Ly.lds_x) + lb));
            }
        }
    }
}

// ---- BWD entry (layer l): x_l <- x_l - lr (e_l + sign f'(x_l) back) [+ Philox kick], f(x_l new) -> FX_l ---------------
// back = acc from G (GEMM over E_{l+1}, or the read-out back-projection handed over in registers); none for sign == 0.
// ADAM (the MAP warm-up, torch.optim.Adam on x without noise): the moments m, v of the wave's tiles are requested with x,
// in front of the wait for the partner's block -- the generic epilogue loads them behind it, one L2/HBM round trip exposed
// per x update (s_tab: row of the bias-correction table).
template <int CTT, int NW, int NTW, int ACT, bool NOISE, bool ADAM = false, bool XL = false, bool REG = false, class M = Ws2Generic>
__device__ __forceinline__ void lean_bwd(const KParams& P, const KPhase& ph, float* lds, int nt, int kk, const LeanLane& L,
                                         int t, const int* prog_g, int need, int* err, int& dead, int s_tab = 0, float* rx = nullptr,
                                         unsigned row_gen = 0u, const f32x4* racc = nullptr) {
    static_assert(!(NOISE && ADAM), "Adam with the fused kick takes the generic epilogue");
    if (nt <= 0) return;
    const int tstep = REG ? ph.rot : NW;
    const KLayer& Ly = P.layer[ph.layer];
    const int l = ph.layer, n = Ly.n;
    const bool from_g = ((ph.flags & PHF_WS_GEMM) && ph.nkb > 0) || (ph.flags & PHF_WS2_HANDOFF);
    const uint32_t npad4 = 4u * (uint32_t)Ly.npad;
    uint32_t rowb, lrowb, orowb;
#pragma unroll
    for (int ct = 0; ct < CTT; ++ct) {
        rowb = mul24(L.chain, npad4) + 16u * L.q;
        lrowb = mul24(L.lrow, 4u * (uint32_t)Ly.ld) + 16u * L.q;
        orowb = mul24(L.lrow, 4u * (uint32_t)ph.out_ld) + 16u * L.q;
    }
    const float ecoef = Ly.ecoef;
    f32x4 xv[NTW], ev[NTW];
    f32x4 mv[ADAM ? NTW : 1], vv[ADAM ? NTW : 1];
    const char* const e_lds = reinterpret_cast<const char*>(lds + Ly.lds_e);
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const uint32_t tb = 64u * (uint32_t)(ph.tile0 + kk + tstep * (i < nt ? i : 0));
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            if constexpr (XL) {
                xv[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds + Ly.lds_x) + lrowb + tb);
            } else {
#if defined(MCPC_EXP_NOX) || defined(MCPC_EXP_NOELOAD)
            xv[i] = splat(0.5f);
#else
            xv[i] = gld4s(Ly.x, rowb + tb);
#endif
            }
            if constexpr (ADAM) {
                // (moments are kept tile-major: one contiguous KiB per wave access, tile_major_offset in mcpc_kernels.h)
                const uint32_t mb = (mul24(L.chain >> 4, (uint32_t)Ly.ntiles) + (uint32_t)(ph.tile0 + kk + tstep * (i < nt ? i : 0))) * 1024u + 16u * (uint32_t)(L.c + 16 * L.q);
                mv[i] = gld4s(Ly.m, mb);
                vv[i] = gld4s(Ly.v, mb);
            }
#ifdef MCPC_EXP_NOELOAD
            if (l == 0) ev[i] = (xv[i] - splat(0.25f)) * ecoef;
#else
            if (l == 0) {                                                               // e_1 = c_1 (x_1 - mu_1), mu_1 constant
                if constexpr (XL) ev[i] = (xv[i] - *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds + Ly.lds_bias) + lrowb + tb)) * ecoef;
                else ev[i] = (xv[i] - gld4(P.mu1, rowb + tb)) * ecoef;
            }
#endif
            else if constexpr (!ADAM) ev[i] = *reinterpret_cast<const f32x4*>(e_lds + lrowb + tb);
        }
    }
    f32x4 av[NTW];
    if constexpr (REG) {       // (unified-wave kernel: the back-projection arrives in registers, zeros when there is none)
#pragma unroll
        for (int i = 0; i < NTW; ++i) av[i] = racc[i];
        (void)from_g; (void)prog_g; (void)need; (void)err; (void)dead; (void)orowb;
    } else if (from_g) {
        ws_wait_one(prog_g, need, err, dead);
        const char* const src = reinterpret_cast<const char*>(lds + ph.out_lds);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const uint32_t tb = 64u * (uint32_t)(ph.tile0 + kk + tstep * (i < nt ? i : 0));
            av[i] = *reinterpret_cast<const f32x4*>(src + orowb + tb);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NTW; ++i) av[i] = splat(0.f);
    }
    const float sign = ph.sign, lr = P.lr, nscale = P.noise_scale;
    const uint64_t seed = P.seed, step = P.step_base + (uint64_t)t, chain_base = P.chain_base;
    char* const fx_lds = reinterpret_cast<char*>(lds + Ly.lds_a);
    float rmx = 0.f;                       // largest |value| this lane writes of its chain's FX_l row (rowexp_track)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i >= nt) continue;
        const int tile = ph.tile0 + kk + tstep * i;
        const uint32_t tb = 64u * (uint32_t)tile;
        const bool pad_tile = 16 * tile + 16 > n;                  // wave-uniform: only the last tile of a ragged layer
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const f32x4 x = xv[i], back = av[i];
            f32x4 e;
            if constexpr (ADAM) {         // (the error rows are read here, not held across the wait: registers go to m and v)
                if (l == 0) e = ev[i];
                else e = *reinterpret_cast<const f32x4*>(e_lds + lrowb + tb);
            } else {
                e = ev[i];
            }
            const f32x4 g = x_grad4<ACT>(x, e, back, sign);
            f32x4 xn;
            if constexpr (ADAM) {
                f32x4 m = mv[i], v = vv[i];
                adam_moments4(m, v, g, P.omb1, P.beta2, P.omb2);
                const uint32_t mb = (mul24(L.chain >> 4, (uint32_t)Ly.ntiles) + (uint32_t)tile) * 1024u + 16u * (uint32_t)(L.c + 16 * L.q);
                gst4s(Ly.m, mb, m);
                gst4s(Ly.v, mb, v);
                xn = adam_x4(x, m, v, P.adam_coef[2 * s_tab], P.adam_coef[2 * s_tab + 1], P.eps);
            } else {
                xn = x - g * lr;
            }
            if constexpr (NOISE)
                xn = xn + normals4(seed, step, (uint32_t)l, (uint32_t)(chain_base + (uint64_t)L.chain), (uint32_t)(4 * tile + L.q)) * nscale;
            if (pad_tile) zero_padded4(xn, 16 * tile + 4 * L.q, n);
            if constexpr (XL) {
                *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(lds + Ly.lds_x) + lrowb + tb) = xn;
            } else {
#ifndef MCPC_EXP_NOX
            gst4s(Ly.x, rowb + tb, xn);
#endif
            }
            const f32x4 fxn = act4<ACT>(xn);
            *reinterpret_cast<f32x4*>(fx_lds + lrowb + tb) = fxn;                // the next step's GEMMs read f(x_new) from FX_l
            rmx = absmax4(rmx, fxn);
        }
    }
    if (M::has_rx(rx) && ph.o_row >= 0) rowexp_track(rx, ph.o_row, L.c, rmx, row_gen);
}

// ---- HEADF entry (read-out chunk): out = acc + bias, e_o = dL/dout -> ring slot (LDS), loss, spills, output records -----
// XL: bias from LDS; YB (with XL only): the target is 0/1, its words come from LDS and no fp32 target is requested -- a compile-time
// choice, so that the 0/1 case holds no global load at all (see the note on loads under an `if` below).
// YWG (with XL, YB, REG): the target words were requested from global memory by the caller, in front of the row's GEMM (ywreg[i])
template <int CTT, int NW, int NTW, bool XL = false, bool YB = false, bool REG = false, bool YWG = false, class M = Ws2Generic>
__device__ __forceinline__ float lean_headf(const KParams& P, const KPhase& ph, float* lds, int nt, int kk, const LeanLane& L,
                                            int slot, int rec_idx, bool do_energy, const int* prog_g, int need, int* err, int& dead,
                                            bool ybin, float* rx = nullptr, const f32x4* racc = nullptr, unsigned row_gen = 0u,
                                            bool planes_ok = false, const uint32_t* ywreg = nullptr) {
    if (nt <= 0) return 0.f;
    const int tstep = REG ? ph.rot : NW;
    const KHead& H = P.head;
    // unified-wave kernel: a Bernoulli read-out's error goes to LDS as planes (see below; headf_planes is the GEMM side's test too)
    const bool planes = REG && planes_ok;
    const int kind = M::loss_kind(H), n = H.n, mask_start = H.mask_start;
    const uint32_t npad4 = 4u * (uint32_t)H.npad;
    uint32_t rowb, orowb;
#pragma unroll
    for (int ct = 0; ct < CTT; ++ct) {
        rowb = mul24(L.chain, npad4) + 16u * L.q;
        orowb = mul24(L.lrow, 4u * (uint32_t)ph.out_ld) + 16u * L.q;
    }
    f32x4 yv[NTW], bv[NTW];
    uint32_t yw[NTW];                                        // ybin: the word of the bit-packed target that holds this lane's four units
    const uint32_t wrow4 = 4u * (uint32_t)H.ywords;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int tile = ph.tile0 + kk + tstep * (i < nt ? i : 0);
        const uint32_t tb = 64u * (uint32_t)tile;
        if constexpr (XL) {
            bv[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds + H.lds_bias) + 16u * L.q + tb);
        } else {
#ifdef MCPC_EXP_NOELOAD
        bv[i] = splat(0.25f);
#else
        bv[i] = gld4(H.bias, 16u * L.q + tb);
#endif
        }
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            if constexpr (XL && YB && YWG) {
                yv[i] = splat(0.f);
                yw[i] = ywreg[i];                 // (i: a compile-time index after unrolling -- the caller's array stays in registers)
            } else if constexpr (XL && YB) {
                yv[i] = splat(0.f);
                yw[i] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(lds + H.lds_yw) + mul24(L.lrow, wrow4) + 4u * (uint32_t)(tile >> 1));
            } else if constexpr (XL) {
                // (an fp32 target is read from its tile-major image: one contiguous KiB per wave access, like Adam's moments)
                const bool has_y = kind != MCPC_LOSS_NONE;
                yv[i] = gld4s(has_y ? H.ytile : H.bias,
                              has_y ? (mul24(L.chain >> 4, (uint32_t)H.ntiles) + (uint32_t)tile) * 1024u + 16u * (uint32_t)(L.c + 16 * L.q) : 16u * L.q + tb);
                yw[i] = 0u;
            } else {
            // Branch-free on purpose (a load under an `if` makes hipcc join the paths behind `s_waitcnt vmcnt(0)`, which here
            // would also wait for every spill store still in flight): both loads are always issued; the one that is not
            // needed reads a harmless hot address (the bias row again / the word array, which always exists).
#if defined(MCPC_EXP_NOY) || defined(MCPC_EXP_NOELOAD)        // (timing experiment only, wrong results: targets are not loaded)
            yv[i] = splat(0.f); yw[i] = 0u;
#else
            const bool fp32_y = kind != MCPC_LOSS_NONE && !ybin;
            yv[i] = gld4s(fp32_y ? H.y : H.bias, fp32_y ? rowb + tb : 16u * L.q + tb);
            yw[i] = *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(
                (gbytes_t)H.ybits + mul24(L.chain, wrow4) + 4u * (uint32_t)(tile >> 1));
#endif
            }
        }
    }
    char* const eo = reinterpret_cast<char*>(lds + ph.out_lds);
    f32x4 av[NTW];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) av[i] = racc[i];
        (void)prog_g; (void)err; (void)dead;
    } else {
        ws_wait_one(prog_g, need, err, dead);
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const uint32_t cb = 64u * (uint32_t)(kk + tstep * (i < nt ? i : 0));               // column inside the chunk
            av[i] = *reinterpret_cast<const f32x4*>(eo + orowb + cb);
        }
    }
    const float inv_var = H.inv_var;
    float* const spill = M::spills(slot) ? H.spill_e + (size_t)slot * P.Bpad * H.npad : nullptr;
    float* const rec = (rec_idx >= 0 && H.rec_out != nullptr) ? H.rec_out + (size_t)rec_idx * P.B * H.n : nullptr;
    float lsum = 0.f;
    float omx = 0.f;                       // largest |value| this call spills of E_o
    float rmx = 0.f;                       // largest |value| this lane writes of its chain's row of the chunk (rowexp_track)
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        if (i >= nt) continue;
        const int tile = ph.tile0 + kk + tstep * i;
        const uint32_t tb = 64u * (uint32_t)tile, cb = 64u * (uint32_t)(kk + tstep * i);
        const bool inside = 16 * tile >= mask_start && 16 * tile + 16 <= n;        // wave-uniform: every unit of the tile counts
#pragma unroll
        for (int ct = 0; ct < CTT; ++ct) {
            const f32x4 o = av[i] + bv[i];
            f32x4 e = splat(0.f);
            if (kind != MCPC_LOSS_NONE) {
                f32x4 y = yv[i];
                if (ybin) {                                     // units 16 tile + 4 q .. + 3: a nibble of the word
                    const uint32_t nib = yw[i] >> (16u * (uint32_t)(tile & 1) + 4u * (uint32_t)L.q);
                    y.x = (float)(nib & 1u); y.y = (float)((nib >> 1) & 1u); y.z = (float)((nib >> 2) & 1u); y.w = (float)((nib >> 3) & 1u);
                }
                // a padding chain's error is computed like any chain's; only its share of the loss is dropped (livem)
                const float ov[4] = {o.x, o.y, o.z, o.w}, yy[4] = {y.x, y.y, y.z, y.w};
                float ev[4];
                const int u0 = 16 * tile + 4 * L.q;
                if (kind == MCPC_LOSS_GAUSSIAN) {
                    MCPC_LOSS_GAUSSIAN4(ev, ov, yy, inv_var, lsum, inside || ((u0 + r) >= mask_start && (u0 + r) < n), L.livem)
                } else if (do_energy) {       // (a tile whose every unit counts: a wave-uniform branch instead of a select per unit)
                    if (inside) { MCPC_LOSS_BERNOULLI_ENERGY4(ev, ov, yy, lsum, true, L.livem) }
                    else { MCPC_LOSS_BERNOULLI_ENERGY4(ev, ov, yy, lsum, (u0 + r) >= mask_start && (u0 + r) < n, L.livem) }
                } else {
                    MCPC_LOSS_BERNOULLI_GRAD4(ev, ov, yy, inside || ((u0 + r) >= mask_start && (u0 + r) < n))
                }
                e.x = ev[0]; e.y = ev[1]; e.z = ev[2]; e.w = ev[3];
            }
            if (REG && planes) {
                // the chunk as the back-projection's GEMM reads it: per 8 units [h0..h7][m0..m7] (mcpc_gemm_f16.h: b_planes), split here, once,
                // with the constant exponent of a bounded read-out error -- the lane's units 4 q .. 4 q + 3 of the tile are one half of a group
                unsigned h0, m0, h1, m1;
                const float sc = pow2i(headb_fixed_exp(MCPC_LOSS_BERNOULLI, true));
                split2_pair(f32x2{e.x, e.y}, sc, h0, m0);
                split2_pair(f32x2{e.z, e.w}, sc, h1, m1);
                char* const gp = eo + (orowb - 16u * L.q) + cb + 32u * (uint32_t)(L.q >> 1) + 8u * (uint32_t)(L.q & 1);
                *reinterpret_cast<uint2*>(gp) = make_uint2(h0, h1);
                *reinterpret_cast<uint2*>(gp + 16) = make_uint2(m0, m1);
            } else {
                *reinterpret_cast<f32x4*>(eo + orowb + cb) = e;
            }
            rmx = absmax4(rmx, e);
#ifdef MCPC_EXP_SPILL_LINEAR
            if (M::spills(slot)) spill_st4(spill, (uint32_t)P.Bpad * npad4, mul24(L.chain - (uint32_t)L.c, npad4) + 1024u * (uint32_t)tile + 16u * (uint32_t)(L.c + 16 * L.q), mask4(e, L.livem), M::spill_sys(P));
#else
            if (M::spills(slot)) {
                spill_st4(spill, (uint32_t)P.Bpad * npad4,
                          H.spill_tm ? mul24(L.chain - (uint32_t)L.c, npad4) + 1024u * (uint32_t)tile + 16u * (uint32_t)(L.c + 16 * L.q) : rowb + tb,
                          mask4(e, L.livem), M::spill_sys(P));
                omx = absmax4(omx, mask4(e, L.livem));
            }
#endif
            if (rec != nullptr && L.livem) st_unpadded(rec, (int)L.chain, H.n, 16 * tile + 4 * L.q, o);
        }
    }
    if (M::spills(slot)) spill_track(lds + P.lds_spillmax, kSpillIdEo, omx, L.c + 16 * L.q);
    // (a ring slot is reused inside a step: its generation is the entry, `need` = entries completed so far)
    // (the unified-wave kernel keeps the whole e_o row in LDS: its chunks of one step combine under the step's generation)
    if (M::has_rx(rx) && ph.o_row >= 0) rowexp_track(rx, ph.o_row, L.c, rmx, REG ? row_gen : (unsigned)need);
    return lsum;
}

}  // namespace mcpc
