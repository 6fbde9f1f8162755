// The tile of the layer-wise step kernels (mcpc_steps_lw.h) and of the evaluators that share it (mcpc_chain_energy.h, mcpc_pred_err.h,
// mcpc_ancestral.h): one job of the table, and the GEMM of a workgroup's 64 chains x 128 units over it.  Device functions only.
//
// Tile: one workgroup of 4 waves = 64 chains x 128 units; a wave owns 2 unit tiles x 4 chain tiles of 16 x 16 (8 accumulators).  Per
// 32-deep k-block the 64 x 32 block of the B operand (activations / errors: fp32 rows in global memory) is read ONCE per workgroup, scaled
// by its chain row's power of two and split into the two fp16 planes by the thread that loaded it (split8: the PS form of b_planes), and
// handed to all four waves through a double-buffered LDS block of 2 x 64 x 36 floats; the weight fragments of mcpc_pack_kernel stream
// L2 -> registers.  Arithmetic of mcpc_gemm_f16.h, unchanged: per row one exponent from the row's own maximum (a pre-pass of the
// workgroup over its 64 rows), three MFMAs per product ([a_m b_m,] a_m b_h, a_h b_m, a_h b_h; four for K <= 64), k-blocks ascending in one
// fp32 accumulator per tile, un-scaled at the end.  Lanes whose eight k values lie beyond a k range that is not a multiple of 32 stage
// zeros and load nothing (global rows are npad wide: what lies behind them is the next chain's row).
#pragma once
#include "mcpc_kernels.h"

namespace mcpc {

// (the tile's shape -- kLwChains, kLwWaves, kLwUnitTiles, kLwLdsBytes, ... -- and LwJob are the planner's too: mcpc_types.h)

__device__ __forceinline__ LwJob lw_load_job(const LwJob* tbl, int i) {
    typedef __attribute__((address_space(4))) const int cint;
    cint* w = (cint*)(tbl + i);
    LwJob j; j.layer = w[0]; j.ut0 = w[1];
    return j;
}

// acc[i][ct] = sum_k W[tile i][k] B[chain0 + 16 ct + c][k] (fp32), un-scaled.  All 256 threads take part (staging, barriers) whatever nt.
//   A, voff: fragment base and this lane's byte offset of block 0 of the wave's tiles;  Bg: rows [Bpad][ldb], kw valid columns
template <bool MM>
__device__ __forceinline__ void lw_gemm(f32x4 (&acc)[kLwUTW][kLwCTT], const gu32x4* __restrict__ A, const uint32_t (&voff)[kLwUTW], int nkb, int kw,
                                        const float* __restrict__ Bg, int ldb, int chain0, int a_exp, float* stage, int* sexp, int tid, int lane) {
    const int srow = tid >> 2, sg = tid & 3;                  // staging: this thread's chain row and 8-float group of every k-block
    const float* const brow = Bg + (size_t)(chain0 + srow) * ldb + 8 * sg;
    const int last = nkb - 1;
    const bool tail_ok = (uint32_t)(kKB * last + 8 * sg) < (uint32_t)kw;       // does this group of the LAST block lie inside the row?
    // the row's exponent: largest |value| of the row (gemm_row_exp: the same maximum, the same field)
    float mx = 0.f;
#pragma unroll 4
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb < last || tail_ok) {
            const f32x4 a = ld4(brow + kb * kKB), b = ld4(brow + kb * kKB + 4);
            mx = absmax4(absmax4(mx, a), b);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    const int b_exp = scale_exp_for_max(mx);
    if (sg == 0) sexp[srow] = b_exp;
    const float bscale = pow2i(b_exp);
    const f32x4 z4 = splat(0.f);
    f32x4 s0, s1;                                             // the staged values of the NEXT block, in flight
#define LW_STAGE_LOAD(k_)                                                                           \
    do {                                                                                            \
        const int kc_ = (k_) < last ? (k_) : last;                                                  \
        const bool ok_ = kc_ < last || tail_ok;                                                     \
        const float* const src_ = ok_ ? brow + kc_ * kKB : Bg;                                      \
        const f32x4 v0_ = ld4(src_), v1_ = ld4(src_ + 4);                                           \
        s0 = ok_ ? v0_ : z4; s1 = ok_ ? v1_ : z4;                                                   \
    } while (0)
#define LW_STAGE_WRITE(buf_)                                                                        \
    do {                                                                                            \
        const frag_t f_ = split8<false>(s0, s1, bscale);      /* DIET = false: mcpc_gemm_f16.h */                                                   \
        float* const dst_ = stage + (buf_) * (kLwChains * kLwLd) + srow * kLwLd + 8 * sg;           \
        *reinterpret_cast<u32x4*>(dst_) = f_.h; *reinterpret_cast<u32x4*>(dst_ + 4) = f_.m;         \
    } while (0)
    const char __attribute__((address_space(1)))* const Ab = (const char __attribute__((address_space(1)))*)A;
    frag_t fa[kLwUTW];
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) { fa[i].h = *(const gu32x4*)(Ab + voff[i]); fa[i].m = *(const gu32x4*)(Ab + voff[i] + 1024u); }
    LW_STAGE_LOAD(0);
    LW_STAGE_WRITE(0);
    LW_STAGE_LOAD(1);
    __syncthreads();
    const int c = lane & 15, g = lane >> 4;
    const float* const rd = stage + c * kLwLd + 8 * g;
    for (int k = 0; k < nkb; ++k) {
        // the fragments of block k + 1 (the last block re-reads itself: never conditional)
        const int kn = k < last ? k + 1 : last;
        const char __attribute__((address_space(1)))* const Ak = Ab + (size_t)kn * (kFragBlock * 16u);
        frag_t fn[kLwUTW];
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) { fn[i].h = *(const gu32x4*)(Ak + voff[i]); fn[i].m = *(const gu32x4*)(Ak + voff[i] + 1024u); }
        frag_t bs[kLwCTT];
        const float* const rk = rd + (k & 1) * (kLwChains * kLwLd);
#pragma unroll
        for (int ct = 0; ct < kLwCTT; ++ct) bs[ct] = b_planes<true>(ld4(rk + 16 * ct * kLwLd), ld4(rk + 16 * ct * kLwLd + 4), 0.f);
        // per accumulator the products of gemm_fixed in its order: small terms first
#define LW_M(ap_, bp_)                                                                              \
        _Pragma("unroll") for (int ct = 0; ct < kLwCTT; ++ct)                                       \
            _Pragma("unroll") for (int i = 0; i < kLwUTW; ++i) acc[i][ct] = mfma4(fa[i].ap_, bs[ct].bp_, acc[i][ct])
        if constexpr (MM) { LW_M(m, m); }
        LW_M(m, h); LW_M(h, m); LW_M(h, h);
#undef LW_M
        if (k < last) {
            LW_STAGE_WRITE((k + 1) & 1);
            LW_STAGE_LOAD(k + 2);
        }
        __syncthreads();              // block k + 1 is staged; every wave is through with the buffer block k + 2 will take
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) fa[i] = fn[i];
    }
#undef LW_STAGE_LOAD
#undef LW_STAGE_WRITE
    // un-scale: the lane's chains are the rows whose exponents the staging threads published (gemm_unscale)
#pragma unroll
    for (int ct = 0; ct < kLwCTT; ++ct) {
        const float un = pow2i(-a_exp) * pow2i(-sexp[16 * ct + c]);
#pragma unroll
        for (int i = 0; i < kLwUTW; ++i) acc[i][ct] = acc[i][ct] * un;
    }
}

// the wave's tiles of a job and the GEMM over them (nkb == 0: no GEMM, the accumulators stay zero)
__device__ __forceinline__ void lw_job_gemm(f32x4 (&acc)[kLwUTW][kLwCTT], const void* A, int a_tile_stride, int utw, int ntiles, int nkb, int kw,
                                            const float* Bg, int chain0, int a_exp, float* stage, int* sexp, int tid, int lane) {
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i)
#pragma unroll
        for (int ct = 0; ct < kLwCTT; ++ct) acc[i][ct] = splat(0.f);
    if (nkb <= 0) return;
    uint32_t voff[kLwUTW];
#pragma unroll
    for (int i = 0; i < kLwUTW; ++i) {
        const int ut = utw + i < ntiles ? utw + i : ntiles - 1;          // tiles beyond the layer re-read its last tile (never used)
        voff[i] = (uint32_t)(ut * a_tile_stride + lane) * 16u;
    }
    if (nkb <= kShortK) lw_gemm<true>(acc, (const gu32x4*)A, voff, nkb, kw, Bg, kw, chain0, a_exp, stage, sexp, tid, lane);
    else lw_gemm<false>(acc, (const gu32x4*)A, voff, nkb, kw, Bg, kw, chain0, a_exp, stage, sexp, tid, lane);
}

}  // namespace mcpc
