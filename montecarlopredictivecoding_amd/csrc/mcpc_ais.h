// The log-weight increment of annealed importance sampling (include/mcpc.h: mcpc_ais_increment): for every chain r, from its last latent
// layer x_r, the UNSCALED read-out (W, bias) and its target row y_r,
//   o_u     = bias_u + sum_k f(x_rk) W_uk
//   l(a)    = sum over u >= mask_start of  Bernoulli: softplus(a o_u) - y_ru a o_u      Gaussian: (0.5 / var) (a o_u - y_ru)^2
//   logw[r] = (accumulate ? logw[r] : 0) + c0 l(a0) - c1 l(a1)
// i.e. log f_k(x) - log f_{k-1}(x) between two rungs of a ladder from the prior to the posterior (montecarlopredictivecoding_amd/ais.py):
// the Bernoulli ladder scales the logits (a), the Gaussian ladder scales the loss (c).  A side whose c is exactly 0 is not evaluated.
//
// Everything is fp64.  The contraction runs on v_mfma_f64_16x16x4_f64 with the operands converted from fp32 on load (mcpc_loglik.h's
// scheme: lane (m = lane & 15, q = lane >> 4) loads columns k0 + 4 q + (0..3) of its row with one 16-byte load and MFMA j of four
// contracts columns k0 + 4 q + j): f(x) is formed in fp64 from the fp32 x, the products are exact for ReLU and identity and rounded once
// for tanh, so the roundings are the additions.  The A operand is the chains, the B operand the read-out's rows: lane (m, q) holds
// D[chain q + 4 reg][output m], sees ONE output column per tile and four chains.
//
// A workgroup is 16 chains and kAisWaves waves.  The 16-output tiles from mask_start's on are taken kAisTiles at a time (a GROUP: the x
// fragment is loaded and activated once for the four tiles, which matters for tanh); wave w takes groups w, w + kAisWaves, ... in
// ascending order.  The epilogue turns each D value into c0 t(a0) - c1 t(a1) and adds it to the lane's sum of that chain; at the end the
// 16 lanes of a chain are summed by a butterfly (xor 8, 4, 2, 1), the waves' sums go through LDS and are added in ascending wave order,
// then to the old logw.  One fixed order that holds the chain's own values only: a row's result depends on that row, W, bias and the
// scalars alone -- not on `rows`, on the other rows or on where in a tile the row lies -- and two runs are bitwise equal.  No atomics,
// no workspace.
//
// Bounds: rows beyond `rows`, outputs beyond n_out and columns beyond the width contribute exact zeros and READ NOTHING BEYOND THEIR
// BUFFER (mcpc_loglik.h's ll_load4: such a lane is pointed at element 0 of its own buffer and discards what it gets).  An output below
// mask_start or beyond n_out is excluded by its index, never by its value.  All offsets are 64-bit.
//
// Non-finite values: a NaN or Inf in a chain's row reaches the MFMA results of that row alone (the A operand); every other row keeps its
// bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_loglik.h"        // ll_d4, ll_load4, ll_softplus

namespace mcpc {

constexpr int kAisWaves = 4;    // waves of a workgroup; they share 16 chains and split the groups of output tiles
constexpr int kAisTiles = 4;    // 16-output tiles per group: accumulators that share one activated x fragment

struct AisParams {
    const float* x;             // [rows][width]
    const float* W;             // [n_out][width]
    const float* bias;          // [n_out] or nullptr
    const float* y;             // [rows][n_out]
    double* logw;               // [rows]
    int64_t rows;
    int32_t width, n_out, mask_start, gauss, accumulate;
    int32_t tile_begin, n_groups;       // the first output tile that holds an active column; groups of kAisTiles tiles from there
    double a0, c0, a1, c1, half_inv_var;
};

template <int kAct>
__device__ __forceinline__ double ais_act(float v) {
    const double d = (double)v;
    if (kAct == MCPC_ACT_RELU) return d < 0.0 ? 0.0 : d;              // a NaN stays a NaN
    if (kAct == MCPC_ACT_TANH) return tanh(d);
    return d;
}

// one output's term at scale a: Bernoulli softplus(a o) - y a o, Gaussian (0.5 / var) (a o - y)^2
__device__ __forceinline__ double ais_term(double a, double o, double y, bool gauss, double hiv) {
    const double z = a * o;
    if (gauss) { const double d = z - y; return hiv * (d * d); }
    return ll_softplus(z) - y * z;
}

template <int kAct, bool kVec>
__global__ __launch_bounds__(64 * kAisWaves) void mcpc_ais_kernel(const AisParams P) {
    __shared__ double part[kAisWaves][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * 16;
    const int32_t width = P.width, n_out = P.n_out;
    const float* xrow = r0 + m < P.rows ? P.x + (r0 + m) * (int64_t)width : nullptr;
    const bool gauss = P.gauss != 0, side0 = P.c0 != 0.0, side1 = P.c1 != 0.0;

    double s[4] = {0.0, 0.0, 0.0, 0.0};                                 // the lane's sums of chains r0 + q + 4 reg
    for (int32_t g = wave; g < P.n_groups; g += kAisWaves) {            // wave-uniform
        const int32_t u0 = (P.tile_begin + g * kAisTiles) * 16;
        const float* wrow[kAisTiles];
#pragma unroll
        for (int t = 0; t < kAisTiles; ++t) {
            const int64_t u = (int64_t)u0 + 16 * t + m;
            wrow[t] = u < n_out ? P.W + u * (int64_t)width : nullptr;
        }
        ll_d4 acc[kAisTiles];
#pragma unroll
        for (int t = 0; t < kAisTiles; ++t) acc[t] = ll_d4{0.0, 0.0, 0.0, 0.0};
        float xn[4], wn[kAisTiles][4];
        auto load = [&](int32_t k0) {
            const int32_t c = k0 + 4 * q;
            ll_load4<kVec>(xrow, P.x, c, width, xn);
#pragma unroll
            for (int t = 0; t < kAisTiles; ++t) ll_load4<kVec>(wrow[t], P.W, c, width, wn[t]);
        };
        load(0);
        for (int32_t k0 = 0; k0 < width; k0 += 16) {
            double fx[4];
            float wc[kAisTiles][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) fx[j] = ais_act<kAct>(xn[j]);
#pragma unroll
            for (int t = 0; t < kAisTiles; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) wc[t][j] = wn[t][j];
            load(k0 + 16);                                               // the next chunk, in flight under the MFMAs (past the width: zeros)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < kAisTiles; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fx[j], (double)wc[t][j], acc[t], 0, 0, 0);
        }
        // C/D layout of the f64 form: col (output) = lane & 15, row (chain) = (lane >> 4) + 4 reg
#pragma unroll
        for (int t = 0; t < kAisTiles; ++t) {
            const int64_t u = (int64_t)u0 + 16 * t + m;
            const bool u_ok = u < n_out && u >= P.mask_start;
            const double b = P.bias ? (double)P.bias[u < n_out ? u : 0] : 0.0;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t row = r0 + q + 4 * reg;
                const bool ok = u_ok && row < P.rows;
                const double yv = (double)P.y[ok ? row * (int64_t)n_out + u : 0];
                const double o = acc[t][reg] + b;
                double v = 0.0;
                if (side0) v = P.c0 * ais_term(P.a0, o, yv, gauss, P.half_inv_var);
                if (side1) v -= P.c1 * ais_term(P.a1, o, yv, gauss, P.half_inv_var);
                s[reg] += ok ? v : 0.0;
            }
        }
    }
    // the 16 lanes (outputs) of a chain: one butterfly, then the waves in ascending order
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
        for (int d = 8; d >= 1; d >>= 1) s[reg] += __shfl_xor(s[reg], d, 64);
        if (m == 0) part[wave][q + 4 * reg] = s[reg];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int64_t row = r0 + threadIdx.x;
        if (row < P.rows) {
            double tot = part[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kAisWaves; ++w) tot += part[w][threadIdx.x];
            P.logw[row] = (P.accumulate ? P.logw[row] : 0.0) + tot;
        }
    }
}

template <int kAct>
inline void ais_launch(const AisParams& P, bool vec, hipStream_t stream) {
    const dim3 grid((unsigned)((P.rows + 15) / 16)), block(64 * kAisWaves);
    if (vec) hipLaunchKernelGGL((mcpc_ais_kernel<kAct, true>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((mcpc_ais_kernel<kAct, false>), grid, block, 0, stream, P);
}

inline void ais_dispatch(int32_t act, const AisParams& P, hipStream_t stream) {
    const bool vec = P.width % 4 == 0 && (uintptr_t)P.x % 16 == 0 && (uintptr_t)P.W % 16 == 0;
    if (act == MCPC_ACT_RELU) ais_launch<MCPC_ACT_RELU>(P, vec, stream);
    else if (act == MCPC_ACT_TANH) ais_launch<MCPC_ACT_TANH>(P, vec, stream);
    else ais_launch<MCPC_ACT_IDENTITY>(P, vec, stream);
}

}  // namespace mcpc
