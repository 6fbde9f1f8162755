// The per-chain arithmetic of a Hamiltonian Monte Carlo transition of L leapfrog steps (include/mcpc.h: mcpc_hmc_begin, mcpc_hmc_leap,
// mcpc_hmc_accept): a trajectory of the unit-mass Hamiltonian H(x, p) = F(x) + |p|^2 / 2 with ONE Metropolis decision at its end (Duane
// et al. 1987; Neal 2011).  As in mcpc_mala.h the gradient g = dF/dx and the energy E = F of a state come from the engine (mcpc_run with
// update_x = 0, mcpc_chain_energies); these kernels see them as plain arrays.  A state is n_layers tensors [rows][n_l] fp32,
// 1 <= n_layers <= MCPC_MAX_LATENT.  With eps = sqrt(2 lr) and h = eps / 2 a trajectory from (x, g) is
//     BEGIN    p = xi                 q = p - h g            x_1 = x + eps q                       (q: the momentum at the half step)
//     LEAP     q = q - eps g_t        x_{t+1} = x_t + eps q                                         (L - 1 times, g_t the gradient at x_t)
//     ACCEPT   p' = q - h g_L         log_alpha = H(x, p) - H(x_L, p')
// With L = 1 the end point x + eps xi - (eps^2 / 2) g = x - lr g + sqrt(2 lr) xi is the MALA proposal at noise_var = 2 and log_alpha is
// MALA's: the scheme generalises mcpc_mala.h, it does not replace it.
//
// ELEMENTS, fp32, EVERY OPERATION ROUNDED SEPARATELY (nothing is contracted into an fma: `#pragma clang fp contract(off)`).  The host
// forms eps = (float)sqrt(2.0 * lr) in double and rounds it once; h = 0.5f * eps is exact.
//     BEGIN    p = xi        q = fl(p - fl(h g))        x_out = fl(x + fl(eps q))
//     LEAP     q = fl(q - fl(eps g_t))                  x_t = fl(x_t + fl(eps q))                   (in place)
//     ACCEPT   p' = fl(q - fl(h g_t))
// with xi the normal of (seed, step, layer l, chain_base + row, unit): normals4 of mcpc_device.h, what mcpc_philox_normals returns and
// the very normals mcpc_mala_propose takes at that (seed, step).  tests/hmc_cases.py restates all three bit for bit.
//
// KINETIC ENERGY, per chain, fp64: K = 0.5 * sum_u (double)p_u (double)p_u (the square of an fp32 value is exact in fp64).  LANE `lane`
// of the chain's wave owns the groups of four units lane, lane + 64, ... of every layer and adds their squares to its ONE sum in
// ascending order: layers, then groups, then the units of a group.  The 64 lanes are summed by a butterfly (xor 32, 16, 8, 4, 2, 1),
// exactly as mcpc_mala_accept sums; then one product by 0.5.  BEGIN writes K0 of p, ACCEPT forms K1 of p' and
//     log_alpha = (E - E_t) + (K0 - K1)                              (two differences and one sum, each rounded)
//     u = ((w >> 8) + 1) 2^-24,  w = word 0 of philox4x32_10(chain_base + row, 0xFD << 24, step lo, step hi; seed)
//     accept = log(u) < log_alpha                                    (fp64 log; a NaN log_alpha compares false: the chain rejects)
// Layer 0xFD is outside every layer in use: the normals and mcpc_sample_prior take 0 .. MCPC_MAX_LATENT, mcpc_smc_ancestors 0xFE and
// mcpc_mala_accept 0xFF, so no Philox word is consumed twice.
// An accepted chain's x, g and E are overwritten with x_t, g_t, E_t (each lane copies the units it read); a rejected chain is not
// written.  x_t, g_t, q and K0 are never written by ACCEPT.
//
// That order involves the chain's own values only: a row's result does not depend on `rows` or on the other rows, a NaN or Inf stays
// in its chain, and two runs are bitwise equal.  No atomics, no LDS, no workspace.  The early exits are wave-uniform and the kernels
// have no barrier.  An element of LEAP is read and written by the same lane.
// A workgroup is four waves, a wave one chain, as in mcpc_mala.h: these are latency kernels.
// Bounds: a lane touches unit u of row r only when r < rows and u < n_l.  Rows of odd width are not 16-byte aligned, so the loads are
// scalar.  All offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_device.h"
#include "mcpc_mala.h"

namespace mcpc {

constexpr uint32_t kHmcLayer = 0xFDu;   // the layer index of the decision's uniform

struct HmcParams {
    float* x[MCPC_MAX_LATENT];          // begin: read.  accept: overwritten for an accepted chain
    float* g[MCPC_MAX_LATENT];
    float* xt[MCPC_MAX_LATENT];         // begin: x_out.  leap: in place.  accept: read
    const float* gt[MCPC_MAX_LATENT];   // leap, accept: the gradient at xt
    float* q[MCPC_MAX_LATENT];          // begin: q_out.  leap: in place.  accept: read
    int32_t n[MCPC_MAX_LATENT];
    double* E;
    const double* Et;
    double* K0;                         // begin: written.  accept: read
    double* diag;                       // [rows][3] or nullptr
    int32_t* n_accepted;                // [rows] or nullptr
    int64_t rows;
    int32_t n_layers;
    float eps, h;
    uint64_t seed, step, chain_base;
};

// fl(a - fl(c b)): the momentum's half and full steps
__device__ __forceinline__ float hmc_kick(float a, float c, float b) {
#pragma clang fp contract(off)
    const float t = c * b;
    return a - t;
}

// fl(x + fl(eps q)): the position's step
__device__ __forceinline__ float hmc_drift(float x, float eps, float q) {
#pragma clang fp contract(off)
    const float t = eps * q;
    return x + t;
}

// the butterfly of mcpc_mala_accept, then the one product by 0.5
__device__ __forceinline__ double hmc_kinetic(double s) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return 0.5 * s;
}

__global__ __launch_bounds__(64 * kMalaWaves) void mcpc_hmc_begin_kernel(const HmcParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kMalaWaves + wave;
    if (r >= P.rows) return;                                            // wave-uniform; the kernel has no barrier
    const uint32_t chain = (uint32_t)(P.chain_base + (uint64_t)r);
    double s = 0.0;
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const int64_t base = r * (int64_t)n;
        const float* x = P.x[l] + base;
        const float* g = P.g[l] + base;
        float* q = P.q[l] + base;
        float* xt = P.xt[l] + base;
        for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
            const f32x4 z = normals4(P.seed, P.step, (uint32_t)l, chain, (uint32_t)(u0 >> 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u0 + j < n) {
#pragma clang fp contract(off)
                    const float p = mala_pick(z, j);
                    const float qq = hmc_kick(p, P.h, g[u0 + j]);
                    q[u0 + j] = qq;
                    xt[u0 + j] = hmc_drift(x[u0 + j], P.eps, qq);
                    const double pp = (double)p * (double)p;
                    s = s + pp;
                }
            }
        }
    }
    const double K0 = hmc_kinetic(s);
    if (lane == 0) P.K0[r] = K0;
}

__global__ __launch_bounds__(64 * kMalaWaves) void mcpc_hmc_leap_kernel(const HmcParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kMalaWaves + wave;
    if (r >= P.rows) return;                                            // wave-uniform; the kernel has no barrier
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const int64_t base = r * (int64_t)n;
        const float* gt = P.gt[l] + base;
        float* q = P.q[l] + base;
        float* xt = P.xt[l] + base;
        for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u0 + j < n) {
                    const float qq = hmc_kick(q[u0 + j], P.eps, gt[u0 + j]);
                    q[u0 + j] = qq;
                    xt[u0 + j] = hmc_drift(xt[u0 + j], P.eps, qq);
                }
            }
        }
    }
}

__global__ __launch_bounds__(64 * kMalaWaves) void mcpc_hmc_accept_kernel(const HmcParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kMalaWaves + wave;
    if (r >= P.rows) return;                                            // wave-uniform; the kernel has no barrier
    const uint32_t chain = (uint32_t)(P.chain_base + (uint64_t)r);
    double s = 0.0;
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const int64_t base = r * (int64_t)n;
        const float* gt = P.gt[l] + base;
        const float* q = P.q[l] + base;
        for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u0 + j < n) {
#pragma clang fp contract(off)
                    const float p = hmc_kick(q[u0 + j], P.h, gt[u0 + j]);
                    const double pp = (double)p * (double)p;
                    s = s + pp;
                }
            }
        }
    }
    const double K1 = hmc_kinetic(s);
    const double E = P.E[r], Et = P.Et[r], K0 = P.K0[r];
    double log_alpha;
    {
#pragma clang fp contract(off)
        const double de = E - Et;
        const double dk = K0 - K1;
        log_alpha = de + dk;
    }
    uint32_t w[4];
    philox4x32_10(chain, kHmcLayer << 24, (uint32_t)P.step, (uint32_t)(P.step >> 32), (uint32_t)P.seed, (uint32_t)(P.seed >> 32), w);
    const float u = (float)((w[0] >> 8) + 1u) * 0x1p-24f;
    const bool accept = log((double)u) < log_alpha;                     // false for a NaN
    if (lane == 0) {
        if (P.diag) {
            double* dg = P.diag + r * 3;
            dg[0] = log_alpha; dg[1] = (double)u; dg[2] = accept ? 1.0 : 0.0;
        }
        if (P.n_accepted && accept) P.n_accepted[r] += 1;
        if (accept) P.E[r] = Et;
    }
    if (!accept) return;                                                // wave-uniform
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const int64_t base = r * (int64_t)n;
        float *x = P.x[l] + base, *g = P.g[l] + base;
        const float *xt = P.xt[l] + base, *gt = P.gt[l] + base;
        for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (u0 + j < n) { x[u0 + j] = xt[u0 + j]; g[u0 + j] = gt[u0 + j]; }
        }
    }
}

}  // namespace mcpc
