// The per-chain arithmetic of a Metropolis-adjusted Langevin step (include/mcpc.h: mcpc_mala_propose, mcpc_mala_accept): the proposal
// and the accept / reject decision that make a Langevin transition leave its target exactly invariant (Roberts & Tweedie 1996).  The
// gradient g = dF/dx and the energy E = F of a state come from the engine (mcpc_run with update_x = 0, mcpc_chain_energies); these
// kernels see them as plain arrays.  A state is n_layers tensors [rows][n_l] fp32, 1 <= n_layers <= MCPC_MAX_LATENT.
//
// PROPOSE, per element, fp32, EVERY OPERATION ROUNDED SEPARATELY (nothing is contracted into an fma: `#pragma clang fp contract(off)`):
//     p = fl(lr * g)    a = fl(x - p)    n = fl(s * xi)    x' = fl(a + n)            lr, s = sqrt(noise_var * lr) rounded to fp32
// with xi the normal of (seed, step, layer l, chain_base + row, unit): normals4 of mcpc_device.h, what mcpc_philox_normals returns and
// what a fused Langevin step at the same (seed, step) consumes.  The step kernels write `x - g * lr` and `xn + z * nscale` and leave
// the contraction to the compiler; here the four roundings are spelled out so that tests/mala_cases.py can restate them bit for bit.
//
// ACCEPT, per chain, fp64 from the fp32 inputs, every operation rounded separately.  For unit u of layer l
//     d = x - x'            a = d + lr g'            b = (x' - x) + lr g            (x' - x is -d bit for bit)
//     sa += a a             sb += b b
// LANE `lane` of the chain's wave owns the groups of four units lane, lane + 64, ... of every layer and adds their terms to its ONE sa
// and ONE sb in ascending order: layers, then groups, then the units of a group.  The 64 lanes are summed by a butterfly (xor 32, 16,
// 8, 4, 2, 1; an addition is commutative, so every lane ends with the same bits).  Then
//     log_alpha = (E - E') - (sa - sb) / (2 noise_var lr)          (the denominator is formed on the host: 2 noise_var exact, one product)
//     u = ((w >> 8) + 1) 2^-24,  w = word 0 of philox4x32_10(chain_base + row, 0xFF << 24, step lo, step hi; seed)
//     accept = log(u) < log_alpha                                   (fp64 log; a NaN log_alpha compares false: the chain rejects)
// That order involves the chain's own values only: a row's result does not depend on `rows` or on the other rows, and two runs are
// bitwise equal.  No atomics, no LDS, no workspace.  Layer 0xFF is outside every layer the normals and mcpc_sample_prior use
// (layers 0 .. MCPC_MAX_LATENT), so no Philox word is consumed twice (mcpc_smc.h takes 0xFE, mcpc_hmc.h 0xFD).
// An accepted chain's x, g and E are overwritten with x', g', E' (each lane copies the units it read); a rejected chain is not
// written.  x_next, when asked for, is PROPOSE at step + 1 from the selected (x, g), formed from the registers the copy holds.
//
// A workgroup is four waves, a wave one chain: a network's latent units are a few hundred to about 1300, 2 to 6 groups per lane, so
// this is a latency kernel.  Narrow networks leave lanes idle; the launch is the cost there, not the lanes.
// Bounds: a lane touches unit u of row r only when r < rows and u < n_l.  Rows of odd width are not 16-byte aligned, so the loads are
// scalar; the four loads of a group are independent and in flight together.  All offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_device.h"

namespace mcpc {

constexpr int kMalaWaves = 4;           // waves (chains) of a workgroup
constexpr uint32_t kMalaLayer = 0xFFu;  // the layer index of the accept step's uniform

struct MalaParams {
    float* x[MCPC_MAX_LATENT];          // propose: read.  accept: overwritten for an accepted chain
    float* g[MCPC_MAX_LATENT];
    const float* xp[MCPC_MAX_LATENT];   // accept: the proposal and its gradient
    const float* gp[MCPC_MAX_LATENT];
    float* out[MCPC_MAX_LATENT];        // propose: x'.  accept: x_next (has_out)
    int32_t n[MCPC_MAX_LATENT];
    double* E;
    const double* Ep;
    double* diag;                       // [rows][3] or nullptr
    int32_t* n_accepted;                // [rows] or nullptr
    int64_t rows;
    int32_t n_layers, has_out;
    float lr, s;
    double lr_d, denom;                 // accept: lr as given, 2 noise_var lr
    uint64_t seed, step, chain_base;
};

// x' of one element: four roundings
__device__ __forceinline__ float mala_move(float x, float g, float z, float lr, float s) {
#pragma clang fp contract(off)
    const float p = lr * g;
    const float a = x - p;
    const float n = s * z;
    return a + n;
}

__device__ __forceinline__ float mala_pick(const f32x4& z, int j) { return j == 0 ? z.x : (j == 1 ? z.y : (j == 2 ? z.z : z.w)); }

__global__ __launch_bounds__(64 * kMalaWaves) void mcpc_mala_propose_kernel(const MalaParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kMalaWaves + wave;
    if (r >= P.rows) return;                                            // wave-uniform; the kernel has no barrier
    const uint32_t chain = (uint32_t)(P.chain_base + (uint64_t)r);
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const int64_t base = r * (int64_t)n;
        const float* x = P.x[l] + base;
        const float* g = P.g[l] + base;
        float* out = P.out[l] + base;
        for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
            const f32x4 z = normals4(P.seed, P.step, (uint32_t)l, chain, (uint32_t)(u0 >> 2));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (u0 + j < n) out[u0 + j] = mala_move(x[u0 + j], g[u0 + j], mala_pick(z, j), P.lr, P.s);
        }
    }
}

__global__ __launch_bounds__(64 * kMalaWaves) void mcpc_mala_accept_kernel(const MalaParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kMalaWaves + wave;
    if (r >= P.rows) return;                                            // wave-uniform; the kernel has no barrier
    const uint32_t chain = (uint32_t)(P.chain_base + (uint64_t)r);
    double sa = 0.0, sb = 0.0;
    {
#pragma clang fp contract(off)
        for (int l = 0; l < P.n_layers; ++l) {
            const int32_t n = P.n[l];
            const int64_t base = r * (int64_t)n;
            const float *x = P.x[l] + base, *g = P.g[l] + base, *xp = P.xp[l] + base, *gp = P.gp[l] + base;
            for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
                float vx[4], vg[4], vxp[4], vgp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool ok = u0 + j < n;
                    const int32_t u = ok ? u0 + j : 0;                   // (n >= 1: unit 0 of the row exists; the value is not used)
                    vx[j] = x[u]; vg[j] = g[u]; vxp[j] = xp[u]; vgp[j] = gp[u];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (u0 + j < n) {
                        const double d = (double)vx[j] - (double)vxp[j];
                        const double e = (double)vxp[j] - (double)vx[j];
                        const double ta = P.lr_d * (double)vgp[j];
                        const double tb = P.lr_d * (double)vg[j];
                        const double a = d + ta;
                        const double b = e + tb;
                        const double aa = a * a;
                        const double bb = b * b;
                        sa = sa + aa;
                        sb = sb + bb;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sa += __shfl_xor(sa, m, 64);
        sb += __shfl_xor(sb, m, 64);
    }
    const double E = P.E[r], Ep = P.Ep[r];
    double log_alpha;
    {
#pragma clang fp contract(off)
        const double de = E - Ep;
        const double ds = sa - sb;
        const double q = ds / P.denom;
        log_alpha = de - q;
    }
    uint32_t w[4];
    philox4x32_10(chain, kMalaLayer << 24, (uint32_t)P.step, (uint32_t)(P.step >> 32), (uint32_t)P.seed, (uint32_t)(P.seed >> 32), w);
    const float u = (float)((w[0] >> 8) + 1u) * 0x1p-24f;
    const bool accept = log((double)u) < log_alpha;                     // false for a NaN
    if (lane == 0) {
        if (P.diag) {
            double* dg = P.diag + r * 3;
            dg[0] = log_alpha; dg[1] = (double)u; dg[2] = accept ? 1.0 : 0.0;
        }
        if (P.n_accepted && accept) P.n_accepted[r] += 1;
        if (accept) P.E[r] = Ep;
    }
    if (!accept && !P.has_out) return;                                  // wave-uniform
    for (int l = 0; l < P.n_layers; ++l) {
        const int32_t n = P.n[l];
        const int64_t base = r * (int64_t)n;
        float *x = P.x[l] + base, *g = P.g[l] + base;
        const float *xp = P.xp[l] + base, *gp = P.gp[l] + base;
        for (int32_t u0 = 4 * lane; u0 < n; u0 += 256) {
            float sx[4], sg[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t uu = u0 + j < n ? u0 + j : 0;
                sx[j] = accept ? xp[uu] : x[uu];
                sg[j] = accept ? gp[uu] : g[uu];
            }
            if (accept) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (u0 + j < n) { x[u0 + j] = sx[j]; g[u0 + j] = sg[j]; }
            }
            if (P.has_out) {
                float* out = P.out[l] + base;
                const f32x4 z = normals4(P.seed, P.step + 1, (uint32_t)l, chain, (uint32_t)(u0 >> 2));
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (u0 + j < n) out[u0 + j] = mala_move(sx[j], sg[j], mala_pick(z, j), P.lr, P.s);
            }
        }
    }
}

inline dim3 mala_grid(int64_t rows) { return dim3((unsigned)((rows + kMalaWaves - 1) / kMalaWaves)); }

}  // namespace mcpc
