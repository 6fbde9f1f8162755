// The per-element arithmetic of a Langevin / PC inference step, on the four units a lane holds of one chain (C layout of the MFMA tiles).
// Every step kernel form -- barrier, in-place (generic and specialised), unified-wave, layer-wise -- calls these and nothing else for it, so
// their trajectories, energies and Hebbian sums agree bitwise by construction (tests/test_step_math_single_definition.py).
// No addressing, no loads or stores, no KParams: what counts as "on" or "live" is the caller's business and arrives as a predicate.
#pragma once
#include "mcpc_device.h"
#include "../../include/mcpc.h"

namespace mcpc {

// ---- activations ------------------------------------------------------------------------------------------------------------------------
template <int ACT> __device__ __forceinline__ float actf(float x) {
    if constexpr (ACT == MCPC_ACT_RELU) return fmaxf(x, 0.0f);
    else if constexpr (ACT == MCPC_ACT_TANH) return tanh_f(x);
    else return x;
}
template <int ACT> __device__ __forceinline__ float actd(float x, float fx) {
    if constexpr (ACT == MCPC_ACT_RELU) return x > 0.0f ? 1.0f : 0.0f;
    else if constexpr (ACT == MCPC_ACT_TANH) return 1.0f - fx * fx;
    else return 1.0f;
}
template <int ACT> __device__ __forceinline__ f32x4 act4(f32x4 x) {
    f32x4 r;
    r.x = actf<ACT>(x.x); r.y = actf<ACT>(x.y); r.z = actf<ACT>(x.z); r.w = actf<ACT>(x.w);
    return r;
}

// ---- prediction error of a latent layer: d = x - mu, e = c d, and the layer's energy term of these four units -----------------------------
__device__ __forceinline__ f32x4 pc_error4(f32x4 x, f32x4 mu, float ecoef, f32x4& d) {
    d = x - mu;
    return d * ecoef;
}
__device__ __forceinline__ float pc_energy4(f32x4 d, float ecoef) {
    const f32x4 dd = d * d;
    return 0.5f * ecoef * (dd.x + dd.y + dd.z + dd.w);
}

// ---- x update ---------------------------------------------------------------------------------------------------------------------------
// g = e + sign * f'(x) * back
template <int ACT> __device__ __forceinline__ f32x4 x_grad4(f32x4 x, f32x4 e, f32x4 back, float sign) {
    f32x4 g;
    g.x = e.x + sign * actd<ACT>(x.x, actf<ACT>(x.x)) * back.x;
    g.y = e.y + sign * actd<ACT>(x.y, actf<ACT>(x.y)) * back.y;
    g.z = e.z + sign * actd<ACT>(x.z, actf<ACT>(x.z)) * back.z;
    g.w = e.w + sign * actd<ACT>(x.w, actf<ACT>(x.w)) * back.w;
    return g;
}
// torch.optim.Adam's single-tensor path (adam_m, adam_v, adam_x in mcpc_device.h): lerp_, mul_ / addcmul_, then sqrt / bias2 + eps and
// addcdiv_.  Two halves, so that a caller stores the new moments between them.
__device__ __forceinline__ void adam_moments4(f32x4& m, f32x4& v, f32x4 g, float omb1, float beta2, float omb2) {
    m.x = adam_m(m.x, g.x, omb1); m.y = adam_m(m.y, g.y, omb1); m.z = adam_m(m.z, g.z, omb1); m.w = adam_m(m.w, g.w, omb1);
    v.x = adam_v(v.x, g.x, beta2, omb2); v.y = adam_v(v.y, g.y, beta2, omb2); v.z = adam_v(v.z, g.z, beta2, omb2); v.w = adam_v(v.w, g.w, beta2, omb2);
}
__device__ __forceinline__ f32x4 adam_x4(f32x4 x, f32x4 m, f32x4 v, float nss, float bc2s, float eps) {
    f32x4 xn;
    xn.x = adam_x(x.x, m.x, v.x, nss, bc2s, eps);
    xn.y = adam_x(x.y, m.y, v.y, nss, bc2s, eps);
    xn.z = adam_x(x.z, m.z, v.z, nss, bc2s, eps);
    xn.w = adam_x(x.w, m.w, v.w, nss, bc2s, eps);
    return xn;
}
// padded units (u0 .. u0 + 3 at or beyond n) stay exactly zero: their gradient is zero, only the noise must be masked
__device__ __forceinline__ void zero_padded4(f32x4& xn, int u0, int n) {
    if (u0 + 0 >= n) xn.x = 0.f;
    if (u0 + 1 >= n) xn.y = 0.f;
    if (u0 + 2 >= n) xn.z = 0.f;
    if (u0 + 3 >= n) xn.w = 0.f;
}

// ---- read-out losses ---------------------------------------------------------------------------------------------------------------------
// e = dloss / dout of the four units: the derivative where ON holds, exactly zero elsewhere -- selects, not products: whatever a padding
// chain or a masked unit holds.  The loss itself is added to lsum, unit by unit, where ON && COUNTS.
//   ev, ov, yv   float[4]: error (written), output, target          ON, COUNTS   expressions of the call site; ON may use r = 0 .. 3
// Statement macros on purpose, the one exception in this header.  As __forceinline__ functions -- on float4s with the predicate as a
// lambda, as an array or as arguments, or per unit with the loops left at the call sites -- the same operations compiled to other code in
// EVERY step kernel (branches became selects, the two Bernoulli forms were merged), 0.5 to 1.9 % slower on four of the five kernel
// families, and `sigmoid - y` was no longer contracted into one fma where the lean epilogues inline it: their trajectories left the
// other forms' (profiles/step_math_ab.txt).  Textually the compiler sees what it saw when each epilogue carried its own copy.
#define MCPC_LOSS_GAUSSIAN4(ev, ov, yv, inv_var, lsum, ON, COUNTS)                                                                 \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                \
        const bool on = (ON);                                                                                                      \
        const float dlt = ov[r] - yv[r];                                                                                           \
        ev[r] = on ? inv_var * dlt : 0.f;                                                                                          \
        lsum += (on && (COUNTS)) ? 0.5f * inv_var * dlt * dlt : 0.f;                                                               \
    }
// Bernoulli read-out (BCE with logits) with its energy: sigmoid and loss term from one exponential
#define MCPC_LOSS_BERNOULLI_ENERGY4(ev, ov, yv, lsum, ON, COUNTS)                                                                  \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                \
        const bool on = (ON);                                                                                                      \
        float sg, bc;                                                                                                              \
        sigmoid_bce_f(ov[r], yv[r], sg, bc);                                                                                       \
        ev[r] = on ? sg - yv[r] : 0.f;                                                                                             \
        lsum += (on && (COUNTS)) ? bc : 0.f;                                                                                       \
    }
// the same error when the step records no energy (sigmoid_f: the same arithmetic, so recording the loss never changes a trajectory)
#define MCPC_LOSS_BERNOULLI_GRAD4(ev, ov, yv, ON)                                                                                  \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                \
        const bool on = (ON);                                                                                                      \
        ev[r] = on ? sigmoid_f(ov[r]) - yv[r] : 0.f;                                                                               \
    }
// the read-out's error e (an f32x4 lvalue) for outputs o and targets y under loss `kind` (not MCPC_LOSS_NONE)
#define MCPC_READOUT_LOSS4(e, o, y, kind, do_energy, inv_var, lsum, ON, COUNTS)                                                    \
    do {                                                                                                                           \
        const float ov[4] = {o.x, o.y, o.z, o.w}, yv[4] = {y.x, y.y, y.z, y.w};                                                    \
        float ev[4];                                                                                                               \
        if (kind == MCPC_LOSS_GAUSSIAN) { MCPC_LOSS_GAUSSIAN4(ev, ov, yv, inv_var, lsum, ON, COUNTS) }                             \
        else if (do_energy) { MCPC_LOSS_BERNOULLI_ENERGY4(ev, ov, yv, lsum, ON, COUNTS) }                                          \
        else { MCPC_LOSS_BERNOULLI_GRAD4(ev, ov, yv, ON) }                                                                         \
        e.x = ev[0]; e.y = ev[1]; e.z = ev[2]; e.w = ev[3];                                                                        \
    } while (0)
// the mean of a Bernoulli read-out o
__device__ __forceinline__ float bernoulli_mean(float o) { return sigmoid_f(o); }

}  // namespace mcpc
