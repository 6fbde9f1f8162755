// The fill of a launch's LDS images, shared by the in-place kernel (mcpc_steps_ws2.h) and the unified-wave kernel (mcpc_steps_u.h): both run
// 512 threads per workgroup (kWs2Threads == kUThreads) over one 16-chain unit.
#pragma once
#include "mcpc_kernels.h"       // rowexp_track

namespace mcpc {

static_assert(kWs2Threads == kUThreads, "one fill for both kernel forms");

template <int ACT>
__device__ __forceinline__ void ws2_fill_fx(const KLayer& Ly, float* lds, int chain0, int tid, bool keep_x,
                                            float* lds_rowexp = nullptr, int row_id = 0) {
    const int qpr = Ly.npad / 4;                            // quads per row
    for (int idx = tid; idx < 16 * qpr; idx += kWs2Threads) {
        const int r = idx / qpr, u0 = 4 * (idx - r * qpr);
        const f32x4 x = ld4s(Ly.x + (size_t)(chain0 + r) * Ly.npad + u0);
        const f32x4 fx = act4<ACT>(x);
        st4(lds + Ly.lds_a + r * Ly.ld + u0, fx);
        if (keep_x) st4(lds + Ly.lds_x + r * Ly.ld + u0, x);
        // generation 0 of the row's exponent word (mcpc_kernels.h: rowexp_track; the words were zeroed with the plan)
        if (lds_rowexp != nullptr && r < 16) rowexp_track(lds_rowexp, row_id, r, absmax4(0.f, fx), 0u);
    }
}

// KParams::xl: what the epilogues of a launch read over and over and nobody else writes -- biases, the mu_1 rows and the bit-packed
// target rows of the workgroup's chains -- copied to LDS once (the state rows X_l: ws2_fill_fx)
__device__ __forceinline__ void ws2_fill_constants(const KParams& P, float* lds, int chain0, int tid) {
    for (int l = 1; l < P.L; ++l) {
        const KLayer& Ly = P.layer[l];
        for (int i = tid; i < Ly.npad / 4; i += kWs2Threads) st4(lds + Ly.lds_bias + 4 * i, ld4(Ly.bias + 4 * i));
    }
    {
        const KLayer& Ly = P.layer[0];
        const int qpr = Ly.npad / 4;
        for (int idx = tid; idx < 16 * qpr; idx += kWs2Threads) {
            const int r = idx / qpr, u0 = 4 * (idx - r * qpr);
            st4(lds + Ly.lds_bias + r * Ly.ld + u0, ld4(P.mu1 + (size_t)(chain0 + r) * Ly.npad + u0));
        }
    }
    if (P.has_head) {
        const KHead& H = P.head;
        for (int i = tid; i < H.npad / 4; i += kWs2Threads) st4(lds + H.lds_bias + 4 * i, ld4(H.bias + 4 * i));
        if (H.lds_yw >= 0) {
            uint32_t* const yw = reinterpret_cast<uint32_t*>(lds + H.lds_yw);
            for (int idx = tid; idx < 16 * H.ywords; idx += kWs2Threads) {
                const int r = idx / H.ywords, w = idx - r * H.ywords;
                yw[idx] = H.ybits[(size_t)(chain0 + r) * H.ywords + w];
            }
        }
    }
}

}  // namespace mcpc
