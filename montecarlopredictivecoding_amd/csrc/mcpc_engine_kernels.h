// The small kernels the engine's entry points launch (mcpc_api.hip, the ONE unit that includes this header: the kernels are not
// templates): weight packing, target images, padding and un-padding, mu_1, gradient export, the normals.
#pragma once
#include "mcpc_types.h"
#include "mcpc_step_math.h"
#include "mcpc_gemm_f16.h"

namespace mcpc {

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
