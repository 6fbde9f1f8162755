// Streaming first and second moments of recorded steps (include/mcpc.h: mcpc_moments_accumulate).
//
// A record buffer is [records][row_elems] fp32, as mcpc_run writes rec_x[l] / rec_out.  One thread OWNS kVec consecutive elements of
// a row and walks the chosen records in ascending order with fp64 accumulators in registers: no atomics, no split of the record axis,
// no fp32 pre-sums.  The result therefore depends neither on the launch shape nor on how the caller chunks the records, and with the
// identity transform it is bitwise the sequential fp64 loop on the host (the square of an fp32 value is exact in fp64, so
// sumsq + v * v rounds once whether or not the compiler contracts it into an fma).
//
// Bandwidth: 4 B read per element and record, 16 B (32 with sumsq) of accumulator read-modify-write per element and CALL -- long
// chunks amortise the latter.  kVec = 4 reads 16 B per lane (row_elems % 4 == 0 and 16-B aligned pointers: then every row is
// aligned); kVec = 1 is the form for everything else (an odd row_elems puts every second row off alignment).  kInFlight records'
// loads are issued before the first is consumed.  At small row_elems the kernel is latency-bound on the record loop; that is
// accepted -- parallelism over the record axis would reorder the sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mcpc_step_math.h"

namespace mcpc {

constexpr int kMomInFlight = 8;         // records whose loads are in flight per thread
constexpr int kMomMaxBlocks = 2048;     // grid cap (256 CUs x 8 blocks); the rest is grid-stride

template <int kVec> struct MomVec;
template <> struct MomVec<1> { using type = float; };
template <> struct MomVec<4> { using type = float4; };

template <int kXf>
__device__ __forceinline__ float mom_transform(float v) {
    if constexpr (kXf == 1) return bernoulli_mean(v);
    else return v;
}

// rec: the FIRST record taken (the host has applied `first`); row_step: floats between two records taken (stride * row_elems);
// n_vec: row_elems / kVec.
template <int kVec, int kXf, bool kSq>
__global__ __launch_bounds__(256) void mcpc_moments_kernel(const float* __restrict__ rec, int64_t n_vec, int64_t row_step, int32_t n,
                                                           double* __restrict__ sum, double* __restrict__ sumsq, int accumulate) {
    using V = typename MomVec<kVec>::type;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += step) {
        const int64_t i0 = v * kVec;
        double s[kVec], q[kVec];
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            s[j] = accumulate ? sum[i0 + j] : 0.0;
            q[j] = (kSq && accumulate) ? sumsq[i0 + j] : 0.0;
        }
        const float* p = rec + i0;
        int32_t k = 0;
        for (; k + kMomInFlight <= n; k += kMomInFlight) {
            V r[kMomInFlight];
#pragma unroll
            for (int u = 0; u < kMomInFlight; ++u) r[u] = *reinterpret_cast<const V*>(p + (int64_t)u * row_step);
            p += (int64_t)kMomInFlight * row_step;
#pragma unroll
            for (int u = 0; u < kMomInFlight; ++u) {
                const float* f = reinterpret_cast<const float*>(&r[u]);
#pragma unroll
                for (int j = 0; j < kVec; ++j) {
                    const double g = (double)mom_transform<kXf>(f[j]);
                    s[j] = s[j] + g;
                    if (kSq) q[j] = q[j] + g * g;
                }
            }
        }
        for (; k < n; ++k) {
            const V r = *reinterpret_cast<const V*>(p);
            p += row_step;
            const float* f = reinterpret_cast<const float*>(&r);
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                const double g = (double)mom_transform<kXf>(f[j]);
                s[j] = s[j] + g;
                if (kSq) q[j] = q[j] + g * g;
            }
        }
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            sum[i0 + j] = s[j];
            if (kSq) sumsq[i0 + j] = q[j];
        }
    }
}

template <int kVec, int kXf, bool kSq>
inline void mom_launch(const float* rec, int64_t row_elems, int64_t row_step, int32_t n, double* sum, double* sumsq, int accumulate,
                       hipStream_t stream) {
    const int64_t n_vec = row_elems / kVec;
    // few elements: waves of their own (blocks of 64) reach more CUs; the sums do not depend on the launch shape
    const int block = n_vec <= 64 * 1024 ? 64 : 256;
    const int64_t blocks = (n_vec + block - 1) / block;
    const int grid = (int)(blocks < kMomMaxBlocks ? blocks : kMomMaxBlocks);
    hipLaunchKernelGGL((mcpc_moments_kernel<kVec, kXf, kSq>), dim3(grid), dim3(block), 0, stream, rec, n_vec, row_step, n, sum, sumsq,
                       accumulate);
}

template <int kVec>
inline void mom_dispatch(int transform, const float* rec, int64_t row_elems, int64_t row_step, int32_t n, double* sum, double* sumsq,
                         int accumulate, hipStream_t stream) {
    if (transform == 1) {
        if (sumsq) mom_launch<kVec, 1, true>(rec, row_elems, row_step, n, sum, sumsq, accumulate, stream);
        else mom_launch<kVec, 1, false>(rec, row_elems, row_step, n, sum, sumsq, accumulate, stream);
    } else {
        if (sumsq) mom_launch<kVec, 0, true>(rec, row_elems, row_step, n, sum, sumsq, accumulate, stream);
        else mom_launch<kVec, 0, false>(rec, row_elems, row_step, n, sum, sumsq, accumulate, stream);
    }
}

}  // namespace mcpc
