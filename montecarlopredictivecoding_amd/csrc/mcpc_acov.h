// Streaming lagged products of recorded steps (include/mcpc.h: mcpc_acov_accumulate): per element e of a record row (E = B * width) and
// lag k = 0..K, lagged[e][k] = sum over the samples j of the STREAM of g(s_j) * g(s_{j-k}), j - k >= 0, in fp64; beside it sum[e], the
// first K samples (head) and the last K (window).  A centred autocovariance, the integrated autocorrelation time and the effective
// sample size follow from these without a second pass (autocovariance.py).
//
// The first reducer whose result depends on the ORDER of the records, and on records of earlier calls: the caller passes the number of
// samples consumed so far (n_seen) and keeps the state; the kernel reads window[k][e] = g of the sample k + 1 places back when it starts
// and rewrites it when it ends, so g is computed once per sample and a lag crosses a chunk boundary like any other.
//
// The contract of mcpc_moments.h: one thread OWNS kVec consecutive elements and walks the samples in ascending order, K + 1 fp64
// accumulators per element in registers; no atomics, no split of the record axis.  A product of two fp32 values is exact in fp64, so
// acc + a * b rounds once whether or not it is contracted, and the result is bitwise the sequential host loop, whatever the launch
// shape and however the stream is chunked.
//
// The register window.  The last kCap values live in registers, w[0] the newest; an array indexed by a runtime value would go to
// scratch, so every index is a compile-time constant: the kernel is instantiated per capacity kCap in {8, 16, 32, 64} (K rounded up;
// the lags above K are computed on whatever the slots above K hold and never stored), and the steady state consumes BLOCKS of
// kAcovInFlight samples: sample u of a block meets the block's own samples u - 1 .. 0 and then w[0 ..], all by constant index, and the
// window moves by a whole block at once (kCap - kAcovInFlight register moves per block and element instead of kCap per sample).  The
// window is held in fp64 up to kCap = 32 (no conversion per product) and in fp32 at kCap = 64 (64 + 130 registers instead of 258; the
// compiler converts a slot once per block, not per product, and parks what does not fit 256 VGPRs in AGPRs: DESIGN.md section 4 has the
// registers, occupancy and scratch = 0 of every instantiation).  kVec per capacity: 4 / 2 / 1 / 1, bounded by 3 kCap + 2 .. 4 kCap + 2
// registers per element.
//
// Absent terms.  A lag k has no term for the stream's samples j < k.  Those first K samples are walked one at a time by a step whose
// lags are predicated on the number of samples seen (a uniform branch per lag): a zero-filled window would put Inf * 0 = NaN there.
//
// Loads: a lane reads 4 * kVec consecutive bytes of a row, a wave a contiguous piece; the next block's kAcovInFlight rows are
// requested before the current block is consumed.  lagged is [E][K + 1]: a thread reads and writes its own K + 1 doubles once per call
// (strided across lanes; long chunks amortise it).  window and head are [K][E]: coalesced.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mcpc.h"
#include "mcpc_moments.h"

namespace mcpc {

constexpr int kAcovInFlight = 8;        // samples per block: their loads are in flight together, and the window moves by as many
constexpr int64_t kAcovMaxThreads = 1LL << 31;   // threads per launch (a grid holds fewer than 2^32)

static_assert(MCPC_ACOV_MAX_LAG == 64, "the largest capacity instantiated is 64");

template <> struct MomVec<2> { using type = float2; };

struct AcovParams {
    const float* rec;       // the FIRST record taken (the host has applied `first`)
    int64_t n_vec;          // E / kVec
    int64_t v0;             // the launch's first thread stands at v0 (a row of 2^31 vectors or more takes several launches)
    int64_t E;              // B * width
    int64_t row_step;       // floats between two records taken (stride * E)
    int64_t n_seen;         // samples of the stream before this call
    int32_t n, K;
    double* lagged;         // [E][K + 1]
    double* sum;            // [E]
    float* window;          // [K][E]
    float* head;            // [K][E]
};

template <int kCap> struct AcovWin { using type = std::conditional_t<(kCap > 32), float, double>; };

// one sample; kWarm: only the lags k <= have hold a term (have: samples of the stream before this one, uniform over the grid)
template <int kCap, bool kWarm, typename W>
__host__ __device__ __forceinline__ void acov_step(double (&acc)[kCap + 1], W (&w)[kCap], double& s, float g, int32_t have) {
    const double gd = (double)g;
    s = s + gd;
    acc[0] = acc[0] + gd * gd;
#pragma unroll
    for (int k = 1; k <= kCap; ++k)
        if (!kWarm || k <= have) acc[k] = acc[k] + gd * (double)w[k - 1];
#pragma unroll
    for (int k = kCap - 1; k > 0; --k) w[k] = w[k - 1];
    w[0] = (W)g;
}

// U samples, g[0] the oldest; every lag has its term (the stream holds at least K samples before them)
template <int kCap, int U, typename W>
__host__ __device__ __forceinline__ void acov_block(double (&acc)[kCap + 1], W (&w)[kCap], double& s, const float (&g)[U]) {
    double gd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) gd[u] = (double)g[u];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        s = s + gd[u];
        acc[0] = acc[0] + gd[u] * gd[u];
#pragma unroll
        for (int k = 1; k <= kCap; ++k) {
            const double partner = k <= u ? gd[u - k] : (double)w[k - u - 1];
            acc[k] = acc[k] + gd[u] * partner;
        }
    }
#pragma unroll
    for (int i = kCap - 1; i >= U; --i) w[i] = w[i - U];
#pragma unroll
    for (int i = 0; i < U && i < kCap; ++i) w[i] = (W)g[U - 1 - i];
}

template <int kXf>
__host__ __device__ __forceinline__ float acov_g(float v) {
    if constexpr (kXf == 0) return v;
    else return mom_transform<kXf>(v);
}

// everything a thread does for the kVec elements from v * kVec on (host-callable, so that a CPU build can walk the same code)
template <int kCap, int kVec, int kXf>
__host__ __device__ __forceinline__ void acov_elements(const AcovParams& P, int64_t v) {
    using V = typename MomVec<kVec>::type;
    using W = typename AcovWin<kCap>::type;
    constexpr int U = kAcovInFlight;
    const int32_t K = P.K, n = P.n;
    const bool fresh = P.n_seen == 0;
    const int32_t have0 = (int32_t)(P.n_seen < (int64_t)K ? P.n_seen : (int64_t)K);              // valid window slots at the start
    const int64_t total = P.n_seen + n;
    const int32_t have1 = (int32_t)(total < (int64_t)K ? total : (int64_t)K);                    // ... and at the end
    const int64_t i0 = v * kVec;
    double acc[kVec][kCap + 1], s[kVec];
    W w[kVec][kCap];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        s[j] = fresh ? 0.0 : P.sum[i0 + j];
#pragma unroll
        for (int k = 0; k <= kCap; ++k) acc[j][k] = (!fresh && k <= K) ? P.lagged[(i0 + j) * (K + 1) + k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kCap; ++k) {
        V r{};
        if (k < have0) r = *reinterpret_cast<const V*>(P.window + (int64_t)k * P.E + i0);
        const float* f = reinterpret_cast<const float*>(&r);
#pragma unroll
        for (int j = 0; j < kVec; ++j) w[j][k] = (W)f[j];
    }

    const float* p = P.rec + i0;
    int32_t i = 0;
    // the stream's first K samples: lags without a term yet are skipped, and the sample goes to head
    for (int64_t t = P.n_seen; i < n && t < (int64_t)K; ++i, ++t) {
        V r = *reinterpret_cast<const V*>(p);
        p += P.row_step;
        float* f = reinterpret_cast<float*>(&r);
#pragma unroll
        for (int j = 0; j < kVec; ++j) f[j] = acov_g<kXf>(f[j]);
        *reinterpret_cast<V*>(P.head + t * P.E + i0) = r;
#pragma unroll
        for (int j = 0; j < kVec; ++j) acov_step<kCap, true>(acc[j], w[j], s[j], f[j], (int32_t)t);
    }
    // blocks of U samples; the next block's rows are requested before this one is consumed
    if (i + U <= n) {
        V cur[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = *reinterpret_cast<const V*>(p + (int64_t)u * P.row_step);
        for (; i + U <= n; i += U) {
            p += (int64_t)U * P.row_step;
            V nxt[U];
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = cur[u];
            if (i + 2 * U <= n) {
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = *reinterpret_cast<const V*>(p + (int64_t)u * P.row_step);
            }
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                float g[U];
#pragma unroll
                for (int u = 0; u < U; ++u) g[u] = acov_g<kXf>(reinterpret_cast<const float*>(&cur[u])[j]);
                acov_block<kCap, U>(acc[j], w[j], s[j], g);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }
    for (; i < n; ++i) {
        const V r = *reinterpret_cast<const V*>(p);
        p += P.row_step;
        const float* f = reinterpret_cast<const float*>(&r);
#pragma unroll
        for (int j = 0; j < kVec; ++j) acov_step<kCap, false>(acc[j], w[j], s[j], acov_g<kXf>(f[j]), 0);
    }

#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        P.sum[i0 + j] = s[j];
#pragma unroll
        for (int k = 0; k <= kCap; ++k)
            if (k <= K) P.lagged[(i0 + j) * (K + 1) + k] = acc[j][k];
    }
#pragma unroll
    for (int k = 0; k < kCap; ++k) {
        if (k < have1) {
            V r;
            float* f = reinterpret_cast<float*>(&r);
#pragma unroll
            for (int j = 0; j < kVec; ++j) f[j] = (float)w[j][k];
            *reinterpret_cast<V*>(P.window + (int64_t)k * P.E + i0) = r;
        }
    }
}

// One thread per vector and no loop over them: around a grid-stride loop the compiler hoists the ~3 kCap uniform predicates (k <= K,
// k < slots valid) out of it and runs out of SGPRs.
template <int kCap, int kVec, int kXf>
__global__ __launch_bounds__(256, (kCap <= 16 ? 2 : 1)) void mcpc_acov_kernel(const AcovParams P) {
    const int64_t v = P.v0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < P.n_vec) acov_elements<kCap, kVec, kXf>(P, v);
}

template <int kCap, int kVec>
inline void acov_launch(int transform, AcovParams P, hipStream_t stream) {
    P.n_vec = P.E / kVec;
    // few elements: waves of their own (blocks of 64) reach more CUs; the sums do not depend on the launch shape
    const int block = P.n_vec <= 64 * 1024 ? 64 : 256;
    for (P.v0 = 0; P.v0 < P.n_vec; P.v0 += kAcovMaxThreads) {
        const int64_t count = P.n_vec - P.v0 < kAcovMaxThreads ? P.n_vec - P.v0 : kAcovMaxThreads;
        const dim3 grid((unsigned)((count + block - 1) / block));
        if (transform == MCPC_MOM_SIGMOID) hipLaunchKernelGGL((mcpc_acov_kernel<kCap, kVec, 1>), grid, dim3(block), 0, stream, P);
        else hipLaunchKernelGGL((mcpc_acov_kernel<kCap, kVec, 0>), grid, dim3(block), 0, stream, P);
    }
}

// kVec elements per thread as the registers of the capacity allow (4 / 2 / 1 / 1) where the row and the pointers allow it, else 1
inline void acov_dispatch(int transform, const AcovParams& P, hipStream_t stream) {
    const uintptr_t align = (uintptr_t)P.rec | (uintptr_t)P.window | (uintptr_t)P.head;
    if (P.K <= 8) {
        if (P.E % 4 == 0 && align % 16 == 0) acov_launch<8, 4>(transform, P, stream);
        else acov_launch<8, 1>(transform, P, stream);
    } else if (P.K <= 16) {
        if (P.E % 2 == 0 && align % 8 == 0) acov_launch<16, 2>(transform, P, stream);
        else acov_launch<16, 1>(transform, P, stream);
    } else if (P.K <= 32) {
        acov_launch<32, 1>(transform, P, stream);
    } else {
        acov_launch<64, 1>(transform, P, stream);
    }
}

}  // namespace mcpc
