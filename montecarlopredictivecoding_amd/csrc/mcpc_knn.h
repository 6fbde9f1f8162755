// The k smallest squared distances from every query row into a reference set (include/mcpc.h: mcpc_knn_accumulate): the hot path of the
// Perez-Cruz nearest-neighbour KL estimator the reference runs on two scipy KD-trees (utils/training_evaluation.py, KLdivergence).  Brute
// force: for query i and reference j, D(i, j) = sum_c (q[i][c] - ref[j][c])^2, and best[i][0..k) keeps the k smallest D(i, .), ascending.
//
// The arithmetic, defined once:
//   distance   a = 0; for c = 0..d-1 ascending: t = q[i][c] - ref[j][c] (one fp32 rounding); a = fmaf(t, t, a) (one rounding).  Every
//              term is non-negative, so D is within (d + 3) * 2^-24 relative of the exact distance of the same fp32 rows (the
//              derivation is in tests/knn_cases.py).
//   selection  fminf / fmaxf alone: v goes into the last slot by b[k-1] = fminf(b[k-1], v) and one pass of compare-exchanges
//              (fminf, fmaxf) towards slot 0 restores the order.  fminf(b, NaN) = b: a NaN distance (a non-finite reference row) is never
//              selected, and a query row that holds a NaN keeps +inf.  Slots start at +inf, or at the caller's values with a NaN read as +inf.
// min and max are exact, commutative and associative, so the k smallest of a multiset do not depend on the order its members arrive in:
// best is bitwise independent of the tile size, of the number of reference splits, of the order of the reference rows and of how the
// caller chunks ref over calls (accumulate = 1 folds the old best in as k more candidates).  No row is skipped as "self".
//
// Why not the GEMM form, and so no MFMA.  |q|^2 + |r|^2 - 2 q.r would put the pair loop on the matrix unit, but it cancels exactly where
// the estimator looks: for a near neighbour the three terms are of the size of |q|^2 and their sum is of the size of the spacing, so the
// result carries an absolute error of |q|^2 * 2^-24 into a quantity whose logarithm is summed.  The fp32 MFMA is an exact fmaf chain of
// PRODUCTS a * b; a sum of squared DIFFERENCES has no such form.  The differences are taken first, in fp32, on the VALU.
//
// Decomposition.  256-lane workgroups; grid x runs over blocks of 256 * Q query rows, grid y over splits of the reference tiles.  A lane
// owns Q query rows in VGPRs, two rows to a float2 (Q * RS <= 64 floats, RS = the d of the instantiation rounded up to 4), so that one
// v_pk_add_f32 and one v_pk_fma_f32 serve a coordinate of two rows; a row's K slots are VGPRs too.  A tile of the reference (256 rows,
// 128 from RS = 12 on) is staged in LDS with row stride RS and read with 16-byte loads at an address the whole wave shares: identical
// addresses broadcast without bank conflicts, and one read feeds 4 * Q subtract-FMA pairs.  Two LDS buffers: the next tile's global loads
// are issued before the current tile is consumed and stored after it, one barrier per tile.  Rows of the last tile past the end of ref
// are staged as NaN: their distances are NaN and never win -- the path a non-finite reference row takes.  A d between two instantiations
// runs on the next one with zero coordinates on both sides: t = 0 and fmaf(0, 0, a) = a, bit for bit.
// Each (query block, split) leaves its K best in the workspace ([split][nq][K]); mcpc_knn_merge_kernel, one lane per query row, folds
// the splits and, when accumulating, the old best.  Both kernels bound every index by nq / nr; all offsets are 64-bit.
//
// VALU instructions per pair at d = 5, k = 2 (figure 5): 5 packed (10 for two pairs) + 3 selection = 8 lane-instructions, against
// 256 CUs * 64 lanes * 2.4 GHz = 39.3e12 lane-instructions/s: at most 4.9e12 pairs/s.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpc.h"

namespace mcpc {

static_assert(MCPC_KNN_MAX_DIM == 32 && MCPC_KNN_MAX_K == 4, "the instantiations below cover d <= 32 and k <= 4");

constexpr int kKnnThreads = 256;
constexpr int kKnnTargetGroups = 4096;      // workgroups a launch aims at: 16 per CU, so that the last round of groups is a small share

typedef float knn_f2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int knn_rs(int dc) { return (dc + 3) / 4 * 4; }                       // LDS row stride, floats
__host__ __device__ constexpr int knn_q(int dc) { return 64 / knn_rs(dc) >= 8 ? 8 : (64 / knn_rs(dc)) & ~1; }   // rows per lane (even)
__host__ __device__ constexpr int knn_tile(int dc) { return knn_rs(dc) <= 8 ? 256 : 128; }          // reference rows per tile

// the d an instantiation computes: every d up to 8, then steps
inline int knn_dc(int d) { return d <= 8 ? d : d <= 12 ? 12 : d <= 16 ? 16 : d <= 24 ? 24 : 32; }
inline int knn_kt(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : 4; }                                    // slots an instantiation keeps

struct KnnGeometry {
    int dc, kt, q, tile;
    int64_t n_qblocks, n_tiles, n_splits, tiles_per_split;
};

// Depends on the shape alone (not on the device): the workspace size is a function of (nq, nr, d, k).
inline KnnGeometry knn_geometry(int64_t nq, int64_t nr, int d, int k) {
    KnnGeometry g{};
    g.dc = knn_dc(d); g.kt = knn_kt(k); g.q = knn_q(g.dc); g.tile = knn_tile(g.dc);
    const int64_t per_block = (int64_t)kKnnThreads * g.q;
    g.n_qblocks = (nq + per_block - 1) / per_block;
    g.n_tiles = (nr + g.tile - 1) / g.tile;
    int64_t want = g.n_qblocks > 0 ? (kKnnTargetGroups + g.n_qblocks - 1) / g.n_qblocks : 1;
    if (want > g.n_tiles) want = g.n_tiles;
    if (want < 1) want = 1;
    g.tiles_per_split = g.n_tiles > 0 ? (g.n_tiles + want - 1) / want : 0;
    g.n_splits = g.n_tiles > 0 ? (g.n_tiles + g.tiles_per_split - 1) / g.tiles_per_split : 0;
    return g;
}

struct KnnParams {
    const float* q;         // [nq][d]
    const float* ref;       // [nr][d]
    int64_t nq, nr;
    int32_t d, k;
    int64_t tiles_per_split, n_tiles, n_splits;
    float* part;            // workspace [n_splits][nq][KT]
    float* best;            // [nq][k]
    int32_t accumulate;
};

// b[0..K) ascending and free of NaN; v any value
template <int K>
__device__ __forceinline__ void knn_insert(float (&b)[K], float v) {
    b[K - 1] = fminf(b[K - 1], v);
#pragma unroll
    for (int s = K - 2; s >= 0; --s) {
        const float lo = fminf(b[s], b[s + 1]), hi = fmaxf(b[s], b[s + 1]);
        b[s] = lo;
        b[s + 1] = hi;
    }
}

// The same on the pair loop, as single instructions.  fminf / fmaxf of a loop-carried value make the compiler canonicalise it first
// (v_max_f32 x, x, x: one more instruction per slot and row, 1 in 9 at d = 5, k = 2), because it cannot see that the slots only ever
// hold +inf or results of v_min / v_max and v is the result of an FMA: never a signalling NaN.  With a quiet NaN v_min_f32 and
// v_max_f32 return the other operand, as fminf and fmaxf do.
__device__ __forceinline__ float knn_vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float knn_vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
template <int K>
__device__ __forceinline__ void knn_insert_fast(float (&b)[K], float v) {
    b[K - 1] = knn_vmin(b[K - 1], v);
#pragma unroll
    for (int s = K - 2; s >= 0; --s) {
        const float lo = knn_vmin(b[s], b[s + 1]), hi = knn_vmax(b[s], b[s + 1]);
        b[s] = lo;
        b[s + 1] = hi;
    }
}

template <int DC, int K>
__global__ __launch_bounds__(kKnnThreads) void mcpc_knn_kernel(const KnnParams P) {
    constexpr int RS = knn_rs(DC), Q = knn_q(DC), TILE = knn_tile(DC), NT = kKnnThreads;
    constexpr int PER = (TILE * DC + NT - 1) / NT;          // tile elements a lane moves
    __shared__ __attribute__((aligned(16))) float tile[2][TILE * RS];
    const int tid = threadIdx.x;
    const int32_t d = P.d;
    const int64_t row0 = (int64_t)blockIdx.x * (NT * Q) + tid;              // this lane's rows: row0 + i * NT
    const int64_t t_begin = (int64_t)blockIdx.y * P.tiles_per_split;
    const int64_t t_end = t_begin + P.tiles_per_split < P.n_tiles ? t_begin + P.tiles_per_split : P.n_tiles;

    knn_f2 qv[Q / 2][DC];
    float best[Q][K];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int64_t row = row0 + (int64_t)i * NT;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const float v = (row < P.nq && c < d) ? P.q[row * d + c] : 0.0f;
            if (i & 1) qv[i / 2][c].y = v;
            else qv[i / 2][c].x = v;
        }
#pragma unroll
        for (int s = 0; s < K; ++s) best[i][s] = INFINITY;
    }

    // element e of a tile: row e / DC, coordinate e % DC; a row past nr is NaN, a coordinate past d is 0
    float stage[PER];
    auto load = [&](int64_t t) {
        const int64_t base = t * TILE;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + u * NT;
            const int r = e / DC, c = e - r * DC;
            float v = 0.0f;
            if (e < TILE * DC) {
                if (base + r >= P.nr) v = __builtin_nanf("");
                else if (c < d) v = P.ref[(base + r) * d + c];
            }
            stage[u] = v;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = tid + u * NT;
            const int r = e / DC, c = e - r * DC;
            if (e < TILE * DC) tile[buf][r * RS + c] = stage[u];
        }
    };

    if (t_begin < t_end) {
        load(t_begin);
        store(0);
    }
    __syncthreads();
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int buf = (int)((t - t_begin) & 1);
        const bool more = t + 1 < t_end;
        if (more) load(t + 1);
        const float* rows = tile[buf];
#pragma unroll 2
        for (int j = 0; j < TILE; ++j) {
            float r[RS];
#pragma unroll
            for (int c4 = 0; c4 < RS / 4; ++c4) {
                const float4 v = *reinterpret_cast<const float4*>(rows + j * RS + c4 * 4);
                r[c4 * 4 + 0] = v.x; r[c4 * 4 + 1] = v.y; r[c4 * 4 + 2] = v.z; r[c4 * 4 + 3] = v.w;
            }
#pragma unroll
            for (int p = 0; p < Q / 2; ++p) {
                knn_f2 a = {0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < DC; ++c) {
                    const knn_f2 rc = {r[c], r[c]};
                    const knn_f2 t2 = qv[p][c] - rc;
                    a = __builtin_elementwise_fma(t2, t2, a);
                }
                knn_insert_fast<K>(best[2 * p], a.x);
                knn_insert_fast<K>(best[2 * p + 1], a.y);
            }
        }
        if (more) store(buf ^ 1);
        __syncthreads();
    }

    float* part = P.part + (int64_t)blockIdx.y * P.nq * K;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const int64_t row = row0 + (int64_t)i * NT;
        if (row < P.nq) {
#pragma unroll
            for (int s = 0; s < K; ++s) part[row * K + s] = best[i][s];
        }
    }
}

// One lane per query row: the k best of the splits' partial results and, when accumulating, of the old best (a NaN there reads as +inf).
__global__ __launch_bounds__(kKnnThreads) void mcpc_knn_merge_kernel(const KnnParams P, int kt) {
    const int64_t row = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
    if (row >= P.nq) return;
    float b[MCPC_KNN_MAX_K];
#pragma unroll
    for (int s = 0; s < MCPC_KNN_MAX_K; ++s) b[s] = INFINITY;
    if (P.accumulate)
        for (int s = 0; s < P.k; ++s) knn_insert<MCPC_KNN_MAX_K>(b, P.best[row * P.k + s]);
    for (int64_t sp = 0; sp < P.n_splits; ++sp)
        for (int s = 0; s < kt; ++s) knn_insert<MCPC_KNN_MAX_K>(b, P.part[(sp * P.nq + row) * kt + s]);
#pragma unroll
    for (int s = 0; s < MCPC_KNN_MAX_K; ++s)
        if (s < P.k) P.best[row * P.k + s] = b[s];
}

template <int DC>
inline void knn_launch(const KnnGeometry& g, const KnnParams& P, hipStream_t stream) {
    const dim3 grid((unsigned)g.n_qblocks, (unsigned)g.n_splits), block(kKnnThreads);
    if (g.kt == 1) hipLaunchKernelGGL((mcpc_knn_kernel<DC, 1>), grid, block, 0, stream, P);
    else if (g.kt == 2) hipLaunchKernelGGL((mcpc_knn_kernel<DC, 2>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((mcpc_knn_kernel<DC, 4>), grid, block, 0, stream, P);
}

inline void knn_dispatch(const KnnGeometry& g, const KnnParams& P, hipStream_t stream) {
    if (g.n_splits > 0) {
        switch (g.dc) {
            case 1: knn_launch<1>(g, P, stream); break;
            case 2: knn_launch<2>(g, P, stream); break;
            case 3: knn_launch<3>(g, P, stream); break;
            case 4: knn_launch<4>(g, P, stream); break;
            case 5: knn_launch<5>(g, P, stream); break;
            case 6: knn_launch<6>(g, P, stream); break;
            case 7: knn_launch<7>(g, P, stream); break;
            case 8: knn_launch<8>(g, P, stream); break;
            case 12: knn_launch<12>(g, P, stream); break;
            case 16: knn_launch<16>(g, P, stream); break;
            case 24: knn_launch<24>(g, P, stream); break;
            default: knn_launch<32>(g, P, stream); break;
        }
    }
    const dim3 grid((unsigned)((P.nq + kKnnThreads - 1) / kKnnThreads)), block(kKnnThreads);
    hipLaunchKernelGGL(mcpc_knn_merge_kernel, grid, block, 0, stream, P, g.kt);
}

}  // namespace mcpc
