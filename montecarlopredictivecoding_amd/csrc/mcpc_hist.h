// Streaming histograms of recorded steps (include/mcpc.h: mcpc_hist_accumulate): integer counts of g(r) per unit over the records taken,
// per chain or pooled over the chains, in n_bins caller-given bins plus the columns under / over / nan.
//
// A bin is decided by COMPARISON alone.  A value and every edge are mapped to an order-preserving u32 key (the bits of a non-negative
// float with the top bit set, the complement of a negative one; -0.0 is taken as +0.0 first), so that the order of the keys is the order
// of the floats with denormals compared as they are, whatever the float mode of the build.  NaN is told by its bits before that.
//
// A record row is E = B * width floats.  A workgroup of 256 threads owns a TILE of TE = TV * kVec consecutive elements of the row and a
// SEGMENT of the records taken; its counters are u32 in LDS (a segment holds fewer than 2^31 records), bin-major with the element minor,
//     cnt[column][slot(e)],   slot(e) = (e % kVec) * TV + e / kVec,
// so that the lanes of a wave, which hold consecutive 16-B (kVec = 4) or 4-B (kVec = 1) pieces of the row, add into consecutive banks
// whatever bins their values fall into.  TV lanes span the tile and 256 / TV groups of them take every (256 / TV)-th record of the
// segment; groups that meet in a counter do so through LDS atomic adds (integer: exact, any order).  TV is the largest power of two
// for which the counters fit kHistLdsWords and that the row can fill: many bins give a narrow tile and more record groups.
// The edge keys come by value in the launch arguments and are copied to LDS once; a value is classified by a branch-free binary search
// over them (log2 steps, each one LDS read and one compare).
//
// The counters reach global memory once, at the end of the workgroup:
//   exclusive (pool = 0 and one segment):  counts[e][c] = (accumulate ? counts[e][c] : 0) + cnt, plain 8-B stores, coalesced;
//   shared    (pool = 1, or several segments): 64-bit integer atomic adds of the non-zero counters; the host has zeroed counts on the
//             same stream when accumulate = 0.  Pooled, tiles width / gcd(TE, width) apart hold the same units in the same slots: a
//             workgroup counts a run of such tiles into the same counters, and at the end adds up the slots that are the same unit.
// Integer adds commute, so the result depends neither on the decomposition nor on how the caller chunks the records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "../../include/mcpc.h"
#include "mcpc_moments.h"

namespace mcpc {

constexpr int kHistThreads = 256;
constexpr int kHistTable = 256;             // LDS words of the search table (MCPC_HIST_MAX_BINS)
constexpr int kHistLdsWords = 16384;        // 64 KiB of LDS per workgroup: the table and the counters
constexpr int kHistInFlight = 4;            // records whose loads are in flight per thread
constexpr int kHistTargetBlocks = 1024;     // segments are sized for about this many workgroups (256 CUs x 4)
constexpr int kHistMinSegment = 8;          // records per record group and segment, at least: below that the flush dominates
constexpr int64_t kHistMaxGrid = 1 << 22;   // workgroups per launch (a grid holds fewer than 2^32 threads); more tiles: grid-stride

static_assert(MCPC_HIST_MAX_BINS == kHistTable, "the search table holds MCPC_HIST_MAX_BINS keys");

struct HistParams {
    uint32_t key[kHistTable];   // key[i] = hist_key(edges[i]) for i < n_bins, 0xffffffff beyond (above every non-NaN key)
    uint32_t key_hi;            // hist_key(edges[n_bins])
    int32_t n_bins, top;        // top: the largest power of two <= max(n_bins - 1, 1), the first step of the search
    int32_t TV;                 // lanes across a tile (a power of two, 1..256)
    int32_t n, seg;             // records taken; records per segment (gridDim.y segments)
    int32_t width, pool, exclusive, accumulate;
    int64_t E;                  // B * width
    int64_t row_step;           // floats between two records taken (stride * E)
    int64_t tiles;              // tiles of TV * kVec elements in a row
    int64_t period, splits;     // a workgroup counts the tiles first, first + period * splits, ... before it flushes (pool = 0: one tile)
};

__host__ __device__ __forceinline__ uint32_t hist_key_bits(uint32_t b) {
    if (b == 0x80000000u) b = 0u;                                   // -0.0 == 0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

inline uint32_t hist_key(float v) {
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return hist_key_bits(b);
}

// The search table of n_bins + 1 validated edges, shared with mcpc_hist2d.h: key[i] = hist_key(edges[i]) for i < n_bins and 0xffffffff
// up to `cap` (above every non-NaN key), *key_hi = hist_key(edges[n_bins]); returns the first step of the search, the largest power of
// two <= max(n_bins - 1, 1).
inline int32_t hist_key_table(const float* edges, int32_t n_bins, uint32_t* key, int32_t cap, uint32_t* key_hi) {
    for (int32_t i = 0; i < cap; ++i) key[i] = i < n_bins ? hist_key(edges[i]) : 0xffffffffu;
    *key_hi = hist_key(edges[n_bins]);
    int32_t top = 1;
    while (2 * top <= n_bins - 1) top *= 2;
    return top;
}

// One step of the branch-free binary search over the table: what `lo` advances by.  Callers interleave the steps of several values so
// that their table reads are in flight together.
__host__ __device__ __forceinline__ int32_t hist_search_step(const uint32_t* table, int32_t lo, int32_t step, uint32_t kv) {
    return (table[lo + step] <= kv) ? step : 0;
}

// The column of a value with bits `b` and key `kv` whose search ended at `lo`: the bin, or under / over / nan.
__host__ __device__ __forceinline__ int32_t hist_column(int32_t lo, uint32_t b, uint32_t kv, uint32_t key_lo, uint32_t key_hi,
                                                        int32_t n_bins) {
    int32_t col = lo;
    col = kv < key_lo ? n_bins : col;
    col = kv > key_hi ? n_bins + 1 : col;
    col = (b & 0x7fffffffu) > 0x7f800000u ? n_bins + 2 : col;
    return col;
}

// The host's plan: depends on E, width, pool, n and n_bins alone (and the result on none of it).
struct HistPlan {
    int32_t TV, seg, segments;
    int64_t tiles, period, splits;
    size_t lds_bytes;
};

inline int64_t hist_gcd(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

inline HistPlan hist_plan(int64_t E, int32_t width, int pool, int32_t n, int32_t n_bins, int kVec) {
    HistPlan p{};
    const int64_t ncol = n_bins + 3;
    const int64_t n_vec = (E + kVec - 1) / kVec;
    int32_t TV = kHistThreads;
    while (TV > 1 && (ncol * TV * kVec > kHistLdsWords - kHistTable || TV / 2 >= n_vec)) TV /= 2;
    p.TV = TV;
    const int64_t TE = (int64_t)TV * kVec;
    p.tiles = (E + TE - 1) / TE;
    // pooled: tiles `period` apart hold the same units in the same slots, and a workgroup counts a run of them before it flushes once
    p.period = pool ? width / hist_gcd(TE, width) : p.tiles;
    if (p.period > p.tiles) p.period = p.tiles;
    const int64_t runs = (p.tiles + p.period - 1) / p.period;                          // tiles of one class
    const int64_t fill = (kHistTargetBlocks + p.period - 1) / p.period;
    p.splits = runs < fill ? runs : fill;
    const int64_t jobs = p.period * p.splits;
    const int32_t groups = kHistThreads / TV;
    const int64_t want = (kHistTargetBlocks + jobs - 1) / jobs;                        // segments asked for
    const int64_t most = ((int64_t)n + (int64_t)groups * kHistMinSegment - 1) / ((int64_t)groups * kHistMinSegment);
    int64_t segments = want < most ? want : most;
    if (segments < 1) segments = 1;
    p.seg = (int32_t)(((int64_t)n + segments - 1) / segments);
    p.segments = (int32_t)(((int64_t)n + p.seg - 1) / p.seg);
    p.lds_bytes = (size_t)(kHistTable + ncol * TE) * sizeof(uint32_t);
    return p;
}

template <int kVec, int kXf>
__global__ __launch_bounds__(kHistThreads) void mcpc_hist_kernel(const float* __restrict__ rec, const HistParams P,
                                                                 unsigned long long* __restrict__ counts) {
    using V = typename MomVec<kVec>::type;
    extern __shared__ uint32_t hist_lds[];
    uint32_t* const table = hist_lds;
    uint32_t* const cnt = hist_lds + kHistTable;
    const int tid = threadIdx.x;
    const int32_t TV = P.TV, TE = TV * kVec, ncol = P.n_bins + 3;
    for (int i = tid; i < kHistTable; i += kHistThreads) table[i] = P.key[i];
    const int32_t lane = tid & (TV - 1), group = tid / TV, groups = kHistThreads / TV;
    const int64_t k0 = (int64_t)blockIdx.y * P.seg;
    const int64_t k1 = ((int64_t)P.n - k0) < (int64_t)P.seg ? (int64_t)P.n : k0 + P.seg;
    const uint32_t key_lo = P.key[0], key_hi = P.key_hi;

    // N values at once: their searches are independent, so that the LDS reads of a step are in flight together
    auto count = [&](const float* f, auto n_tag) {
        constexpr int N = decltype(n_tag)::value;
        uint32_t b[N], kv[N];
        int32_t lo[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            b[i] = __float_as_uint(mom_transform<kXf>(f[i]));
            kv[i] = hist_key_bits(b[i]);
            lo[i] = 0;
        }
        for (int32_t step = P.top; step > 0; step >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) lo[i] += hist_search_step(table, lo[i], step, kv[i]);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int32_t col = hist_column(lo[i], b[i], kv[i], key_lo, key_hi, P.n_bins);
            atomicAdd(&cnt[col * TE + (i % kVec) * TV + lane], 1u);
        }
    };

    // a job: the tiles first, first + period * splits, ... (pool = 0: one tile); (one job per workgroup unless the row is huge)
    for (int64_t job = blockIdx.x; job < P.period * P.splits; job += gridDim.x) {
        const int64_t first = job;                                                   // (every later one is congruent to it mod period)
        if (first >= P.tiles) continue;                                              // (the whole workgroup)
        for (int i = tid; i < ncol * TE; i += kHistThreads) cnt[i] = 0u;
        __syncthreads();
        for (int64_t tile = first; tile < P.tiles; tile += P.period * P.splits) {
            const int64_t base = tile * TE;                                          // the tile's first element
            const int32_t valid = (int32_t)((P.E - base) < (int64_t)TE ? (P.E - base) : (int64_t)TE);
            if (lane * kVec >= valid) continue;                                      // (kVec = 4: E % 4 == 0, a piece is whole or absent)
            const float* p = rec + (k0 + group) * P.row_step + base + (int64_t)lane * kVec;
            const int64_t hop = (int64_t)groups * P.row_step;
            int64_t k = k0 + group;
            for (; k + (kHistInFlight - 1) * groups < k1; k += kHistInFlight * groups) {
                V r[kHistInFlight];
#pragma unroll
                for (int u = 0; u < kHistInFlight; ++u) r[u] = *reinterpret_cast<const V*>(p + (int64_t)u * hop);
                p += (int64_t)kHistInFlight * hop;
                count(reinterpret_cast<const float*>(r), std::integral_constant<int, kHistInFlight * kVec>{});
            }
            for (; k < k1; k += groups) {
                const V r = *reinterpret_cast<const V*>(p);
                p += hop;
                count(reinterpret_cast<const float*>(&r), std::integral_constant<int, kVec>{});
            }
        }
        __syncthreads();

        // the flush: `nd` destinations x ncol columns; pooled, destination d sums the tile's elements d, d + width, ... (one unit).
        // The first tile of a job is its fullest.
        const int64_t base = first * TE;
        const int32_t valid = (int32_t)((P.E - base) < (int64_t)TE ? (P.E - base) : (int64_t)TE);
        const int32_t nd = (P.pool && P.width < valid) ? P.width : valid;
        const int32_t hop_e = P.pool ? P.width : TE;
        for (int32_t i = tid; i < nd * ncol; i += kHistThreads) {
            const int32_t d = i / ncol, c = i - d * ncol;
            unsigned long long s = 0;
            for (int32_t e = d; e < valid; e += hop_e) s += cnt[c * TE + (e % kVec) * TV + e / kVec];
            const int64_t dest = P.pool ? (base + d) % P.width : base + d;
            unsigned long long* o = counts + dest * ncol + c;
            if (P.exclusive) *o = P.accumulate ? *o + s : s;
            else if (s) atomicAdd(o, s);
        }
        __syncthreads();
    }
}

template <int kVec>
inline void hist_launch(int transform, const float* rec, const HistParams& P, const HistPlan& plan, int64_t* counts, hipStream_t stream) {
    const int64_t jobs = plan.period * plan.splits;
    const int64_t gx = jobs * plan.segments <= kHistMaxGrid ? jobs : kHistMaxGrid / plan.segments;
    const dim3 grid((unsigned)gx, (unsigned)plan.segments), block(kHistThreads);
    if (transform == MCPC_MOM_SIGMOID)
        hipLaunchKernelGGL((mcpc_hist_kernel<kVec, 1>), grid, block, plan.lds_bytes, stream, rec, P, (unsigned long long*)counts);
    else
        hipLaunchKernelGGL((mcpc_hist_kernel<kVec, 0>), grid, block, plan.lds_bytes, stream, rec, P, (unsigned long long*)counts);
}

}  // namespace mcpc
