// Streaming joint histograms of recorded steps (include/mcpc.h: mcpc_hist2d_accumulate): integer counts of the pair
// (g_x(rec_x[k][c][px]), g_y(rec_y[k][c][py])) over the records taken, per chain or pooled over the chains, for up to
// MCPC_HIST2D_MAX_PAIRS pairs of columns, in an (nx + 3) x (ny + 3) grid: the bins of each axis, then under / over / nan.
//
// Each axis is classified exactly as mcpc_hist.h classifies a value: hist_key_bits, hist_key_table, hist_search_step and hist_column
// are that header's, so a marginal of the grid is the 1-D histogram of the column, bit for bit.
//
// Decomposition.  A SLOT is one grid: (chain, pair) with pool = 0, a pair with pool = 1; in either case slot s is grid s of `counts`.
// A workgroup of 256 threads owns G consecutive slots, as many as fit the LDS counters (u32; G = 1 for the largest grid of
// MCPC_HIST2D_MAX_CELLS, 8 for the 43 x 43 of a class-plane panel), a SEGMENT of the records taken and, pooled, a range of chains.
// Its threads are GL = G rounded up to a power of two slot lanes times 256 / GL record lanes: thread (sl, rl) counts slot s0 + sl over
// the records k0 + rl, k0 + rl + 256 / GL, ... of the segment, kHist2dInFlight records' loads (both axes) in flight, their
// 2 * kHist2dInFlight searches interleaved.  Consecutive slots are the pairs of one chain (or, with one pair, consecutive chains), so the
// slot lanes of a wave address ONE contiguous chain row per record: a wave's load fetches each 64-B line of that row once and serves
// the group's pairs from it, instead of a line per pair.  The row is not staged through LDS: with the largest grid the counters leave
// no room for it, and a pair reads two words of it.  Lanes that meet in a counter (a repeated pair, the record lanes of a slot) do so
// through LDS atomic adds (integer: exact, any order).  A segment times a chain range holds fewer than 2^31 samples.
//
// The counters reach global memory once per workgroup, slot-major as `counts` is, so the flush is one coalesced pass:
//   exclusive (pool = 0 and one segment):  counts = (accumulate ? counts : 0) + cnt, plain 8-B stores;
//   shared    (pool = 1, or several segments): 64-bit integer atomic adds of the non-zero counters; the host has zeroed counts on the
//             same stream when accumulate = 0.
// Integer adds commute: the result depends neither on the plan, nor on how the caller chunks the records, nor on the order of pairs.
// Edge keys and pairs come by value in the launch arguments (2.2 KiB of the 4 KiB a launch may carry); the keys are copied to LDS once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_hist.h"

namespace mcpc {

constexpr int kHist2dThreads = 256;
constexpr int kHist2dTable = MCPC_HIST2D_MAX_BINS;      // LDS words of one axis' search table
constexpr int kHist2dCounterWords = kHistLdsWords - 2 * kHist2dTable;   // 64 KiB of LDS: two tables and the counters
constexpr int kHist2dInFlight = 4;                      // records whose loads are in flight per thread (two loads each)
constexpr int kHist2dTargetBlocks = 1024;               // chain ranges and segments are sized for about this many workgroups
constexpr int kHist2dMinSegment = 8;                    // records per record lane and segment, at least: below that the flush dominates

static_assert(MCPC_HIST2D_MAX_CELLS <= kHist2dCounterWords, "one grid's counters fit the LDS beside the tables");
static_assert((MCPC_HIST2D_MAX_BINS & (MCPC_HIST2D_MAX_BINS - 1)) == 0, "the search's first step stays inside the table");

struct Hist2dParams {
    uint32_t key_x[kHist2dTable], key_y[kHist2dTable];  // as HistParams::key, per axis
    uint32_t hi_x, hi_y;
    int32_t nx, ny, top_x, top_y;
    int32_t col[MCPC_HIST2D_MAX_PAIRS][2];              // pair -> (column of rec_x, column of rec_y)
    int32_t n_pairs, B, wx, wy;
    int32_t G, GL;                                      // slots per workgroup; slot lanes (a power of two >= G)
    int32_t n, seg;                                     // records taken; records per segment (gridDim.y segments)
    int32_t chains_per;                                 // pooled: chains per workgroup (gridDim.z ranges)
    int32_t pool, exclusive, accumulate;
    int64_t slots, groups;                              // grids in all; groups of G of them
    int64_t step_x, step_y;                             // floats between two records taken
};

// The host's plan: a function of the shape alone (and the result of none of it).
struct Hist2dPlan {
    int32_t G, GL, seg, segments, chains_per, chain_ranges;
    int64_t slots, groups, cells;
    size_t lds_bytes;
};

inline Hist2dPlan hist2d_plan(int32_t B, int32_t /*wx*/, int32_t /*wy*/, int32_t n_pairs, int32_t nx, int32_t ny, int pool, int32_t n) {
    Hist2dPlan p{};
    p.cells = (int64_t)(nx + 3) * (ny + 3);
    p.slots = pool ? (int64_t)n_pairs : (int64_t)B * n_pairs;
    int64_t G = kHist2dCounterWords / p.cells;
    if (G > kHist2dThreads) G = kHist2dThreads;
    if (G > p.slots) G = p.slots;
    p.G = (int32_t)G;
    p.GL = 1;
    while (p.GL < p.G) p.GL *= 2;
    p.groups = (p.slots + G - 1) / G;
    const int32_t RL = kHist2dThreads / p.GL;
    // pooled: the chains are split first (a chain range costs nothing but its flush), then the records
    int64_t ranges = 1;
    if (pool) {
        ranges = (kHist2dTargetBlocks + p.groups - 1) / p.groups;
        if (ranges > B) ranges = B;
    }
    p.chains_per = pool ? (int32_t)((B + ranges - 1) / ranges) : 1;
    p.chain_ranges = pool ? (int32_t)((B + p.chains_per - 1) / p.chains_per) : 1;
    const int64_t jobs = p.groups * p.chain_ranges;
    const int64_t want = (kHist2dTargetBlocks + jobs - 1) / jobs;
    const int64_t most = ((int64_t)n + (int64_t)RL * kHist2dMinSegment - 1) / ((int64_t)RL * kHist2dMinSegment);
    int64_t segments = want < most ? want : most;
    if (segments < 1) segments = 1;
    int64_t seg = ((int64_t)n + segments - 1) / segments;
    while (seg > 1 && seg * p.chains_per > (int64_t)INT32_MAX) seg = (seg + 1) / 2;   // a workgroup's u32 counters do not wrap
    p.seg = (int32_t)seg;
    p.segments = (int32_t)(((int64_t)n + seg - 1) / seg);
    p.lds_bytes = (size_t)(2 * kHist2dTable + G * p.cells) * sizeof(uint32_t);
    return p;
}

// The cell of one sample in a grid of ny + 3 columns: the classification of both axes, for host and device (the device kernel
// interleaves the same steps over several samples).
__host__ __device__ inline int32_t hist2d_cell(const uint32_t* tx, const uint32_t* ty, uint32_t bx, uint32_t by, int32_t nx, int32_t ny,
                                               int32_t top_x, int32_t top_y, uint32_t lo_x, uint32_t hi_x, uint32_t lo_y, uint32_t hi_y) {
    const uint32_t kx = hist_key_bits(bx), ky = hist_key_bits(by);
    int32_t ix = 0, iy = 0;
    for (int32_t step = top_x; step > 0; step >>= 1) ix += hist_search_step(tx, ix, step, kx);
    for (int32_t step = top_y; step > 0; step >>= 1) iy += hist_search_step(ty, iy, step, ky);
    return hist_column(ix, bx, kx, lo_x, hi_x, nx) * (ny + 3) + hist_column(iy, by, ky, lo_y, hi_y, ny);
}

template <int kXfX, int kXfY>
__global__ __launch_bounds__(kHist2dThreads) void mcpc_hist2d_kernel(const float* __restrict__ rec_x, const float* __restrict__ rec_y,
                                                                     const Hist2dParams P, unsigned long long* __restrict__ counts) {
    extern __shared__ uint32_t hist2d_lds[];
    uint32_t* const tx = hist2d_lds;
    uint32_t* const ty = hist2d_lds + kHist2dTable;
    uint32_t* const cnt = hist2d_lds + 2 * kHist2dTable;
    const int tid = threadIdx.x;
    for (int i = tid; i < kHist2dTable; i += kHist2dThreads) {
        tx[i] = P.key_x[i];
        ty[i] = P.key_y[i];
    }
    const int32_t nx = P.nx, ny = P.ny, ncy = ny + 3;
    const int64_t cells = (int64_t)(nx + 3) * ncy;
    const int32_t sl = tid & (P.GL - 1), rl = tid / P.GL, RL = kHist2dThreads / P.GL;
    const int64_t k0 = (int64_t)blockIdx.y * P.seg;
    const int64_t k1 = ((int64_t)P.n - k0) < (int64_t)P.seg ? (int64_t)P.n : k0 + P.seg;
    const uint32_t lo_x = P.key_x[0], lo_y = P.key_y[0], hi_x = P.hi_x, hi_y = P.hi_y;

    // N samples at once: their 2 N searches are independent, so that the LDS reads of a step are in flight together
    auto count = [&](uint32_t* my, const float* fx, const float* fy, auto n_tag) {
        constexpr int N = decltype(n_tag)::value;
        uint32_t bx[N], by[N], kx[N], ky[N];
        int32_t ix[N], iy[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            bx[i] = __float_as_uint(mom_transform<kXfX>(fx[i]));
            by[i] = __float_as_uint(mom_transform<kXfY>(fy[i]));
            kx[i] = hist_key_bits(bx[i]);
            ky[i] = hist_key_bits(by[i]);
            ix[i] = iy[i] = 0;
        }
        for (int32_t step = P.top_x; step > 0; step >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) ix[i] += hist_search_step(tx, ix[i], step, kx[i]);
        }
        for (int32_t step = P.top_y; step > 0; step >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) iy[i] += hist_search_step(ty, iy[i], step, ky[i]);
        }
#pragma unroll
        for (int i = 0; i < N; ++i)
            atomicAdd(&my[hist_column(ix[i], bx[i], kx[i], lo_x, hi_x, nx) * ncy + hist_column(iy[i], by[i], ky[i], lo_y, hi_y, ny)], 1u);
    };

    // a job: G consecutive slots (one job per workgroup unless there are more groups than a grid holds)
    for (int64_t job = blockIdx.x; job < P.groups; job += gridDim.x) {
        const int64_t s0 = job * P.G;
        const int32_t g = (int32_t)((P.slots - s0) < (int64_t)P.G ? (P.slots - s0) : (int64_t)P.G);
        for (int64_t i = tid; i < g * cells; i += kHist2dThreads) cnt[i] = 0u;
        __syncthreads();
        if (sl < g) {
            const int64_t s = s0 + sl;
            const int32_t pair = (int32_t)(P.pool ? s : s % P.n_pairs);
            int64_t c_lo = P.pool ? (int64_t)blockIdx.z * P.chains_per : s / P.n_pairs;
            int64_t c_hi = P.pool ? c_lo + P.chains_per : c_lo + 1;
            if (c_hi > P.B) c_hi = P.B;
            const int32_t px = P.col[pair][0], py = P.col[pair][1];
            uint32_t* const my = cnt + sl * cells;
            const int64_t hop_x = (int64_t)RL * P.step_x, hop_y = (int64_t)RL * P.step_y;
            for (int64_t c = c_lo; c < c_hi; ++c) {
                const float* qx = rec_x + (k0 + rl) * P.step_x + c * P.wx + px;
                const float* qy = rec_y + (k0 + rl) * P.step_y + c * P.wy + py;
                int64_t k = k0 + rl;
                for (; k + (kHist2dInFlight - 1) * RL < k1; k += kHist2dInFlight * RL) {
                    float fx[kHist2dInFlight], fy[kHist2dInFlight];
#pragma unroll
                    for (int u = 0; u < kHist2dInFlight; ++u) {
                        fx[u] = qx[(int64_t)u * hop_x];
                        fy[u] = qy[(int64_t)u * hop_y];
                    }
                    qx += (int64_t)kHist2dInFlight * hop_x;
                    qy += (int64_t)kHist2dInFlight * hop_y;
                    count(my, fx, fy, std::integral_constant<int, kHist2dInFlight>{});
                }
                for (; k < k1; k += RL) {
                    const float fx = *qx, fy = *qy;
                    qx += hop_x;
                    qy += hop_y;
                    count(my, &fx, &fy, std::integral_constant<int, 1>{});
                }
            }
        }
        __syncthreads();
        unsigned long long* const out = counts + s0 * cells;
        for (int64_t i = tid; i < g * cells; i += kHist2dThreads) {
            const unsigned long long v = cnt[i];
            if (P.exclusive) out[i] = P.accumulate ? out[i] + v : v;
            else if (v) atomicAdd(out + i, v);
        }
        __syncthreads();
    }
}

inline void hist2d_launch(int xf_x, int xf_y, const float* rec_x, const float* rec_y, const Hist2dParams& P, const Hist2dPlan& plan,
                          int64_t* counts, hipStream_t stream) {
    const int64_t per = (int64_t)plan.segments * plan.chain_ranges;
    const int64_t gx = plan.groups * per <= kHistMaxGrid ? plan.groups : (kHistMaxGrid / per > 0 ? kHistMaxGrid / per : 1);
    const dim3 grid((unsigned)gx, (unsigned)plan.segments, (unsigned)plan.chain_ranges), block(kHist2dThreads);
    unsigned long long* const out = (unsigned long long*)counts;
    const bool sx = xf_x == MCPC_MOM_SIGMOID, sy = xf_y == MCPC_MOM_SIGMOID;
    if (sx && sy) hipLaunchKernelGGL((mcpc_hist2d_kernel<1, 1>), grid, block, plan.lds_bytes, stream, rec_x, rec_y, P, out);
    else if (sx) hipLaunchKernelGGL((mcpc_hist2d_kernel<1, 0>), grid, block, plan.lds_bytes, stream, rec_x, rec_y, P, out);
    else if (sy) hipLaunchKernelGGL((mcpc_hist2d_kernel<0, 1>), grid, block, plan.lds_bytes, stream, rec_x, rec_y, P, out);
    else hipLaunchKernelGGL((mcpc_hist2d_kernel<0, 0>), grid, block, plan.lds_bytes, stream, rec_x, rec_y, P, out);
}

}  // namespace mcpc
