// Streaming posterior of a linear probe on recorded steps (include/mcpc.h: mcpc_probe_accumulate): the first reducer that applies a
// function the caller supplies.  For chain c, taken record j and class i < C the sample's logit, link value, vote and entropy are formed
// and reduced on the device: psum[c][i] = sum_j p_i, psumsq[c][i] = sum_j p_i^2 (fp64), votes[c][argmax_i v_i] += 1 (int64; column C
// counts the samples with a NaN logit, which cast no vote), entsum[c] = sum_j H_j (fp64, softmax only).
//
// The arithmetic, defined once:
//   logit    z = (double)bias[i]; for k = 0..width-1 ascending z = z + (double)W[i][k] * (double)r_j[c][k]; v_i = (float)z.  A product of
//            two fp32 values is exact in fp64, so each step rounds once whether or not it is contracted: v_i is bitwise the sequential
//            fp64 loop on the host (the argument of mcpc_acov.h).
//   link     identity p_i = v_i; sigmoid p_i = sigmoid_f(v_i) (mom_transform<1>, the library's own); softmax m = max_i v_i,
//            e_i = expf(v_i - m), S = sum_i e_i in fp32 by a butterfly over the Cpad class lanes (Cpad = C rounded up to a power of two,
//            the lanes above C hold 0: the order depends on C alone, and every lane gets the same bits because an fp32 addition
//            commutes), p_i = e_i / S.  expf and logf are the HIP math library's (1 ulp), the division is IEEE.
//   entropy  H_j = logf(S) - sum_i p_i (v_i - m) in fp32, the sum by the same butterfly.
//   sums     psum += (double)p_i, psumsq += (double)p_i * (double)p_i (exact product, one rounding), entsum += (double)H_j, in ascending j.
//   votes    the largest v_i, the lowest index on a tie (np.argmax); a sample with a NaN among its logits counts in column C instead.
//
// The contract of mcpc_moments.h / mcpc_acov.h: every (chain, class) accumulator has ONE owner, the lane (chain, class), which walks the
// samples in ascending order; no atomics, no split of the record axis, no float sum ordered by scheduling.  The result depends neither
// on the launch shape nor on how the caller chunks the records.
//
// Decomposition.  A wave (one workgroup of 64) serves G = 64 / Cpad chains; lane = (chain of the group, class lane).  The samples are
// consumed in BLOCKS of kProbeInFlight = 8 (a shorter last block is predicated): the 8 logit chains of a block are independent and give
// the fp64 FMA pipe its ILP, only the additions into the accumulators are ordered.  A chain's record row is read ONCE per sample: the
// columns are walked in pieces of Cpad, class lane i loads column k0 + i of its chain (a wave reads G contiguous pieces) and the Cpad
// values reach the chain's lanes by __shfl (ds_bpermute; nothing for Cpad = 1); the next piece's 8 loads -- the next block's first piece
// after the last one -- are issued before the current piece is consumed (indices past the end are clamped, not branched around).
// W is staged k-major ([k][Cpad] fp32, lanes of a chain read consecutive words: no bank conflict; the chains of a wave read the same
// words: broadcast) through LDS in k-tiles of kProbeKTile = 64 columns, at most 16 KiB: a width up to 64 stages W once per call, a
// wider one restages each tile once per block of 8 samples (one uncoalesced pass over C x 64 words from L2 per 64 x 8 FMAs of every
// lane), so any width runs.  There is no form with W in registers: it would save one ds_read_b32 per 8 FMAs and 8 shuffles.  Max, sum
// and argmax go across the Cpad lanes by xor-butterflies.
// Accumulators are read and written once per call.  Few chains (128 chains x 16 lanes = 32 waves) leave the kernel latency-bound on
// the record loop; that is accepted as it is for moments -- parallelism over the records would reorder the sums.
//
// The probe as a derived record (include/mcpc.h: mcpc_probe_records) is the SAME kernel with kRecords set: the logit loop, the link and
// the butterflies are the code above, and the link value p_i goes to out[j][c][i] (fp32, the layout of a record) instead of into the
// sums, so that out holds bitwise what the accumulating form adds.  Nothing is ordered there, so the blocks of kProbeInFlight samples
// are dealt out over gridDim.y as well (block b, b + gridDim.y, ... per workgroup; about kProbeRecordWaves waves in all), and few
// chains no longer leave the launch latency-bound.  The accumulating form is gridDim.y = 1 of the same loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_moments.h"

namespace mcpc {

constexpr int kProbeInFlight = 8;       // samples per block: their loads are in flight together, their logit chains are independent
constexpr int kProbeKTile = 64;         // columns of W staged through LDS at a time
constexpr int kProbeRecordWaves = 4096; // mcpc_probe_records: waves a launch is sized for (256 CUs x 16)

static_assert(MCPC_PROBE_MAX_CLASSES == 64, "a chain's classes are the lanes of at most one wave");

struct ProbeParams {
    const float* rec;       // the FIRST record taken (the host has applied `first`)
    const float* W;         // [C][width]
    const float* bias;      // [C] or null
    int64_t row_step;       // floats between two records taken (stride * E)
    int32_t B, width, n, C;
    int32_t accumulate;
    double* psum;           // [B][C]
    double* psumsq;         // [B][C] or null
    int64_t* votes;         // [B][C + 1]
    double* entsum;         // [B] (softmax)
    float* out;             // kRecords: [n][B][C], the link values themselves
};

template <int kCpad>
__device__ __forceinline__ float probe_sum(float v) {
#pragma unroll
    for (int d = 1; d < kCpad; d *= 2) v = v + __shfl_xor(v, d);
    return v;
}

// kLink: MCPC_PROBE_IDENTITY / _SIGMOID / _SOFTMAX; kRecords: write the link values to P.out instead of reducing them
template <int kCpad, int kLink, bool kRecords>
__global__ __launch_bounds__(64) void mcpc_probe_kernel(const ProbeParams P) {
    constexpr int U = kProbeInFlight, KT = kProbeKTile;
    __shared__ float wt[KT * kCpad];
    const int lane = threadIdx.x;
    const int i = lane & (kCpad - 1);                       // class lane
    const int base = lane & ~(kCpad - 1);                   // the chain's first lane
    const int64_t c = (int64_t)blockIdx.x * (64 / kCpad) + lane / kCpad;
    const int32_t width = P.width, n = P.n, C = P.C;
    const bool chain = c < P.B;
    const bool own = chain && i < C;                        // this lane owns (c, i)
    const bool resident = width <= KT;                      // W is staged once
    const int32_t n_piece = (width + kCpad - 1) / kCpad;
    const int32_t n_block = (n + U - 1) / U;
    const int32_t b_first = kRecords ? (int32_t)blockIdx.y : 0, b_step = kRecords ? (int32_t)gridDim.y : 1;

    auto stage = [&](int32_t k0) {                          // wt[kk][ii] = W[ii][k0 + kk], 0 outside
        for (int idx = lane; idx < KT * kCpad; idx += 64) {
            const int kk = idx / kCpad, ii = idx & (kCpad - 1);
            wt[idx] = (ii < C && k0 + kk < width) ? P.W[(int64_t)ii * width + k0 + kk] : 0.0f;
        }
    };
    // piece `pc` of the rows of block `b`: column pc * kCpad + i of samples b * U + u.  Where there is no such chain, column or sample
    // the index is clamped to the last one there is: the value is loaded and never used, and the 8 loads carry no branch, so that the
    // compiler can count them (s_waitcnt vmcnt(8) before a piece is consumed, the next piece's loads still in flight)
    const float* row = P.rec + (chain ? c : 0) * (int64_t)width;
    auto load = [&](int32_t b, int32_t pc, float (&dst)[U]) {
        const int32_t k = pc * kCpad + i < width ? pc * kCpad + i : width - 1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = (int64_t)b * U + u < n ? (int64_t)b * U + u : (int64_t)n - 1;
            dst[u] = row[j * P.row_step + k];
        }
    };

    double s = 0.0, q = 0.0, ent = 0.0;
    int64_t vote = 0, n_nan = 0;
    const bool sq = !kRecords && P.psumsq != nullptr;
    if (!kRecords && own && P.accumulate) {
        s = P.psum[c * C + i];
        if (sq) q = P.psumsq[c * C + i];
        vote = P.votes[c * (C + 1) + i];
        if (i == 0) {
            n_nan = P.votes[c * (C + 1) + C];
            if (kLink == MCPC_PROBE_SOFTMAX) ent = P.entsum[c];
        }
    }
    const double b0 = (own && P.bias) ? (double)P.bias[i] : 0.0;

    if (resident) {
        stage(0);
        __syncthreads();
    }
    float cur[U], nxt[U];
    load(b_first, 0, cur);                                  // n >= 1: the host launches nothing for n = 0
    for (int32_t b = b_first; b < n_block; b += b_step) {
        double z[U];
#pragma unroll
        for (int u = 0; u < U; ++u) z[u] = b0;
        for (int32_t pc = 0; pc < n_piece; ++pc) {
            const int32_t k0 = pc * kCpad;
            if (!resident && k0 % KT == 0) {
                __syncthreads();                            // the previous tile has been read
                stage(k0);
                __syncthreads();
            }
            const bool more = pc + 1 < n_piece;
            load(more ? b : b + b_step, more ? pc + 1 : 0, nxt);    // (behind the last block: its last sample again, not used)
            const float* wk = wt + (k0 % KT) * kCpad + i;
#pragma unroll
            for (int jj = 0; jj < kCpad; ++jj) {
                if (k0 + jj < width) {
                    const double w = (double)wk[jj * kCpad];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float r = kCpad == 1 ? cur[u] : __shfl(cur[u], base + jj);
                        z[u] = z[u] + w * (double)r;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
        const int32_t cnt = n - b * U < U ? n - b * U : U;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < cnt) {
                const float v = (float)z[u];
                // argmax over the chain's classes, the lowest index on a tie; lanes above C never win
                float best = i < C ? v : -INFINITY;
                int arg = i;
                int bad = (i < C && v != v) ? 1 : 0;
#pragma unroll
                for (int d = 1; d < kCpad; d *= 2) {
                    const float ob = __shfl_xor(best, d);
                    const int oa = __shfl_xor(arg, d);
                    bad |= __shfl_xor(bad, d);
                    if (ob > best || (ob == best && oa < arg)) {
                        best = ob;
                        arg = oa;
                    }
                }
                if constexpr (!kRecords) {
                    if (bad) n_nan += 1;
                    else if (arg == i) vote += 1;
                }
                float p;
                if constexpr (kLink == MCPC_PROBE_IDENTITY) {
                    p = v;
                } else if constexpr (kLink == MCPC_PROBE_SIGMOID) {
                    p = mom_transform<1>(v);
                } else {
                    // m: the largest logit that is no NaN (`best`); a NaN logit reaches S through its own e and from there every p
                    const float d = v - best;
                    const float e = i < C ? expf(d) : 0.0f;
                    const float S = probe_sum<kCpad>(e);
                    p = e / S;
                    if constexpr (!kRecords) {
                        const float h = logf(S) - probe_sum<kCpad>(i < C ? p * d : 0.0f);
                        ent = ent + (double)h;
                    }
                }
                if constexpr (kRecords) {
                    if (own) P.out[((int64_t)(b * U + u) * P.B + c) * C + i] = p;
                } else {
                    const double pd = (double)p;
                    s = s + pd;
                    if (sq) q = q + pd * pd;
                }
            }
        }
    }

    if (!kRecords && own) {
        P.psum[c * C + i] = s;
        if (sq) P.psumsq[c * C + i] = q;
        P.votes[c * (C + 1) + i] = vote;
        if (i == 0) {
            P.votes[c * (C + 1) + C] = n_nan;
            if (kLink == MCPC_PROBE_SOFTMAX) P.entsum[c] = ent;
        }
    }
}

// The record form's gridDim.y: blocks of kProbeInFlight samples per chain group, a plain host function of the shape.
inline int32_t probe_record_rows(int64_t chain_groups, int32_t n) {
    const int64_t n_block = ((int64_t)n + kProbeInFlight - 1) / kProbeInFlight;
    int64_t gy = (kProbeRecordWaves + chain_groups - 1) / chain_groups;
    if (gy > n_block) gy = n_block;
    if (gy > 65535) gy = 65535;
    return (int32_t)(gy < 1 ? 1 : gy);
}

template <int kCpad, bool kRecords>
inline void probe_launch(int link, const ProbeParams& P, hipStream_t stream) {
    const int64_t gx = ((int64_t)P.B + 64 / kCpad - 1) / (64 / kCpad);
    const dim3 grid((unsigned)gx, kRecords ? (unsigned)probe_record_rows(gx, P.n) : 1u), block(64);
    if (link == MCPC_PROBE_SOFTMAX)
        hipLaunchKernelGGL((mcpc_probe_kernel<kCpad, MCPC_PROBE_SOFTMAX, kRecords>), grid, block, 0, stream, P);
    else if (link == MCPC_PROBE_SIGMOID)
        hipLaunchKernelGGL((mcpc_probe_kernel<kCpad, MCPC_PROBE_SIGMOID, kRecords>), grid, block, 0, stream, P);
    else
        hipLaunchKernelGGL((mcpc_probe_kernel<kCpad, MCPC_PROBE_IDENTITY, kRecords>), grid, block, 0, stream, P);
}

// Cpad: C rounded up to a power of two
template <bool kRecords = false>
inline void probe_dispatch(int link, const ProbeParams& P, hipStream_t stream) {
    if (P.C <= 1) probe_launch<1, kRecords>(link, P, stream);
    else if (P.C <= 2) probe_launch<2, kRecords>(link, P, stream);
    else if (P.C <= 4) probe_launch<4, kRecords>(link, P, stream);
    else if (P.C <= 8) probe_launch<8, kRecords>(link, P, stream);
    else if (P.C <= 16) probe_launch<16, kRecords>(link, P, stream);
    else if (P.C <= 32) probe_launch<32, kRecords>(link, P, stream);
    else probe_launch<64, kRecords>(link, P, stream);
}

}  // namespace mcpc
