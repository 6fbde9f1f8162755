// Streaming second moments BETWEEN units of recorded steps (include/mcpc.h: mcpc_cov_accumulate): fp64 sums of outer products v v^T
// over the records taken, per chain or pooled over the chains.
//
// The column space is the concatenation of up to kCovMaxBlocks record buffers ([records][B][w_j] fp32, as mcpc_run writes rec_x[l] /
// rec_out), each padded to a multiple of 16 columns OF ITS OWN so that no 16-column tile straddles two buffers.  The contraction runs on
// v_mfma_f64_16x16x4_f64: an fp32 value and the product of two of them are exact in fp64, so the only roundings are the fp64 additions.
// For a tile of 16 columns and 4 rows the A fragment and the B fragment are the same register pair -- lane (m = lane & 15, q = lane >> 4)
// holds v[row q][16 I + m] -- so a wave loads ONE fragment per tile and issues one MFMA per tile pair I <= J.
//
// A job is (chain group, block of at most 4 x 4 tile pairs) and belongs to one wave (a workgroup of 64 lanes): no LDS, no barrier, no
// atomics, no wait on another wave.
//   pool = 0: the group is one chain; the four rows of an MFMA are four records.  The wave adds its tiles into outer[chain] itself and
//             mirrors them into the lower triangle.
//   pool = 1: the group is a run of `gs` consecutive chains (a multiple of 4; the last group may be ragged); the four rows of an MFMA are
//             four chains of one record.  The wave writes its tiles (I <= J only) into a partial matrix [Dpad][Dpad] of its group in the
//             caller's workspace, and mcpc_cov_finish_kernel adds the partials in ascending group order, one thread per element of
//             outer, reading (min, max) for both triangles.
// Lanes beyond a block's width, rows beyond the last record and chains beyond the group's end contribute exact zeros and READ NOTHING
// (the column behind a row is the next chain's data, and behind the last row it is not the buffer's).
// kCovInFlight row groups' fragments are loaded before the first is consumed.
//
// What is bitwise: two runs of the same call (the group size depends on B and the widths alone; every sum has one fixed order), and
// outer[i][j] == outer[j][i] (one value is stored twice; inside a diagonal tile only i <= j is taken).  What is NOT: the same records
// chunked differently over calls -- an MFMA adds four products in an order of its own, and every call rounds once more into outer -- and
// the diagonal against mcpc_moments_accumulate's sumsq.  Both hold within (R + G + 2) * 2^-52 * sum |v_i v_j| (R rows contracted, G pooled
// groups).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_moments.h"

namespace mcpc {

constexpr int kCovMaxBlocks = 7;        // MCPC_MAX_LATENT + 1: every latent layer and the read-out
constexpr int kCovTB = 4;               // tiles per side of a job's block of tile pairs
constexpr int kCovInFlight = 4;         // row groups whose fragments are in flight per wave
constexpr int kCovTargetJobs = 1024;    // pooled: groups are sized for about this many waves (256 CUs x 4 SIMDs)

typedef double cov_d4 __attribute__((ext_vector_type(4)));

struct CovParams {
    const float* rec[kCovMaxBlocks];    // the record buffers, `first` NOT applied
    int32_t width[kCovMaxBlocks];
    int32_t xf[kCovMaxBlocks];          // MCPC_MOM_*
    int32_t tile0[kCovMaxBlocks + 1];   // first 16-column tile of a block; [n_blocks] = NT (unused blocks: NT)
    int32_t col0[kCovMaxBlocks + 1];    // first column of a block in outer; [n_blocks] = D
    int32_t n_blocks, NT, NB, npairs, D, Dpad;
    int32_t B, first, stride, n, gs, accumulate;
    double* out;                        // pool = 0: outer [B][D][D]; pool = 1: the workspace [groups][Dpad][Dpad]
};

// The host's plan: depends on B and the widths alone.
struct CovPlan {
    int32_t NT, NB, npairs, D, Dpad, gs, groups;
};

inline CovPlan cov_plan(int32_t B, const int32_t* widths, int32_t n_blocks, int pool) {
    CovPlan p{};
    int64_t D = 0, NT = 0;
    for (int b = 0; b < n_blocks; ++b) { D += widths[b]; NT += (widths[b] + 15) / 16; }
    p.D = (int32_t)D; p.NT = (int32_t)NT; p.Dpad = (int32_t)(16 * NT);
    p.NB = (p.NT + kCovTB - 1) / kCovTB;
    p.npairs = p.NB * (p.NB + 1) / 2;
    if (pool) {
        const int32_t want = (kCovTargetJobs + p.npairs - 1) / p.npairs;             // groups asked for
        const int32_t per = (B + want - 1) / want;                                   // chains per group, then up to a multiple of 4
        p.gs = (per + 3) / 4 * 4;
        p.groups = (B + p.gs - 1) / p.gs;
    } else {
        p.gs = 1;
        p.groups = B;
    }
    return p;
}

// what a lane needs to know about one 16-column tile
struct CovTile {
    const float* p;     // the lane's column in the first chain of the first record; nullptr: the lane (or the whole tile) reads nothing
    int32_t w;          // floats between two chains
    int32_t cbase;      // the tile's first column in outer
    int32_t cw;         // columns of the tile's block from the tile's first on (>= 16: a full tile)
    int32_t xf;
};

__device__ __forceinline__ CovTile cov_tile(const CovParams& P, int I, int m) {
    CovTile t{nullptr, 0, 0, 0, 0};
    if (I >= P.NT) return t;
#pragma unroll
    for (int b = 0; b < kCovMaxBlocks; ++b) {
        if (b < P.n_blocks && I >= P.tile0[b] && I < P.tile0[b + 1]) {
            const int c0 = 16 * (I - P.tile0[b]);
            t.w = P.width[b];
            t.cw = P.width[b] - c0;
            t.cbase = P.col0[b] + c0;
            t.xf = P.xf[b];
            t.p = m < t.cw ? P.rec[b] + c0 + m : nullptr;
        }
    }
    return t;
}

template <bool kPool, bool kSig>
__global__ __launch_bounds__(64) void mcpc_cov_kernel(const CovParams P) {
    const int lane = threadIdx.x, m = lane & 15, q = lane >> 4;
    // job -> (group, block pair bi <= bj); everything here is wave-uniform
    const int32_t g = (int32_t)(blockIdx.x / (uint32_t)P.npairs);
    int32_t rem = (int32_t)(blockIdx.x % (uint32_t)P.npairs), bi = 0;
    while (rem >= P.NB - bi) { rem -= P.NB - bi; ++bi; }
    const int32_t bj = bi + rem;
    const bool diag = bi == bj;
    const int32_t I0 = bi * kCovTB, J0 = bj * kCovTB;
    const int32_t g0 = g * P.gs, g1 = kPool ? min(g0 + P.gs, P.B) : g0 + 1;
    const int32_t nq = kPool ? (g1 - g0 + 3) / 4 : 1;                                // quads of chains per record

    CovTile tI[kCovTB], tJ[kCovTB];
#pragma unroll
    for (int t = 0; t < kCovTB; ++t) {
        tI[t] = cov_tile(P, I0 + t, m);
        tJ[t] = cov_tile(P, J0 + t, m);
    }
    cov_d4 acc[kCovTB][kCovTB];
#pragma unroll
    for (int a = 0; a < kCovTB; ++a)
#pragma unroll
        for (int b = 0; b < kCovTB; ++b) acc[a][b] = cov_d4{0.0, 0.0, 0.0, 0.0};

    // row groups: (k, quad) in ascending order.  pool: record k, chains g0 + 4 quad + q; else records 4 k + q of chain g0.
    const int64_t nk = kPool ? (int64_t)P.n : ((int64_t)P.n + 3) / 4;
    int64_t k = 0;
    int32_t quad = 0;
    while (k < nk) {
        float fI[kCovInFlight][kCovTB], fJ[kCovInFlight][kCovTB];
        bool ok[kCovInFlight];
#pragma unroll
        for (int u = 0; u < kCovInFlight; ++u) {
            const int64_t r = kPool ? k : 4 * k + q;
            const int32_t chain = kPool ? g0 + 4 * quad + q : g0;
            const bool row_ok = ok[u] = r < (int64_t)P.n && chain < g1;               // false for every lane once k >= nk
            const int64_t row = row_ok ? ((int64_t)P.first + r * (int64_t)P.stride) * (int64_t)P.B + chain : 0;
#pragma unroll
            for (int t = 0; t < kCovTB; ++t) {
                fI[u][t] = (row_ok && tI[t].p) ? tI[t].p[row * (int64_t)tI[t].w] : 0.0f;
                fJ[u][t] = (!diag && row_ok && tJ[t].p) ? tJ[t].p[row * (int64_t)tJ[t].w] : 0.0f;
            }
            if (++quad == nq) { quad = 0; ++k; }
        }
#pragma unroll
        for (int u = 0; u < kCovInFlight; ++u) {
            double dI[kCovTB], dJ[kCovTB];
#pragma unroll
            for (int t = 0; t < kCovTB; ++t) {
                // a lane that read nothing holds 0.0f and must stay an exact zero under the transform
                float a = fI[u][t], b = fJ[u][t];
                if (kSig) {
                    if (tI[t].xf == MCPC_MOM_SIGMOID) a = (ok[u] && tI[t].p) ? mom_transform<MCPC_MOM_SIGMOID>(a) : 0.0f;
                    if (tJ[t].xf == MCPC_MOM_SIGMOID) b = (ok[u] && tJ[t].p) ? mom_transform<MCPC_MOM_SIGMOID>(b) : 0.0f;
                }
                dI[t] = (double)a;
                dJ[t] = diag ? dI[t] : (double)b;
            }
#pragma unroll
            for (int a = 0; a < kCovTB; ++a)
#pragma unroll
                for (int b = 0; b < kCovTB; ++b)
                    if (I0 + a < P.NT && J0 + b < P.NT && I0 + a <= J0 + b)
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(dI[a], dJ[b], acc[a][b], 0, 0, 0);
        }
    }

    // C/D layout of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int a = 0; a < kCovTB; ++a)
#pragma unroll
        for (int b = 0; b < kCovTB; ++b) {
            const int32_t I = I0 + a, J = J0 + b;
            if (I >= P.NT || J >= P.NT || I > J) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int ri = q + 4 * reg;
                const double v = acc[a][b][reg];
                if (kPool) {
                    double* part = P.out + (int64_t)g * P.Dpad * P.Dpad;
                    part[(int64_t)(16 * I + ri) * P.Dpad + 16 * J + m] = v;
                } else {
                    if (ri >= tI[a].cw || m >= tJ[b].cw) continue;
                    const int64_t i = tI[a].cbase + ri, j = tJ[b].cbase + m;
                    if (i > j) continue;                                             // inside a diagonal tile: the upper triangle only
                    double* o = P.out + (int64_t)g * P.D * P.D;
                    const int64_t ij = i * P.D + j, ji = j * P.D + i;
                    if (P.accumulate) {
                        o[ij] = o[ij] + v;
                        if (i != j) o[ji] = o[ji] + v;
                    } else {
                        o[ij] = v;
                        o[ji] = v;
                    }
                }
            }
        }
}

// pooled: outer[i][j] (+)= part[0][a][b] + part[1][a][b] + ... in ascending group order, (a, b) the padded places of (min, max)
__global__ __launch_bounds__(256) void mcpc_cov_finish_kernel(const CovParams P, const double* __restrict__ part, int32_t groups,
                                                              double* __restrict__ outer) {
    const int64_t total = (int64_t)P.D * P.D;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const int32_t i = (int32_t)(e / P.D), j = (int32_t)(e % P.D);
        const int32_t lo = i < j ? i : j, hi = i < j ? j : i;
        int32_t plo = 0, phi = 0;
#pragma unroll
        for (int b = 0; b < kCovMaxBlocks; ++b) {
            if (b < P.n_blocks && lo >= P.col0[b]) plo = 16 * P.tile0[b] + (lo - P.col0[b]);
            if (b < P.n_blocks && hi >= P.col0[b]) phi = 16 * P.tile0[b] + (hi - P.col0[b]);
        }
        const int64_t at = (int64_t)plo * P.Dpad + phi, gstep = (int64_t)P.Dpad * P.Dpad;
        double s = part[at];
        for (int32_t gq = 1; gq < groups; ++gq) s = s + part[at + gq * gstep];
        outer[e] = P.accumulate ? outer[e] + s : s;
    }
}

}  // namespace mcpc
