// Rolling-window variance of recorded steps (include/mcpc.h: mcpc_roll_accumulate): per element e of a record row (E = B * width) the
// variance (ddof 1) of the last W samples of a STREAM, emitted for every `every`-th full window, and per emitted row the sums over the
// elements of sd = sqrt(v), sd^2, v and the count of finite elements.  The first reducer whose result is resolved in TIME: how the
// variability of a chain changes along a call and across the boundary of two calls (rolling.py).
//
// Per element, samples in ascending order, g the transformed fp32 value:
//     s1 = s1 + (double)g;  s2 = s2 + (double)g * (double)g;                       entering sample j
//     if (j >= W) { s1 = s1 - (double)o;  s2 = s2 - (double)o * (double)o; }       o = g of sample j - W
//     if (j >= W - 1 && (j - (W - 1)) % every == 0) { m = s1 / W;  v = (s2 - s1 * m) / (W - 1);  v = v < 0 ? 0 : v; }
// A product of two fp32 values is exact in fp64, so the s1 / s2 lines round once whether or not they are contracted; the v line is
// compiled with contraction off.  v is therefore bitwise the sequential host loop, whatever the launch shape and however the stream is
// chunked.  A window that is not full yet emits nothing: an absent term is absent, not a zero.
//
// The contract of mcpc_moments.h and mcpc_acov.h: one thread OWNS kVec consecutive elements and walks the samples in ascending order,
// s1 and s2 in registers; no atomics, no split of the record axis.  The caller keeps the state: s1, s2 fp64 [E] and hist fp32 [W][E], a
// circular buffer in which sample j lives in row j mod W.  The leaving sample j - W comes from the chunk itself when it lies in it (the
// record is read a second time and g recomputed: the same bits) and from hist otherwise; hist is written for the chunk's last min(n, W)
// samples only, and a thread reads its own slot before it writes it (within one call the samples that read hist are the chunk's first W
// at most, whose slots are distinct, so no slot is read after this call wrote it).
//
// A non-finite sample makes s1 / s2 of ITS element non-finite for the rest of the stream (Inf - Inf = NaN: the sums never recover, even
// after the sample has left the window); v of that element is NaN or Inf from then on.  The pooled row leaves such an element out and
// counts one element fewer: it never poisons a row, and no other element changes a bit.
//
// The pooled sums.  A thread adds its kVec elements in ascending order from 0, the 64 lanes of a wave are added in the association of an
// xor-butterfly by DPP moves and four lane reads (no LDS; every lane ends with the same bits), the waves of a workgroup in ascending order through LDS, and the workgroups' partials go to a
// caller-owned workspace [groups][rows][4] that a finishing kernel adds in ascending group order.  The block is always kRollBlock
// threads, so the association is a function of E and kVec alone and a pooled row is bitwise independent of chunking too.  The wave sums
// of kRollBatch emitted rows are parked in LDS between two barriers: a barrier pair per kRollBatch rows, not per sample.  Lanes past
// the last element walk the last element's records with every store switched off and contribute zeros: the butterfly and the barriers
// need every lane of the workgroup.
//
// Loads: a lane reads 4 * kVec consecutive bytes of a row, a wave a contiguous piece; the entering and the leaving rows of the next
// kRollInFlight samples are requested before the current ones are consumed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcpc.h"
#include "mcpc_moments.h"

namespace mcpc {

constexpr int kRollInFlight = 8;        // samples per block: the loads of their entering and leaving rows are in flight together
constexpr int kRollBlock = 256;         // threads per workgroup, always: the pooled sums' association must not depend on the launch
constexpr int kRollWaves = kRollBlock / 64;
constexpr int kRollBatch = 8;           // emitted rows whose wave sums wait in LDS for one barrier pair
constexpr int64_t kRollMaxGroups = 1LL << 31;

struct RollParams {
    const float* rec;       // the FIRST record taken (the host has applied `first`)
    int64_t n_vec;          // E / kVec
    int64_t E;              // B * width
    int64_t row_step;       // floats between two records taken (stride * E)
    int64_t n_seen;         // samples of the stream before this call
    int64_t emit0;          // the stream index of the first sample at or after n_seen that emits a row
    int64_t rows;           // rows this call emits
    int32_t n, W, every;
    int32_t slot0;          // n_seen mod W
    double* s1;             // [E]
    double* s2;             // [E]
    float* hist;            // [W][E]
    double* out_elem;       // [rows][E] or null
    double* part;           // [groups][rows][4] or null
};

// rows a chunk of n samples emits after n_seen samples of the stream, and the stream index of the first sample that emits one
__host__ __device__ inline int64_t roll_rows(int64_t n_seen, int64_t n, int64_t W, int64_t every, int64_t* emit0) {
    int64_t j = n_seen < W - 1 ? W - 1 : n_seen;
    const int64_t r = (j - (W - 1)) % every;
    if (r) j += every - r;
    if (emit0) *emit0 = j;
    return j < n_seen + n ? (n_seen + n - 1 - j) / every + 1 : 0;
}

template <int kXf>
__host__ __device__ __forceinline__ float roll_g(float v) {
    if constexpr (kXf == 0) return v;
    else return mom_transform<kXf>(v);
}

// the emitted value; not contracted: s1 * m rounds before it is subtracted, as in the host loop
__host__ __device__ __forceinline__ double roll_var(double s1, double s2, double Wd, double W1d) {
#pragma clang fp contract(off)
    const double m = s1 / Wd;
    double v = (s2 - s1 * m) / W1d;
    v = v < 0 ? 0 : v;                                             // NaN stays NaN
    return v;
}

template <int kVec> struct RollState {
    double s1[kVec], s2[kVec];
    int64_t next;           // the stream index of the next sample that emits
    int64_t r;              // rows emitted so far in this call
    int32_t slot;           // the current sample's row of hist
};

// a pool that keeps nothing (out_pool = NULL, and the host walk)
struct RollNoPool {
    template <int kVec> __host__ __device__ __forceinline__ void row(const double (&)[kVec], bool) {}
    __host__ __device__ __forceinline__ void finish() {}
};

// one sample i of the chunk: `in` its record, `out` the leaving one (kSrc 0: none; 1: g as hist holds it; 2: a record of this chunk)
template <int kVec, int kXf, int kSrc, typename Pool>
__host__ __device__ __forceinline__ void roll_sample(const RollParams& P, int64_t i0, bool live, int32_t i,
                                                     const typename MomVec<kVec>::type& in, const typename MomVec<kVec>::type& out,
                                                     RollState<kVec>& st, Pool& pool) {
    using V = typename MomVec<kVec>::type;
    V gv;
    float* g = reinterpret_cast<float*>(&gv);
    const float* fi = reinterpret_cast<const float*>(&in);
    const float* fo = reinterpret_cast<const float*>(&out);
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        g[k] = roll_g<kXf>(fi[k]);
        const double gd = (double)g[k];
        st.s1[k] = st.s1[k] + gd;
        st.s2[k] = st.s2[k] + gd * gd;
        if constexpr (kSrc != 0) {
            const double od = (double)(kSrc == 2 ? roll_g<kXf>(fo[k]) : fo[k]);
            st.s1[k] = st.s1[k] - od;
            st.s2[k] = st.s2[k] - od * od;
        }
    }
    if (live && i >= P.n - P.W) *reinterpret_cast<V*>(P.hist + (int64_t)st.slot * P.E + i0) = gv;      // the chunk's last min(n, W)
    st.slot = st.slot + 1 == P.W ? 0 : st.slot + 1;
    if (P.n_seen + i == st.next) {
        double v[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) v[k] = roll_var(st.s1[k], st.s2[k], (double)P.W, (double)(P.W - 1));
        if (live && P.out_elem) {
#pragma unroll
            for (int k = 0; k < kVec; ++k) P.out_elem[st.r * P.E + i0 + k] = v[k];
        }
        pool.row(v, live);
        st.next += P.every;
        ++st.r;
    }
}

// samples ib .. ie - 1 of the chunk, all with the same source of their leaving sample
template <int kVec, int kXf, int kSrc, typename Pool>
__host__ __device__ __forceinline__ void roll_span(const RollParams& P, int64_t i0, bool live, int32_t ib, int32_t ie, RollState<kVec>& st,
                                                   Pool& pool) {
    using V = typename MomVec<kVec>::type;
    constexpr int U = kRollInFlight;
    const float* rec = P.rec + i0;
    // the leaving record of sample i: hist row (slot of i), which in a block is st.slot of the block's first sample plus u, wrapped
    auto leaving = [&](int32_t i, int32_t ahead) -> V {
        if constexpr (kSrc == 2) return *reinterpret_cast<const V*>(rec + (int64_t)(i - P.W) * P.row_step);
        else if constexpr (kSrc == 1) {
            int32_t s = st.slot + ahead;
            while (s >= P.W) s -= P.W;
            return *reinterpret_cast<const V*>(P.hist + (int64_t)s * P.E + i0);
        } else return V{};
    };
    int32_t i = ib;
    // blocks of U samples; the next block's rows are requested before this one is consumed
    if (i + U <= ie) {
        V cin[U], cout[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cin[u] = *reinterpret_cast<const V*>(rec + (int64_t)(i + u) * P.row_step);
            cout[u] = leaving(i + u, u);
        }
        for (; i + U <= ie; i += U) {
            V nin[U], nout[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { nin[u] = cin[u]; nout[u] = cout[u]; }
            if (i + 2 * U <= ie) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    nin[u] = *reinterpret_cast<const V*>(rec + (int64_t)(i + U + u) * P.row_step);
                    nout[u] = leaving(i + U + u, U + u);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) roll_sample<kVec, kXf, kSrc>(P, i0, live, i + u, cin[u], cout[u], st, pool);
#pragma unroll
            for (int u = 0; u < U; ++u) { cin[u] = nin[u]; cout[u] = nout[u]; }
        }
    }
    for (; i < ie; ++i) {
        const V in = *reinterpret_cast<const V*>(rec + (int64_t)i * P.row_step);
        const V out = leaving(i, 0);
        roll_sample<kVec, kXf, kSrc>(P, i0, live, i, in, out, st, pool);
    }
}

// everything a thread does for the kVec elements from v * kVec on (host-callable, so that a CPU build can walk the same code); a
// thread that is not `live` stores nothing
template <int kVec, int kXf, typename Pool>
__host__ __device__ __forceinline__ void roll_elements(const RollParams& P, int64_t v, bool live, Pool& pool) {
    const int64_t i0 = v * kVec;
    const bool fresh = P.n_seen == 0;
    RollState<kVec> st;
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        st.s1[k] = fresh ? 0.0 : P.s1[i0 + k];
        st.s2[k] = fresh ? 0.0 : P.s2[i0 + k];
    }
    st.next = P.emit0;
    st.r = 0;
    st.slot = P.slot0;
    const int64_t W = P.W, n = P.n;
    // samples of the stream below W have nothing leaving; then hist holds it for the chunk's first W samples, the chunk itself after
    const int32_t a = (int32_t)(P.n_seen >= W ? 0 : (W - P.n_seen < n ? W - P.n_seen : n));
    const int32_t b = (int32_t)(W < n ? W : n);
    roll_span<kVec, kXf, 0>(P, i0, live, 0, a, st, pool);
    if (a < b) roll_span<kVec, kXf, 1>(P, i0, live, a, b, st, pool);
    if (b < P.n) roll_span<kVec, kXf, 2>(P, i0, live, b > a ? b : a, P.n, st, pool);
    if (live) {
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            P.s1[i0 + k] = st.s1[k];
            P.s2[i0 + k] = st.s2[k];
        }
    }
    pool.finish();
}

// a lane's value as another lane of its row of 16 holds it (a DPP move: no LDS, every lane active)
template <int kCtrl>
__device__ __forceinline__ double roll_dpp(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), kCtrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), kCtrl, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double roll_lane(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// The sum over the 64 lanes of a wave, the same bits in every lane, in the association of an xor-butterfly: pairs, quads (quad_perm),
// halves of a row (row_half_mirror: after the quad step every lane of a quad holds the quad's sum, so the mirrored lane holds the other
// quad's), rows (row_mirror), then the four rows' sums out of lanes 0, 16, 32, 48 as (r0 + r1) + (r2 + r3).  An fp addition commutes,
// so both partners of a step get the same bits.
__device__ __forceinline__ double roll_wave_sum(double x) {
    x = x + roll_dpp<0xB1>(x);                                     // quad_perm [1, 0, 3, 2]
    x = x + roll_dpp<0x4E>(x);                                     // quad_perm [2, 3, 0, 1]
    x = x + roll_dpp<0x141>(x);                                    // row_half_mirror
    x = x + roll_dpp<0x140>(x);                                    // row_mirror
    return (roll_lane(x, 0) + roll_lane(x, 16)) + (roll_lane(x, 32) + roll_lane(x, 48));
}

// the pooled sums of a workgroup: wave-first, then the waves in ascending order, a barrier pair per kRollBatch rows
struct RollPool {
    double (*lds)[kRollWaves][4];       // [kRollBatch]
    double* part;                       // this workgroup's [rows][4]
    int64_t done;                       // rows already written to part
    int32_t filled;                     // rows waiting in LDS

    template <int kVec>
    __device__ __forceinline__ void row(const double (&v)[kVec], bool live) {
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                if (live && __builtin_isfinite(v[k])) {
                    const double sd = sqrt(v[k]);
                    a[0] = a[0] + sd;
                    a[1] = a[1] + sd * sd;
                    a[2] = a[2] + v[k];
                    a[3] = a[3] + 1.0;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = roll_wave_sum(a[c]);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) lds[filled][threadIdx.x >> 6][c] = a[c];
        }
        if (++filled == kRollBatch) flush();
    }

    __device__ __forceinline__ void flush() {
        __syncthreads();
        if ((int32_t)threadIdx.x < filled * 4) {
            const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
            double s = lds[r][0][c];
#pragma unroll
            for (int w = 1; w < kRollWaves; ++w) s = s + lds[r][w][c];
            part[(done + r) * 4 + c] = s;
        }
        __syncthreads();
        done += filled;
        filled = 0;
    }

    __device__ __forceinline__ void finish() {
        if (filled) flush();
    }
};

template <int kVec, int kXf, bool kPool>
__global__ __launch_bounds__(kRollBlock) void mcpc_roll_kernel(const RollParams P) {
    __shared__ double lds[kRollBatch][kRollWaves][4];
    int64_t v = (int64_t)blockIdx.x * kRollBlock + threadIdx.x;
    const bool live = v < P.n_vec;
    if (!live) v = P.n_vec - 1;                                    // walks the last vector's records, stores nothing, adds zeros
    if constexpr (kPool) {
        RollPool pool{lds, P.part + (int64_t)blockIdx.x * P.rows * 4, 0, 0};
        roll_elements<kVec, kXf>(P, v, live, pool);
    } else {
        if (!live) return;
        RollNoPool pool;
        roll_elements<kVec, kXf>(P, v, true, pool);
    }
}

// out_pool[r][c] = the workgroups' partials in ascending group order
__global__ __launch_bounds__(256) void mcpc_roll_finish_kernel(const double* __restrict__ part, int64_t groups, int64_t total,
                                                               double* __restrict__ out_pool) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        double s = part[i];
        for (int64_t g = 1; g < groups; ++g) s = s + part[g * total + i];
        out_pool[i] = s;
    }
}

inline int64_t roll_groups(int64_t E, int kVec) { return (E / kVec + kRollBlock - 1) / kRollBlock; }

// the vector form where the row and EVERY pointer a lane reads or writes by vectors allow it
inline int roll_vec(const RollParams& P) {
    const uintptr_t align = (uintptr_t)P.rec | (uintptr_t)P.hist;
    return (P.E % 4 == 0 && align % 16 == 0) ? 4 : 1;
}

template <int kVec>
inline void roll_launch(int transform, RollParams P, double* out_pool, hipStream_t stream) {
    P.n_vec = P.E / kVec;
    const int64_t groups = roll_groups(P.E, kVec);
    const dim3 grid((unsigned)groups), block(kRollBlock);
    const bool sig = transform == MCPC_MOM_SIGMOID;
    if (out_pool) {
        if (sig) hipLaunchKernelGGL((mcpc_roll_kernel<kVec, 1, true>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((mcpc_roll_kernel<kVec, 0, true>), grid, block, 0, stream, P);
        if (P.rows > 0) {
            const int64_t total = P.rows * 4;
            const int64_t blocks = (total + 255) / 256;
            hipLaunchKernelGGL(mcpc_roll_finish_kernel, dim3((unsigned)(blocks < kMomMaxBlocks ? blocks : kMomMaxBlocks)), dim3(256), 0,
                               stream, (const double*)P.part, groups, total, out_pool);
        }
    } else {
        if (sig) hipLaunchKernelGGL((mcpc_roll_kernel<kVec, 1, false>), grid, block, 0, stream, P);
        else hipLaunchKernelGGL((mcpc_roll_kernel<kVec, 0, false>), grid, block, 0, stream, P);
    }
}
}  // namespace mcpc
