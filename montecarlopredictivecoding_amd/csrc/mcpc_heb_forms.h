// What the host knows of the Hebbian kernels (mcpc_hebbian.h) without seeing them: their arguments, the <TE, RA, SWAPPED> forms they are
// instantiated for, their dynamic LDS, and the jobs of the slab reduction.  The planner (mcpc_plan.h: plan_hebbian, plan_flush) resolves
// every launch of a flush from this header alone; the kernels themselves are compiled into one translation unit, mcpc_flush.hip.
#pragma once
#include "mcpc_types.h"

namespace mcpc {

constexpr int kHebKB = 32;           // spilled rows per stage
constexpr int kHebThreads = 512;

struct HebArgs {
    const float* E;                  // [rows][ne]   spilled errors (row stride ne: padded width)
    const float* A;                  // [rows][na]   spilled activations
    float* slab;                     // [ksplit][ne][na]
    float* slab_b;                   // [ksplit][ne]
    int rows, ne, na;                // rows % 32 == 0; ne, na multiples of 16
    int rows_per_split;              // multiple of 32
    int n_mt, n_nt, ksplit;          // error-tile groups, activation-tile groups, K splits: grid = n_mt * n_nt * ksplit workgroups
    int e_col_base;                  // first E column of this launch (a Linear may be covered by launches of different TE)
    const unsigned* e_max;           // mcpc_heb7_kernel: bit pattern of the largest |value| in the E image of this segment, and in the A image:
    const unsigned* a_max;           //   the powers of two its fp16 operands are scaled by (written by the step kernels: KParams::spillmax)
};

#ifndef MCPC_HEB_LDS_PAD
#define MCPC_HEB_LDS_PAD 16        // floats added to a 256-float panel row in LDS (0: the linear image of round 2, for A/B runs)
#endif
constexpr int heb_lds_stride(int row_floats) { return row_floats == 256 ? row_floats + MCPC_HEB_LDS_PAD : row_floats; }
// dynamic LDS of mcpc_heb_kernel<TE, RA, *>: two stages of both panels (host side: the launch, mcpc_flush.hip)
constexpr int heb_lds_bytes(int te, int ra) { return 2 * kHebKB * (heb_lds_stride(16 * te) + heb_lds_stride(16 * 8 * ra)) * (int)sizeof(float); }

// The <TE, RA, SWAPPED> forms BOTH tiled kernels are instantiated for, listed once: the planner resolves every launch of a flush to an
// index into this list (mcpc_plan.h: plan_flush), the executor's kernel table is built from it (mcpc_flush.hip).
#define MCPC_HEB_FORMS(X) X(17, 2, false) X(17, 1, false) X(16, 2, false) X(16, 1, false) X(8, 2, false) X(8, 1, false) \
                          X(1, 2, true) X(2, 2, true) X(4, 2, true)
struct HebForm { int te, ra; bool swapped; };
#define MCPC_HEB_FORM_ROW(te, ra, sw) {te, ra, sw},
constexpr HebForm kHebForms[] = {MCPC_HEB_FORMS(MCPC_HEB_FORM_ROW)};
#undef MCPC_HEB_FORM_ROW
constexpr int kNumHebForms = (int)(sizeof(kHebForms) / sizeof(kHebForms[0]));
constexpr int heb_form_index(int te, int ra, bool swapped) {            // -1: no such instantiation
    for (int i = 0; i < kNumHebForms; ++i)
        if (kHebForms[i].te == te && kHebForms[i].ra == ra && kHebForms[i].swapped == swapped) return i;
    return -1;
}

constexpr int kHeb7KB = 32;            // spilled rows per stage = K of one bf16 MFMA = two row tiles
constexpr int kHeb7LD = 40;            // bf16 elements between the rows of two units in an LDS plane: 32 of data + 8 of padding (80 B)
// dynamic LDS of mcpc_heb7_kernel<TE, *, *>: two plane buffers + the bias sums + every wave's transpose scratch for one activation tile
// (2 row tiles x 4 x 17 float4) (host side: the launch, mcpc_flush.hip)
constexpr int heb7_lds_bytes(int te) { return 2 * 2 * 16 * te * kHeb7LD * 2 + 16 * te * (int)sizeof(float) + 8 * 2 * 272 * (int)sizeof(float); }

// ---- fixed-order slab reduction for every Linear of a flush in ONE launch ---------------------------------------------
struct ReduceJob {
    const float* slab;     // [ksplit][n]
    float* dst;            // [n]
    int n, ksplit;
    float sign;
    int tr_cols, tr_ld;    // tr_cols > 0: the slab holds the transposed matrix [n / tr_cols][tr_cols]; element idx goes to
                           // dst[(idx % tr_cols) * tr_ld + idx / tr_cols]
};
constexpr int kMaxReduceJobs = 2 * (kMaxLatent + 1);
struct ReduceJobs {
    ReduceJob job[kMaxReduceJobs];
    int n_jobs;
};

}  // namespace mcpc
