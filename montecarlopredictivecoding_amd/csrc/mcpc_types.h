// What the host code (planner, engine, executor) and the kernels agree on, and nothing that is a kernel: the parameter structs and table
// entries a launch carries, the tile shapes of every kernel form, the ids of the spilled tensors and of the row-exponent words, and the
// small device helpers several kernel headers use.  Every translation unit of the library may include it; a header that DEFINES a
// kernel is included by the one unit that launches it.
#pragma once
#include "mcpc_device.h"
#include "../../include/mcpc.h"

namespace mcpc {

constexpr int kMaxLatent = MCPC_MAX_LATENT;
constexpr int kBatchPad = 32;     // the batch is padded to a multiple of this (plan_engine: Bpad); a workgroup owns 16 chains = one MFMA column tile
constexpr int kWaves = 4;         // waves per workgroup of the default variant; kMaxWaves bounds the LDS scratch
constexpr int kMaxWaves = 8;
constexpr int kThreads = kWaves * 64;
constexpr int kNT = 4;            // unit tiles per wave per phase with 4 waves (2 with 8 waves): a phase hands out 16 tiles
constexpr int kChunkTiles = 16;   // read-out units processed per chunk = 256
constexpr int kLdPad = 4;         // LDS row padding (floats)
constexpr int kEnergyCols = kMaxLatent + 2;   // loss, E_1..E_L(max), overall

struct KLayer {
    float* x;              // state [Bpad][npad]
    float* m;              // Adam exp_avg    [Bpad][npad]
    float* v;              // Adam exp_avg_sq [Bpad][npad]
    float* xgrad;          // gradients-only mode: [B][n] (unpadded, caller's tensor)
    float* rec;            // trajectory records [rec_count][B][n] (unpadded) or null
    float* spill_e;        // l>=1: [slots][Bpad][npad] errors;  l==0: running sum of e_1 [Bpad][npad]
    float* spill_a;        // [slots][Bpad][npad] activations f(x_l)
    int spill_e_tm, spill_a_tm;   // 1: that image is TILE-MAJOR (spill_offset): what the fp16 Hebbian kernel reads (mcpc_heb7_kernel); 0: row-major
    const float* ext_noise;// [n_steps][B][n] or null
    const f32x4* Wf;       // l>=1: packed forward weights of Linear l  [ntiles][nkb_in][64]
    const f32x4* Wb;       // l>=1: packed backward weights of Linear l [ntiles(l-1)][ntiles][64]
    const float* bias;     // l>=1: padded bias [npad]
    int n, npad, ntiles;   // units, padded to 16, npad/16
    int act;
    float ecoef;
    int lds_a, lds_e;      // float offsets of FX_l / E_l in LDS
    int ld;                // LDS row stride (floats) = npad + kLdPad
    int lds_x;             // KParams::xl: float offset of the state rows X_l (row stride ld)
    int lds_bias;          // KParams::xl: float offset of the bias row [npad] (l >= 1) / of the mu_1 rows (l == 0, row stride ld)
};

struct KHead {
    const f32x4* Wf;       // [ntiles][nkb_in][64]
    const f32x4* Wb;       // [ntiles(L-1)][ntiles][64]
    const float* bias;     // [npad]
    const float* y;        // padded target [Bpad][npad]
    const float* ytile;    // the same image tile-major (tile_major_offset): what the lean read-out epilogue reads of an fp32 target
    const uint32_t* ybits; // the same bit-packed, [Bpad][ywords] (bit u & 31 of word u >> 5 = y[chain][u]); valid iff *y_binary
    const int* y_binary;   // device flag set by mcpc_bind_target: every target value is exactly 0.0f or 1.0f
    const int* y_bounded;  // device flag set by mcpc_bind_target: every target value lies in [-1, 2] (headb_fixed_exp)
    int ywords;            // words per chain = ceil(npad / 32)
    float* rec_out;        // [rec_count][B][n] or null
    float* spill_e;        // [slots][Bpad][npad]
    int spill_tm;          // 1: tile-major (see KLayer::spill_e_tm)
    int n, npad, ntiles;
    int loss_kind;
    float inv_var;
    int mask_start;
    int lds_eo;            // float offset of the read-out error chunk
    int ld;                // its row stride = kChunkTiles*16 + kLdPad
    int lds_bias;          // KParams::xl: float offset of the bias row [npad]
    int lds_yw;            // KParams::xl: float offset of the bit-packed target rows [chains][ywords]; < 0 (unified-wave kernel, a plan without
                           // the room): they stay in global memory
};

// One entry of the per-step phase table (built on the host, identical for every step):
//   [prologue loads] -> acc = (from accb | 0) -> GEMM over nkb k-blocks -> [acc -> accb] -> epilogue -> [barrier]
enum : int { PH_FWD = 0, PH_HEADF = 1, PH_HEADB = 2, PH_BWD = 3, PH_ENERGY = 4, PH_NOP = 5 };   // (PH_NOP: unified-wave kernel, a row without work)
enum : int { PHF_ACC_FROM_B = 1, PHF_ACC_TO_B = 2, PHF_SYNC = 4, PHF_MU1 = 8 };
struct KPhase {
    const void* A;         // packed weight fragments of this GEMM (unused when nkb == 0): layout of the GEMM core in use
    int type;              // PH_*
    int layer;             // FWD: layer whose prediction error is produced; BWD: layer whose x is updated
    int tile0, ntiles;     // output unit tiles of the phase; wave w owns tiles tile0 + w + 4 i
    int a_tile_stride;     // 16-byte units between the fragments of consecutive output tiles
    int a_off0;            // 16-byte offset of the first k-block of the k-window
    int nkb;               // k-blocks of kKB (0: no GEMM -- top-layer pass, update without back-projection)
    int kw;                // valid k width of the B rows (a multiple of 16 in (32 (nkb - 1), 32 nkb]): B lanes beyond it read as zeros
    int b_lds, ldb;        // B operand: LDS float offset and row stride
    int flags;             // PHF_*
    float sign;            // BWD: g = e + sign * f'(x) * back
    int out_lds, out_ld;   // HEADF: LDS offset / row stride of the e_o chunk this phase writes
    int dep_e, dep_g;      // wave-specialised kernels: entry whose completion by all E / all G waves must precede (-1: none;
                           // in-place variant: an index above the entry's own refers to the previous step)
    int a_lin;             // Linear whose packed weights A points into: KParams::wexp[a_lin] is the exponent they were scaled by
    int rot;               // in-place variant: pair k owns tiles tile0 + ((k + rot) & 3) + 4 i (balances uneven chunks);
                           // unified-wave kernel: the tile stride of a wave's row -- its tiles are tile0 + rot i, i < ntiles
    int dep_se;            // in-place variant: entry all E waves must have passed before this entry's block is STORED (its
                           // LDS rows are still read by their epilogues); dep_g is waited for at the same point
    int next_g;            // in-place variant: the next entry (cyclic) in which the GEMM waves have work -- they visit no other
    int b_row, o_row;      // in-place variant: id of the B operand's / of the produced operand's row-exponent words (KParams::lds_rowexp;
                           // -1: none -- the GEMM wave scans the row itself)
};

// Phase descriptors are fetched through the constant address space: wave-uniform s_load_* on the scalar cache.
// (Through a generic pointer hipcc emits a vector load + readfirstlane and an `s_waitcnt vmcnt(0)` that drains the
// weight-fragment prefetch at every phase boundary, and keeps the descriptor in scratch.)
__device__ __forceinline__ KPhase load_phase(const KPhase* tbl, int p) {
    typedef __attribute__((address_space(4))) const int cint;
    cint* w = (cint*)(tbl + p);
    union { KPhase ph; int v[sizeof(KPhase) / 4]; } u;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(KPhase) / 4); ++i) u.v[i] = w[i];
    return u.ph;
}

struct KParams {
    KLayer layer[kMaxLatent];
    KHead head;
    const KPhase* phases;  // [n_phases] in device memory
    const int* wexp;       // [kMaxLatent + 1]: per Linear, the power of two its packed weights are scaled by (mcpc_wexp_kernel)
    unsigned* spillmax;    // [kSpillTensors] bit patterns of the largest |value| spilled per tensor in this Hebbian segment (null: no spill):
                           // the fp16 Hebbian GEMM scales its operands by powers of two taken from them (mcpc_hebbian.h)
    int lds_spillmax;      // LDS float offset of the workgroup's own maxima (kSpillTensors words, zero at launch)
    int n_phases;
    int stagger_cycles;    // workgroups >= 256 (the second resident on a CU) start this many cycles late
    const float* mu1;      // prediction of the top latent layer [Bpad][npad_0] (inputs W0^T + b0)
    const float* adam_coef;// [n_steps][2]: -step_size = -lr/(1-b1^t), sqrt(1-b2^t)
    double* epart;         // [energy rows][nWG][kEnergyCols] per-workgroup partial sums
    int L, has_head;
    int B, Bpad;
    int T, t0, n_steps;
    int xopt, update_x;
    float lr, beta2, omb1, omb2, eps;
    int noise_mode;
    float noise_scale;     // sqrt(noise_var*lr)
    uint64_t seed, step_base, chain_base;
    int acc_begin, acc_end, spill_t0;   // spill slot of step t = t - spill_t0 when acc_begin <= t < acc_end
    int energy_mode;
    int rec_begin, rec_stride, rec_count;
    int lds_red;           // float offset of the energy reduction scratch [2][kMaxLatent+1][kMaxWaves]
    int lds_ws_sync;                 // wave-specialised kernel: float offset of the progress counters
    int ws_prio;                     // 1: epilogue waves run at raised static priority
    int* err;                        // device error word (bit 0/1: a progress-counter wait ran out)
    // in-place kernel, round schedule (plan_rounds in mcpc_plan.h, run_round_cycle in mcpc_run.hip): workgroup -> 16-chain unit and the launches of
    // the cycle that unit has already taken part in
    const int* wg_list;              // [gridDim.x] unit index, or null: unit = blockIdx.x
    const int* wg_rel;               // [gridDim.x] launches of this cycle the unit has already run, or null
    int rr_q;                        // steps per launch of the cycle
    int epart_slots;                 // in-place kernel: energy partials are indexed by 16-chain tile, this many per row
    int lean_ok;                     // in-place kernel: every [Bpad][npad] image is < 4 GiB and Bpad < 2^24 (32-bit lane offsets)
    const void* dummy;               // 4 KiB of valid device memory: what the branch-free fragment prefetch reads for entries without a GEMM
    int xl;                          // in-place kernel, 16-chain plans whose LDS has the room: the state x_l, the biases, mu_1 and the bit-packed
                                     // target of the workgroup's chains live in LDS for the whole launch (mcpc_ws2_lean.h: XL)
    int spill_sys;                   // Hebbian spill stores at system scope (write-through): shards whose spill per step is far beyond the L2s
    int lds_floats;                  // floats of dynamic LDS of this plan (cleared once per launch: see mcpc_gemm_f16.h, k ranges)
    int g_first;                     // in-place variant: first table entry with work for the GEMM waves (-1: none)
    int lds_rowexp;                  // float offset of kRowExpIds x 16 words: per B operand and chain row, (generation << 8) | biased exponent of
                                     // the row's largest |value|, kept by the epilogue waves that WRITE the rows (rowexp_track below)
    int lds_zero;                    // float offset of 16 floats of the plan that nothing writes after that: what the GEMM core's lanes beyond a
                                     // ragged k range read (mcpc_gemm_f16.h)
    unsigned long long* clk;         // profiling only (else null): [0] += shader cycles (s_memtime), [1] += 100 MHz wall ticks (s_memrealtime)
                                     // of one wave of workgroup 0 over the launch -- their ratio is the shader clock under THIS load
#ifdef MCPC_STAMPS
    unsigned long long* dbg;   // diagnostic build only: [nwg][kWaves][16] cycle sums per phase
#endif
};

// Layout of images only the epilogues read or write -- Adam's moments m_l, v_l, the tile-major copy of an fp32 target: TILE-MAJOR --
// the 16 chains x 16 units a wave's float4 access covers are one contiguous KiB, in lane order, instead of sixteen 64-byte pieces of
// sixteen rows.  A row-major access costs the CU's vector-memory path about 100 cycles per wave instruction, a contiguous one a
// fraction of that, and that path is what the step kernel is bound by: the MAP warm-up (Adam on x) took 62.4 us
// per step at cfg-M with row-major moments against 52.0 for SGD with the kick.
// Float offset of units u0 .. u0+3 (u0 a multiple of 4) of `chain` in an image of npad-wide rows:
__device__ __forceinline__ size_t tile_major_offset(int chain, int u0, int npad) {
    return (((size_t)(chain >> 4) * (npad >> 4) + (u0 >> 4)) * 64 + (chain & 15) + 16 * ((u0 >> 2) & 3)) * 4;
}

// Float offset of units u0 .. u0+3 of `row` in a spilled image [rows][npad]: row-major, or tile-major (tile_major_offset) -- the layout in
// which the float4-per-lane store of an epilogue wave (16 rows x 16 units) is one contiguous KiB and which mcpc_heb7_kernel reads.
__device__ __forceinline__ size_t spill_offset(int tm, size_t row, int u0, int npad) {
    return tm ? (((row >> 4) * (size_t)(npad >> 4) + (size_t)(u0 >> 4)) * 64 + (row & 15) + 16 * ((u0 >> 2) & 3)) * 4
              : row * (size_t)npad + (size_t)u0;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// ---- largest |value| per spilled tensor (for the Hebbian GEMM's operand scaling) ---------------------------------------------------------
// tensor ids: activations A_l = l, errors E_l = kMaxLatent + l, read-out errors E_o = 2 kMaxLatent
constexpr int kSpillTensors = 16;
__host__ __device__ __forceinline__ int spill_id_a(int l) { return l; }
__host__ __device__ __forceinline__ int spill_id_e(int l) { return kMaxLatent + l; }
constexpr int kSpillIdEo = 2 * kMaxLatent;
__device__ __forceinline__ float absmax4(float m, f32x4 v) {
    return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}
// the lanes' maxima over what an epilogue call spilled of one tensor -> the workgroup's running maximum of that tensor in LDS
// (non-negative floats order like their bit patterns)
__device__ __forceinline__ void spill_track(float* lds_max, int id, float lane_max, int lane) {
    const float m = wave_max(lane_max);
    if (lane == 0) atomicMax(reinterpret_cast<unsigned*>(lds_max) + id, __float_as_uint(m));
}
// a wave that has finished its steps adds the workgroup's maxima (as far as they are known) to the segment's
__device__ __forceinline__ void spill_max_publish(unsigned* gmax, const float* lds_max, int lane) {
    if (gmax != nullptr && lane < kSpillTensors) {
        const unsigned bits = reinterpret_cast<const volatile unsigned*>(lds_max)[lane];
        if (bits != 0u) atomicMax(gmax + lane, bits);
    }
}

// streamed once per step (state, targets, spills): nontemporal, so the per-XCD L2 (4 MiB) keeps the
// 2.2 MB of packed weights every workgroup re-reads instead of cycling 4 MB of chain data through it
__device__ __forceinline__ f32x4 ld4s(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void st4s(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }
__device__ __forceinline__ f32x4 splat(float v) { f32x4 r = {v, v, v, v}; return r; }

// ---- shapes of the kernel forms: what the planner sizes tables, grids and LDS by ---------------------------------------------------------
// GEMM core (mcpc_gemm_f16.h)
constexpr int kKB = 32;                 // k-depth of one fragment block
constexpr int kFragBlock = 2 * 64;      // u32x4 units per (tile, k-block): two fp16 planes of 64 lanes
constexpr int kShortK = 2;              // GEMMs of at most this many k-blocks (K <= 64) keep the fourth product a_m b_m

// wave-specialised kernels (mcpc_steps_ws.h)
enum : int { PHF_WS_GEMM = 16, PHF_WS_EPI = 32 };   // which role has work in a table entry
enum : int { PHF_WS2_HANDOFF = 64 };                // in-place kernel: BWD entry without GEMM whose block (accb) still comes from G

// ids of the row-exponent words the producers of a GEMM's B rows keep (mcpc_kernels.h: rowexp_track, rowexp_read)
constexpr int kRowExpIds = 16;                         // FX_0..5, E_0..5, ring slots 0..3
constexpr int kRowExpFloats = kRowExpIds * 16;
__device__ __host__ __forceinline__ int rowexp_fx(int l) { return l; }
__device__ __host__ __forceinline__ int rowexp_e(int l) { return kMaxLatent + l; }
__device__ __host__ __forceinline__ int rowexp_ring(int r) { return 2 * kMaxLatent + r; }

// in-place kernel (mcpc_steps_ws2.h)
#ifndef MCPC_WS2_PAIRS
#define MCPC_WS2_PAIRS 4
#endif
constexpr int kWs2Pairs = MCPC_WS2_PAIRS;          // (G, E) pairs per workgroup: 4 = one GEMM and one epilogue wave per SIMD.
                                                   // (8 = two of each: measured 99 vs 95 us per step at cfg-M -- the two GEMM waves of a SIMD walk the
                                                   // same table behind the same dependencies, so they stall together instead of filling each other's gaps)
#ifndef MCPC_WS2_SPAN
#define MCPC_WS2_SPAN 16
#endif
constexpr int kWs2NT = MCPC_WS2_SPAN / kWs2Pairs;   // unit tiles per pair per table entry: an entry hands out 16 tiles
// Tiles per pair and entry (build-time knob).  Measured: 6 (a third group of two tiles in the register rotation) and 5 against 4 --
// 50.7 / 50.0 / 51.4 us per step at 4096 chains in round 2, 34.9 against 34.4 with the bf16x6 core in round 3: the hand-over count is
// not what a step pays for, and the default stays 4 (one table layout; mcpc_gemm_f16.h's rotation is written for at most four).
#ifndef MCPC_WS2_NT16
#define MCPC_WS2_NT16 kWs2NT
#endif
constexpr int kWs2NTW = MCPC_WS2_NT16;
constexpr int kWs2Threads = 2 * kWs2Pairs * 64;
static_assert(kWs2Pairs == 4 || kWs2Pairs == 8, "4 or 8 pairs");

// unified-wave kernel (mcpc_steps_u.h)
constexpr int kUWaves = 8;                      // waves per workgroup, all alike (two per SIMD)
constexpr int kUNT = 4;                         // unit tiles per row (job) at most: the four fragment slots and accumulator tiles of a wave
constexpr int kUThreads = kUWaves * 64;

// layer-wise kernels and the evaluators that share their tile (mcpc_steps_lw.h, mcpc_chain_energy.h)
constexpr int kLwChains = 64;                       // chains per workgroup
constexpr int kLwCTT = kLwChains / 16;              // chain tiles per wave
constexpr int kLwWaves = 4;
constexpr int kLwThreads = kLwWaves * 64;
constexpr int kLwUTW = 2;                           // unit tiles per wave
constexpr int kLwUnitTiles = kLwWaves * kLwUTW;     // unit tiles per workgroup (128 units)
constexpr int kLwLd = kKB + 4;                      // floats per chain row of a staged k-block
constexpr int kLwStageFloats = 2 * kLwChains * kLwLd;
constexpr int kLwLdsBytes = (kLwStageFloats + kLwChains + kLwWaves + 2) * 4;     // staging, row exponents, energy partials, spill maxima

struct LwJob { int layer; int ut0; };               // forward: Linear j (layer L = the read-out); backward: latent layer l; first unit tile

struct CeFinish {
    int first[kMaxLatent + 1], count[kMaxLatent + 1];      // the jobs of Linear j in the table ([L]: the read-out), contiguous and ascending
};

}  // namespace mcpc
