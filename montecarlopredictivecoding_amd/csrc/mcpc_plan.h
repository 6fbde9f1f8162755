// Host-side planning of an engine: everything mcpc_create decides BEFORE it allocates -- padded shapes, the step-kernel form and its
// fallbacks, the LDS plans and step tables, the layer-wise job tables, the round schedule, the spill ring's size -- and what mcpc_run
// decides before it launches: the schedule of a run (plan_run) and every launch of its Hebbian flushes (plan_flush).  Plain host code
// that makes no HIP call, so it runs (and is tested: mcpc_debug_plan, tests/test_plan_host.py; mcpc_debug_run_plan,
// tests/test_run_plan_host.py) without a device.  It sees no kernel: the table types and tile shapes it plans with are in mcpc_types.h,
// the Hebbian kernels' forms in mcpc_heb_forms.h.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mcpc_heb_forms.h"
#include "mcpc_host.h"
#include "mcpc_types.h"

namespace mcpc {

inline int pad16(int n) { return (n + 15) / 16 * 16; }
inline int kblocks(int k_pad) { return (k_pad + kKB - 1) / kKB; }      // k-blocks of the GEMM core that cover k_pad (a multiple of 16)
// which Linears (et x at tiles of 16) take the LDS-tiled Hebbian kernels (mcpc_hebbian.h): wide ones, and 256 outputs with a narrow input
inline bool heb_wide(int et, int at) { return et >= 8 && at % 8 == 0 && (at <= 16 || at % 16 == 0); }
inline bool heb_narrow_in(int et, int at) { return !heb_wide(et, at) && et == 16 && (at == 1 || at == 2 || at == 4); }
constexpr int kLdsLimit = 160 * 1024;       // bytes of LDS a workgroup can have

// A Linear: its shapes and spill layout are planned; the pointers belong to the engine (null in a plan)
struct Lin {
    const float* W = nullptr;      // borrowed, torch layout [out][in]
    const float* bias = nullptr;   // borrowed or null
    bool bound = false;
    int n_out = 0, n_in = 0, out_pad = 0, in_pad = 0;
    float* Wf = nullptr;           // packed forward  [out_tiles][in_tiles][64][4]
    float* Wb = nullptr;           // packed backward [in_tiles][out_tiles][64][4]
    float* bias_pad = nullptr;     // [out_pad]
    float* G = nullptr;            // gradient sums [out_pad][g_ld]
    float* Gb = nullptr;           // [out_pad]
    int g_ld = 0;
    bool spill_tm = false;         // its Hebbian operands are spilled tile-major (the fp16 kernel mcpc_heb7_kernel reads them)
    size_t slab_off = 0;           // float offset of this Linear's split-K slabs inside mcpc_engine::slab (plan_engine)
    size_t slab_floats = 0;        // ... and their size: `slab_splits` weight and bias slabs, the most K-splits a flush of a whole
    int slab_splits = 0;           //     ring part asks for (HebPlan::ksplit_cap)
};

// Developer overrides of the schedule heuristics, parsed ONCE from mcpc_net_desc::tuning at mcpc_create
// ("key=value,key=value"; see include/mcpc.h).  The library itself reads no environment variables.
constexpr int kMaxRingParts = 8;
struct Knobs {
    int ws = -1;              // -1: automatic; 0: barrier kernel; 2: in-place wave-specialised kernel everywhere; 3: insist on the unified-wave
                              // kernel (mcpc_steps_u.h) for the runs it serves (create fails when its LDS plan does not fit); 4: the layer-wise
                              // kernels (mcpc_steps_lw.h) for every run, whatever the widths
    int wide = 0;             // 1: a network no LDS plan serves (mcpc_create would fail with MCPC_ENOMEM) runs on the layer-wise kernels instead
    int no_overlap = 0;       // 1: Hebbian flushes run serially on the caller's stream (one ring segment = the whole ring)
    int slot_cap = 384;       // spill-ring slots at most (3 parts of 128 steps)
    int spill_gb = 0;         // > 0: spill budget in GiB (overrides mcpc_net_desc::spill_budget_bytes)
    int cu_slack = 0;         // CUs the round schedule leaves free (launches of at most n_cu - cu_slack workgroups)
    int flush_streams = 2;    // low-priority streams the GEMMs of an overlapped flush are spread over (1 or 2)
    int flush_tail = 0;       // > 0: the last accumulating segment of a stretch is cut to this many steps (its flush is the one nothing overlaps)
    int ring_parts = 3;       // parts of the spill ring: one is filled by the step kernel, one is being flushed, one is slack -- with two
                              // halves the step kernel waited at every boundary for a flush that takes as long as its own segment
                              // (96.8 -> 95.2 us per step of the learning call; parts of 64 steps beat 48, 96 and 128)
    int dw_ksplit = 0;        // > 0: K-splits per workgroup tile of the Hebbian GEMM (0: one wave of workgroups over the chip)
    int ws_prio = 0;          // 1: epilogue waves at raised priority, 2: GEMM waves, 0: neither (the GEMM waves need most of the issue port
                              // themselves: with the epilogue waves at raised priority a step of cfg-M took 94.2 us against 87.7, round 3)
    int stagger = 0;          // barrier kernel: start cycles of the second workgroup of a CU
    int no_lean = 0;          // 1: the in-place kernel's E waves use the generic epilogues everywhere (A/B, parity tests)
    int no_ybits = 0;         // 1: 0/1 targets are read as fp32 like any other target (A/B, parity tests)
    int overlay16 = 0;        // 1: the ring and the E_l share their LDS, as the 32-chain plans of rounds 1-3 did (A/B, parity tests)
    int no_xl = 0;            // 1: 16-chain plans keep the state and the per-step constants in global memory even when the LDS has the room (A/B, parity tests)
    int rr = 1;               // 0: shards of more 16-chain units than CUs run as one launch in hardware rounds instead of the round schedule (plan_rounds)
    int rr_qmax = 100;        // round schedule: most steps per launch in stretches without Hebbian accumulation
    int heb171 = 0;           // 1: the 17-tile group of a read-out on <17, 1> with twice the activation groups instead of <17, 2> (A/B)
    int heb_fp32 = 0;         // 1: the tiled Hebbian GEMM runs on the fp32 MFMA (mcpc_heb_kernel) instead of the fp16x6 form (A/B, parity tests)
    int spec = 1;             // 0: every launch of the in-place kernel takes its generic instantiation, never a specialised one (A/B, parity tests)
    int spec_wait = 0;        // a run of at least this many steps waits for the host copy of the bound target's flags (mcpc_run.hip:
                              // target_flags_on_host); a shorter one specialises only if the copy has landed.  0, every candidate run
                              // waits: with a target bound in front of every call that won at every length from 4 steps up, and runs
                              // that only polled were 2 % behind the parent (profiles/spec_modes.txt section 7)
    // unified-wave kernel: the cost model its rows are dealt by (build_phases_u) -- developer knobs for its calibration.  The defaults started
    // from in-kernel stamps (shader cycles: 2000 / 1200 / 330 / 68 / 1000 / 1300 / 500) and were then moved by a grid search on the step time
    // itself (scripts/u_cost_search.py, profiles/r06_small_net.txt: 16.9 -> 16.1 us per MCPC step at batch 256): what the model has to get
    // right is the ORDER of the jobs' costs and where a split stops paying, and a row's fixed cost and the read-out's epilogue weigh more in
    // that than their stamps say (they sit on the level's critical path)
    int u_row = 5000;         // per row: descriptor, the next row's fragment requests, the epilogue's fixed part
    int u_gemm0 = 1200;       // per GEMM, before its first k-block
    int u_kb = 200;           // per k-block beyond its tiles' MFMAs and requests (the B split; nothing with the operand in planes)
    int u_kbt = 68;           // per k-block and tile
    int u_eh = 3000, u_eb = 1300, u_ef = 500;      // per tile of an epilogue: read-out / x update / prediction error
};

inline int parse_tuning(const char* str, Knobs& k) {
    if (!str) return 0;
    std::string s(str);
    size_t pos = 0;
    while (pos < s.size()) {
        size_t end = s.find_first_of(",;", pos);
        if (end == std::string::npos) end = s.size();
        std::string item = s.substr(pos, end - pos);
        pos = end + 1;
        while (!item.empty() && item.front() == ' ') item.erase(item.begin());
        while (!item.empty() && item.back() == ' ') item.pop_back();
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        const std::string key = item.substr(0, eq);
        const int val = eq == std::string::npos ? 1 : atoi(item.c_str() + eq + 1);
        struct { const char* name; int* dst; } table[] = {
            {"ws", &k.ws}, {"wide", &k.wide}, {"no_overlap", &k.no_overlap},
            {"slot_cap", &k.slot_cap}, {"spill_gb", &k.spill_gb}, {"cu_slack", &k.cu_slack}, {"ring_parts", &k.ring_parts}, {"flush_tail", &k.flush_tail}, {"flush_streams", &k.flush_streams}, {"dw_ksplit", &k.dw_ksplit},
            {"ws_prio", &k.ws_prio}, {"stagger", &k.stagger}, {"no_lean", &k.no_lean}, {"no_ybits", &k.no_ybits}, {"overlay16", &k.overlay16}, {"heb_fp32", &k.heb_fp32}, {"heb171", &k.heb171}, {"rr", &k.rr}, {"rr_qmax", &k.rr_qmax}, {"no_xl", &k.no_xl}, {"spec", &k.spec}, {"spec_wait", &k.spec_wait},
            {"u_row", &k.u_row}, {"u_gemm0", &k.u_gemm0}, {"u_kb", &k.u_kb}, {"u_kbt", &k.u_kbt}, {"u_eh", &k.u_eh}, {"u_eb", &k.u_eb}, {"u_ef", &k.u_ef}};
        bool found = false;
        for (auto& t : table)
            if (key == t.name) { *t.dst = val; found = true; }
        if (!found) return fail(MCPC_EINVAL, "unknown tuning key '%s' in mcpc_net_desc::tuning", key.c_str());
    }
    if (k.ws != -1 && k.ws != 0 && k.ws != 2 && k.ws != 3 && k.ws != 4)
        return fail(MCPC_EINVAL, "tuning ws=%d: 0 (barrier kernel), 2 (in-place kernel), 3 (unified-wave kernel) or 4 (layer-wise kernels)", k.ws);
    if (k.ws == 4) {
        // knobs of the LDS-resident kernels have nothing to act on: an incompatible pair is an error of its own, not a silent no-op
        const Knobs dflt;
        const struct { const char* name; bool set; } lds_only[] = {
            {"no_lean", k.no_lean != 0}, {"no_xl", k.no_xl != 0}, {"overlay16", k.overlay16 != 0}, {"rr", k.rr != dflt.rr},
            {"u_row", k.u_row != dflt.u_row}, {"u_gemm0", k.u_gemm0 != dflt.u_gemm0}, {"u_kb", k.u_kb != dflt.u_kb}, {"u_kbt", k.u_kbt != dflt.u_kbt},
            {"u_eh", k.u_eh != dflt.u_eh}, {"u_eb", k.u_eb != dflt.u_eb}, {"u_ef", k.u_ef != dflt.u_ef}};
        for (auto& t : lds_only)
            if (t.set) return fail(MCPC_EINVAL, "tuning ws=4 (layer-wise kernels) together with %s, a knob of the LDS-resident kernels", t.name);
    }
    if (k.slot_cap < 2) k.slot_cap = 2;
    if (k.cu_slack < 0) k.cu_slack = 0;
    if (k.ring_parts < 2 || k.ring_parts > kMaxRingParts) return fail(MCPC_EINVAL, "tuning ring_parts=%d: 2..%d", k.ring_parts, kMaxRingParts);
    return 0;
}

// What a step-kernel form's plan is: where its operands live in the workgroup's LDS, and the table its waves walk every step.
struct LdsRegion { const char* name; int layer; int off, floats; };      // (layer -1: not per layer)
struct StepPlan {
    int lds_a[kMaxLatent]{}, lds_e[kMaxLatent]{}, lds_x[kMaxLatent]{}, lds_bias[kMaxLatent]{};       // FX_l, E_l; with xl: X_l, bias / mu_1 rows
    int lds_eo = 0, lds_red = 0, lds_ws_sync = 0, lds_spillmax = 0, lds_rowexp = 0, lds_hbias = 0, lds_yw = 0, lds_bytes = 0;
    int lds_zero = 0;               // 16 floats nothing writes: the GEMM core's over-reading lanes read them (KParams::lds_zero)
    int head_ld = kChunkTiles * 16 + kLdPad;       // row stride of the read-out error rows (KHead::ld)
    bool xl = false;                // state rows, biases, mu_1 rows and target words live in LDS (KParams::xl)
    int g_first = -1;               // in-place table: first entry with work for the GEMM waves (build_phases_ws2)
    int ws2_chunk = 0, ws2_ring = 0; // in-place plan: read-out tiles per chunk, chunks in the LDS ring
    bool ws2_overlay = true;        // the ring of read-out error chunks shares LDS with E_1 .. E_{L-1}; plans that fit keep them apart,
                                    // which frees the order of the forward entries (build_phases_ws2)
    std::vector<LdsRegion> regions; // every region handed out, in order (mcpc_debug_plan)
    std::vector<KPhase> table;      // the step table; KPhase::A is null until mcpc_create binds it to the packed weights
    int n_phases = 0;               // entries a wave walks per step (the unified-wave table holds kUWaves rows of them)
    KPhase* dev = nullptr;          // device copy of `table` (owned by the engine)
    int take(const char* name, int layer, int& off, int floats) { regions.push_back({name, layer, off, floats}); off += floats; return off - floats; }
};

// LDS plan and step table of the unified-wave kernel (mcpc_steps_u.h), kept BESIDE the engine's main plan: use_unified
// picks the kernel per run (lean runs: fused SGD update with or without the Philox kick, Adam without noise), everything else stays
// on the main plan's kernel.
struct UPlan {
    bool ok = false;                // the plan fits the LDS (whole read-out error + state rows resident)
    bool on = false;                // ... and the engine holds its table (automatic tuning, or ws=3)
    bool prefer = false;            // ... and uses it for every lean run (tuning ws=3, or the automatic choice: choose_unified); otherwise
                                    // only for zero-loss runs, whose read-out this kernel alone skips on the steps nobody records
    StepPlan plan;
};

struct EnginePlan {
    Knobs knobs;
    int L = 0, Bpad = 0, nwg = 0, has_head = 0;
    int nwg_live = 0;               // 16-chain in-place plans: workgroups that hold at least one chain of the batch (Bpad is a multiple of 32, so
                                    // the last 16-chain unit may be all padding: it is never launched -- its spill rows and energy slots stay zero);
                                    // layer-wise kernels: workgroups of the forward launch
    static constexpr int ct = 16;   // chains per workgroup: one MFMA column tile (the 32-chain forms of rounds 1-3 left the tree in round 4)
    int nw = kWaves;                // waves per workgroup: 4 (barrier kernel) or 8 (in-place kernel: 4 GEMM + 4 epilogue waves)
    int ws = 0;                     // 0: barrier kernel (the fallback); 2: in-place wave-specialised kernel
    bool lw = false;                // layer-wise kernels (mcpc_steps_lw.h): no LDS plan, no step table
    int npad[kMaxLatent]{};
    int out_pad = 0;
    Lin lin[kMaxLatent + 1];
    StepPlan main;                  // plan of the main form (barrier or in-place kernel; layer-wise: only lds_bytes)
    UPlan u;                        // unified-wave kernel: its own LDS plan and table
    std::vector<LwJob> lw_table;    // layer-wise kernels: forward jobs, then backward jobs
    int lw_nf = 0, lw_nb = 0;       // ... how many of each (= gridDim.y of the two launches)
    // Round schedule (plan_rounds): a shard of more 16-chain units than CUs as `rr_k` launches per cycle, each unit in `rr_m` of them
    bool rr = false;
    int rr_k = 0, rr_m = 0;
    std::vector<int> rr_count, rr_off;   // per launch of a cycle: workgroups, offset of its [ids][rel] rows in rr_host
    std::vector<int> rr_host;
    std::string rr_name;                 // mcpc_step_kernel_name of an engine on the round schedule
    std::string u_rr_name;               // ... when its fused calls run on the unified-wave kernel
    // Hebbian spill ring: `slots` steps in parts of `half_slots`; the flush of one part runs on `aux` while the step kernel fills another
    int slots = 0, half_slots = 0;
    size_t slot_bytes = 0;          // ... and the bytes one step spills
    size_t slab_floats = 0;         // the split-K slabs of all Linears j >= 1 (Lin::slab_off, slab_floats)
};

// the pair of launches a step on the layer-wise kernels is (mcpc_step_kernel_name, mcpc_last_step_kernel_name: as a trace shows them)
static const char* const kLwName = "mcpc::mcpc_lw_fwd_kernel + mcpc::mcpc_lw_bwd_kernel";

inline KPhase blank_phase() { KPhase k{}; k.dep_e = -1; k.dep_g = -1; k.dep_se = -1; k.b_row = -1; k.o_row = -1; return k; }
// the GEMM of a table entry over the packed weights of Linear `a_lin` (KPhase::A follows from a_lin and the entry's type: bind_table)
// with a B operand of `kw` valid columns
inline void set_gemm(KPhase& k, int a_lin, int kw) { k.a_lin = a_lin; k.kw = kw; k.nkb = kblocks(kw); k.a_tile_stride = k.nkb * kFragBlock; }

// LDS plan of the barrier kernel: activations ping-pong between two buffers (FX_l in buffer l&1), the read-out error
// chunk takes the buffer FX_{L-1} is NOT in, errors E_l (l>=1) get their own rows.
inline int plan_lds(const EnginePlan& e, StepPlan& p) {
    p = StepPlan{};
    int buf[2] = {0, 0};
    const int CT = e.ct;
    for (int l = 0; l < e.L; ++l) buf[l & 1] = std::max(buf[l & 1], CT * (e.npad[l] + kLdPad));
    const int eo_floats = e.has_head ? CT * (kChunkTiles * 16 + kLdPad) : 0;
    const int eo_buf = ((e.L - 1) & 1) ^ 1;
    buf[eo_buf] = std::max(buf[eo_buf], eo_floats);
    int off = 0;
    const int base[2] = {p.take("buf", 0, off, buf[0]), p.take("buf", 1, off, buf[1])};
    for (int l = 0; l < e.L; ++l) p.lds_a[l] = base[l & 1];
    p.lds_eo = base[eo_buf];
    for (int l = 1; l < e.L; ++l) p.lds_e[l] = p.take("e", l, off, CT * (e.npad[l] + kLdPad));
    p.lds_red = p.take("red", -1, off, 2 * (kMaxLatent + 1) * kMaxWaves);
    p.lds_zero = p.take("zero", -1, off, 16);            // (mcpc_gemm_f16.h: what lanes beyond a ragged k range read)
    p.lds_spillmax = p.take("spillmax", -1, off, kSpillTensors);     // the workgroup's largest |value| per spilled tensor (mcpc_kernels.h: spill_track)
    p.lds_bytes = off * (int)sizeof(float);
    if (p.lds_bytes > kLdsLimit)
        return fail(MCPC_ENOMEM, "network needs %d bytes of LDS per workgroup (> 163840): latent widths too large for the fused kernel", p.lds_bytes);
    return 0;
}

// What the lean epilogues read every step, resident in LDS (KParams::xl): the state rows X_l (layout of FX_l), the bias rows, the mu_1
// rows (layout of FX_0), the read-out bias and -- `with_yw` -- the bit-packed target rows.
inline void take_xl(const EnginePlan& e, StepPlan& p, int& off, bool with_yw) {
    for (int l = 0; l < e.L; ++l) p.lds_x[l] = p.take("x", l, off, e.ct * (e.npad[l] + kLdPad));
    for (int l = 0; l < e.L; ++l) p.lds_bias[l] = p.take("bias", l, off, l >= 1 ? e.npad[l] : e.ct * (e.npad[0] + kLdPad));
    if (e.has_head) p.lds_hbias = p.take("hbias", -1, off, e.out_pad);
    if (e.has_head && with_yw) p.lds_yw = p.take("yw", -1, off, (e.ct * ((e.out_pad + 31) / 32) + 3) / 4 * 4);
    p.xl = true;
}

// LDS plan of the in-place wave-specialised kernel: every FX_l has its own rows (no staging slots).  With a read-out,
// the prediction errors E_1 .. E_{L-1} and the ring of read-out error chunks share ONE region: the ring is only live
// during the read-out phase at the start of a step, the E_l only from the forward entries (scheduled behind the
// read-out) to the x updates at its end.  16-chain workgroups usually have the room to keep the two apart (ws2_overlay == false),
// and at cfg-M a ring of THREE chunks of 14 tiles (49 tiles = 14 + 12 + 12 + 11, whole k-blocks of the back-projection; a table
// entry hands out up to 16 tiles, four per GEMM wave): two GEMMs of slack between a chunk's epilogue and its back-projection,
// 15 table entries per step.
inline int plan_lds_ws2(const EnginePlan& e, StepPlan& p) {
    p = StepPlan{};
    const int CT = e.ct, L = e.L;
    int off = 0;
    for (int l = 0; l < L; ++l) p.lds_a[l] = p.take("fx", l, off, CT * (e.npad[l] + kLdPad));
    p.lds_red = p.take("red", -1, off, 2 * (kMaxLatent + 1) * kMaxWaves);
    p.lds_ws_sync = p.take("ws_sync", -1, off, 16);
    // E_1 .. E_{L-1} stacked; the ring of read-out error chunks behind them when both fit (16-chain workgroups: the forward
    // entries are then free to run between the read-out chunks), else on top of them (shared region)
    int e_sum = 0;
    for (int l = 1; l < L; ++l) e_sum += CT * (e.npad[l] + kLdPad);
    int ring_floats = 0;
    if (e.has_head) {
        // fewest chunks of at most 16 tiles whose ring of two still fits; chunks equalised; ring of three if that fits too
        const int ht = std::max(e.out_pad / 16, 1);
        const int span = kWs2Pairs * kWs2NTW;     // tiles a table entry hands out
        auto ring_of = [&](int hc, int nb) { return nb * CT * (hc * 16 + kLdPad); };
        // (+ tail: what is added behind the operand regions below -- a plan that close to the limit takes a smaller chunk or ring here
        // instead of failing the final size check)
        constexpr int tail = 16 + kSpillTensors + kRowExpFloats;      // (zero region, spill maxima, row exponents: added below)
        auto fits = [&](int hc, int nb) { return (off + tail + std::max(ring_of(hc, nb), e_sum)) * (int)sizeof(float) <= kLdsLimit; };
        auto fits_apart = [&](int hc, int nb) { return (off + tail + ring_of(hc, nb) + e_sum) * (int)sizeof(float) <= kLdsLimit; };
        // (chunks are whole k-blocks of the back-projection GEMM: tq tiles)
        const int tq = kKB / 16, hb = (ht + tq - 1) / tq;
        int hcb_fit = 0;
        for (int hcb = std::min(span / tq, hb); hcb >= 1; --hcb)
            if (fits(hcb * tq, 2)) { hcb_fit = hcb; break; }
        if (!hcb_fit) return fail(MCPC_ENOMEM, "in-place schedule does not fit the LDS");
        const int nch = (hb + hcb_fit - 1) / hcb_fit;
        const int hc = tq * ((hb + nch - 1) / nch);          // equalised: the widest chunk of the split (tiles)
        const int nb = (nch >= 3 && fits(hc, 3)) ? 3 : 2;
        p.ws2_chunk = hc; p.ws2_ring = nb; ring_floats = ring_of(hc, nb);
        if (L >= 2 && fits_apart(hc, nb) && !e.knobs.overlay16) p.ws2_overlay = false;
    }
    int e_off = off;
    for (int l = 1; l < L; ++l) p.lds_e[l] = p.take("e", l, e_off, CT * (e.npad[l] + kLdPad));
    p.lds_eo = p.ws2_overlay ? off : e_off;
    if (ring_floats) p.regions.push_back({"ring", -1, p.lds_eo, ring_floats});
    off += p.ws2_overlay ? std::max(ring_floats, e_sum) : ring_floats + e_sum;
    // The GEMM core reads the LDS operand in whole 32-deep k-blocks; the lanes whose k values lie beyond a row whose width is not a
    // multiple of 32 read THESE 16 floats instead of what lies behind the row (mcpc_gemm_f16.h): zero-filled at launch, never written.
    p.lds_zero = p.take("zero", -1, off, 16);
    p.lds_spillmax = p.take("spillmax", -1, off, kSpillTensors);     // the workgroup's largest |value| per spilled tensor (mcpc_kernels.h: spill_track)
    p.lds_rowexp = p.take("rowexp", -1, off, kRowExpFloats);         // per B operand and chain row: generation and exponent of the row's maximum (rowexp_track)
    // with room to spare (16-chain plans: 45 KB at cfg-M) the lean epilogues keep what they read every step in LDS
    if (!e.knobs.no_xl) {
        StepPlan with = p;
        int end = off;
        take_xl(e, with, end, true);
        if (end * (int)sizeof(float) <= kLdsLimit) { p = with; off = end; }
    }
    p.lds_bytes = off * (int)sizeof(float);
    if (p.lds_bytes > kLdsLimit) return fail(MCPC_ENOMEM, "in-place schedule does not fit the LDS (%d bytes)", p.lds_bytes);
    return 0;
}

// Table of the in-place wave-specialised kernel (mcpc_steps_ws2.h), R = ring size.  One step =
//   read-out:  HF(0) .. HF(R-1) HB(0) HF(R) HB(1) ...   (FWD_0, which has no GEMM, slipped in behind the first HB);
//   forward:   FWD_{L-1} ... FWD_1   (their outputs E_l share LDS with the ring, so they follow the last HB);
//   updates:   BWD_{L-1} (accb hand-off), BWD_0 ... BWD_{L-2};  energy reduction.
// Read dependencies, waited for in front of the GEMM (dep_e, "all E waves past entry"):
//   HF(c) <- last BWD_{L-1} of the PREVIOUS step (FX_{L-1});  HB(c) <- HF(c);  FWD_l <- last BWD_{l-1} of the previous
//   step (FX_{l-1});  BWD_l GEMM <- last FWD_{l+1} (E_{l+1}).
// Write-after-read dependencies, waited for behind the GEMM, before the block is stored:
//   dep_g ("all G waves past entry"):  HF(c) <- HB(c-R) (ring slot);  HF(c) in a slot that overlaps the E_l <- last GEMM
//     of the previous step that reads an E_l (BWD_{L-2});  FWD_l <- HB(last);
//   dep_se ("all E waves past entry"): HF(c) in a slot that overlaps the E_l <- the last BWD entry of the previous step
//     (its epilogue loads read E_l).
// The others are implied: a G wave that stores into FX_l has just waited for epilogues that can only have run after every
// G wave finished the GEMMs that read the old contents (the BWD_{L-1} hand-off after HB(last) <- HF(last) epilogues, BWD_l
// after the FWD_{l+1} epilogues, which follow FWD_{l+1}'s GEMM over FX_l).
//
// 16-chain plans whose LDS holds the ring AND the E_l side by side (plan_lds_ws2: ws2_overlay == false) order a step differently:
//   read-out:  HF(0) .. HF(R-1) HB(0) FWD_1 HF(R) HB(1) FWD_0 HB(2) FWD_2 ...   (every forward entry fills a gap of the read-out)
//   updates:   as above.
// With 16 chains a GEMM is half as long, the epilogues are not, and the shared region cost twice: HF(0) / HF(1) waited for the LAST
// epilogue of the previous step (their slots overlapped the E_l it reads) and the forward GEMMs sat behind the read-out where
// nothing hid their epilogues.  Apart, HF(c < R) needs no write-after-read wait at all, and FWD_l waits -- behind its GEMM -- for
// the previous step's readers of E_l: dep_g <- last back-projection GEMM, dep_se <- last BWD entry.
inline void build_phases_ws2(const EnginePlan& e, StepPlan& p) {
    const int L = e.L;
    const int span = kWs2Pairs * kWs2NTW;     // tiles per table entry
    auto tiles = [&](int l) { return e.npad[l] / 16; };
    enum { REF_LAST_BWD = -1000, REF_LAST_FWD = -2000, REF_LAST_HB = -3000, REF_LAST_BWD_GEMM = -4000, REF_LAST_BWD_ANY = -5000 };   // symbolic deps
    auto fwd_entries = [&](int l, std::vector<KPhase>& out) {
        for (int base = 0; base < tiles(l); base += span) {
            KPhase k = blank_phase();
            k.type = PH_FWD; k.layer = l; k.tile0 = base; k.ntiles = std::min(span, tiles(l) - base);
            if (l == 0) {
                k.flags = PHF_MU1 | PHF_WS_EPI;
            } else {
                set_gemm(k, l, 16 * tiles(l - 1));
                k.b_lds = p.lds_a[l - 1]; k.ldb = e.npad[l - 1] + kLdPad;
                k.out_lds = p.lds_e[l]; k.out_ld = e.npad[l] + kLdPad;
                k.b_row = rowexp_fx(l - 1); k.o_row = rowexp_e(l);
                k.flags = PHF_WS_GEMM | PHF_WS_EPI; k.dep_e = REF_LAST_BWD - (l - 1);
                if (e.has_head && p.ws2_overlay) k.dep_g = REF_LAST_HB;       // E_l shares LDS with the ring
                else if (e.has_head) {
                    // E_l has rows of its own and the entry runs between the read-out chunks: what still reads the OLD E_l are
                    // the previous step's back-projection GEMMs (all G waves: E_l is a B operand) and x updates (E waves)
                    k.dep_g = REF_LAST_BWD_GEMM; k.dep_se = REF_LAST_BWD_ANY;
                }
            }
            out.push_back(k);
        }
    };
    // FWD_0 has no GEMM and no LDS output: it fills a gap of the read-out; the others follow the read-out
    std::vector<KPhase> fill, after;
    if (e.has_head && !p.ws2_overlay) {
        // every forward entry fills a gap of the read-out, in the order their inputs become ready: the previous step ends with
        // the x updates BWD_{L-1}, BWD_0, BWD_1 ... BWD_{L-2}, so FWD_1 (needs f(x_0)) first, FWD_0 (no GEMM), then FWD_2 ... FWD_{L-1}
        if (L >= 2) fwd_entries(1, fill);
        fwd_entries(0, fill);
        for (int l = 2; l < L; ++l) fwd_entries(l, fill);
    } else {
        for (int l = L - 1; l >= 0; --l) fwd_entries(l, (l >= 1 && e.has_head) ? after : fill);
    }
    std::vector<KPhase>& ph = p.table;
    size_t nf = 0;
    if (e.has_head) {
        const int hc = p.ws2_chunk, R = p.ws2_ring;        // hc: widest chunk = ring slot width
        const int ht = e.out_pad / 16;
        const int nch = (ht + hc - 1) / hc;
        // chunk c = tiles [c_start[c], c_start[c+1]): whole k-blocks of the back-projection (tq tiles each) dealt out evenly, the last
        // chunk clipped to the read-out's width
        const int tq = kKB / 16, hb = (ht + tq - 1) / tq;
        std::vector<int> c_start(nch + 1, 0);
        for (int c = 0; c < nch; ++c) c_start[c + 1] = std::min(ht, c_start[c] + tq * (hb / nch + (c < hb % nch ? 1 : 0)));
        const int chunk_floats = e.ct * (hc * 16 + kLdPad);
        int e_sum = 0;
        for (int l = 1; l < L; ++l) e_sum += e.ct * (e.npad[l] + kLdPad);
        std::vector<int> idx_f(nch, -1), idx_b(nch, -1);
        auto add_f = [&](int c) {
            KPhase f = blank_phase();
            f.type = PH_HEADF; f.layer = L - 1; f.tile0 = c_start[c]; f.ntiles = c_start[c + 1] - c_start[c]; f.rot = c & (kWs2Pairs - 1);
            set_gemm(f, L, 16 * tiles(L - 1));
            f.b_lds = p.lds_a[L - 1]; f.ldb = e.npad[L - 1] + kLdPad;
            f.out_lds = p.lds_eo + (c % R) * chunk_floats; f.out_ld = hc * 16 + kLdPad;
            f.b_row = rowexp_fx(L - 1); f.o_row = rowexp_ring(c % R);
            f.flags = PHF_WS_GEMM | PHF_WS_EPI; f.dep_e = REF_LAST_BWD - (L - 1);
            if (c >= R) f.dep_g = idx_b[c - R];
            else if (p.ws2_overlay && (c % R) * chunk_floats < e_sum) { f.dep_g = REF_LAST_BWD_GEMM; f.dep_se = REF_LAST_BWD_ANY; }   // slot overlaps the E_l
            idx_f[c] = (int)ph.size(); ph.push_back(f);
        };
        auto add_b = [&](int c) {
            KPhase b = blank_phase();
            b.type = PH_HEADB; b.layer = L - 1; b.tile0 = 0; b.ntiles = tiles(L - 1);
            b.a_lin = L; b.a_tile_stride = kblocks(e.out_pad) * kFragBlock; b.a_off0 = (c_start[c] / tq) * kFragBlock;
            b.kw = 16 * (c_start[c + 1] - c_start[c]); b.nkb = (c_start[c + 1] - c_start[c] + tq - 1) / tq;
            b.b_lds = p.lds_eo + (c % R) * chunk_floats; b.ldb = hc * 16 + kLdPad;
            b.b_row = rowexp_ring(c % R);
            b.flags = PHF_WS_GEMM; b.dep_e = idx_f[c];
            idx_b[c] = (int)ph.size(); ph.push_back(b);
            if (nf < fill.size()) ph.push_back(fill[nf++]);      // one forward entry behind every back-projection
        };
        for (int c = 0; c < nch; ++c) {
            add_f(c);
            if (c >= R - 1) add_b(c - (R - 1));
        }
        for (int c = std::max(nch - (R - 1), 0); c < nch; ++c) add_b(c);
    }
    while (nf < fill.size()) ph.push_back(fill[nf++]);
    // bottom-up (FWD_1 first): the small GEMMs go first, so that the epilogue of FWD_1 has FWD_2's GEMM to hide behind
    for (auto it = after.rbegin(); it != after.rend(); ++it) ph.push_back(*it);
    // x updates: BWD_{L-1} first (its back-projection is complete: accb), then bottom-up from BWD_0, so that BWD_{L-2},
    // which reads the E_{L-1} produced last, comes last
    for (int base = 0; base < tiles(L - 1); base += span) {
        KPhase k = blank_phase();
        k.type = PH_BWD; k.layer = L - 1; k.tile0 = base; k.ntiles = std::min(span, tiles(L - 1) - base);
        k.flags = PHF_WS_EPI | (e.has_head ? PHF_WS2_HANDOFF : 0);
        k.sign = e.has_head ? 1.0f : 0.0f;
        k.out_lds = p.lds_a[L - 1]; k.out_ld = e.npad[L - 1] + kLdPad;
        k.o_row = rowexp_fx(L - 1);
        ph.push_back(k);
    }
    for (int l = 1; l <= L - 1; ++l)
        for (int base = 0; base < tiles(l - 1); base += span) {
            KPhase k = blank_phase();
            k.type = PH_BWD; k.layer = l - 1; k.tile0 = base; k.ntiles = std::min(span, tiles(l - 1) - base);
            set_gemm(k, l, 16 * tiles(l));
            k.b_lds = p.lds_e[l]; k.ldb = e.npad[l] + kLdPad; k.sign = -1.0f;
            k.out_lds = p.lds_a[l - 1]; k.out_ld = e.npad[l - 1] + kLdPad;
            k.b_row = rowexp_e(l); k.o_row = rowexp_fx(l - 1);
            k.flags = PHF_WS_GEMM | PHF_WS_EPI; k.dep_e = REF_LAST_FWD - l;
            ph.push_back(k);
        }
    { KPhase k = blank_phase(); k.type = PH_ENERGY; k.flags = PHF_WS_EPI; ph.push_back(k); }
    // resolve the symbolic dependencies
    std::vector<int> last_fwd(L, -1), last_bwd(L, -1);
    int last_hb = -1, last_bwd_gemm = -1, last_bwd_any = -1;
    for (size_t i = 0; i < ph.size(); ++i) {
        if (ph[i].type == PH_FWD) last_fwd[ph[i].layer] = (int)i;
        if (ph[i].type == PH_BWD) { last_bwd[ph[i].layer] = (int)i; last_bwd_any = (int)i; if (ph[i].flags & PHF_WS_GEMM) last_bwd_gemm = (int)i; }
        if (ph[i].type == PH_HEADB) last_hb = (int)i;
    }
    auto resolve = [&](int d) {
        if (d == REF_LAST_BWD_ANY) return last_bwd_any;
        if (d == REF_LAST_BWD_GEMM) return last_bwd_gemm;
        if (d == REF_LAST_HB) return last_hb;
        if (d <= REF_LAST_FWD && d > REF_LAST_HB) return last_fwd[REF_LAST_FWD - d];
        if (d <= REF_LAST_BWD && d > REF_LAST_FWD) return last_bwd[REF_LAST_BWD - d];
        return d;
    };
    for (auto& k : ph) { k.dep_e = resolve(k.dep_e); k.dep_g = resolve(k.dep_g); k.dep_se = resolve(k.dep_se); }
    // the GEMM waves walk only the entries they have work in (a GEMM, or the hand-off of the read-out's back-projection): FWD_0, the
    // energy entry and x updates without a back-projection cost them a table round each for nothing
    auto g_works = [&](const KPhase& k) { return (k.flags & (PHF_WS_GEMM | PHF_WS2_HANDOFF)) != 0; };
    p.g_first = -1;
    for (size_t i = 0; i < ph.size(); ++i) if (g_works(ph[i])) { p.g_first = (int)i; break; }
    for (size_t i = 0; i < ph.size(); ++i) {
        ph[i].next_g = p.g_first;
        for (size_t d = 1; d <= ph.size(); ++d) {
            const size_t j = (i + d) % ph.size();
            if (g_works(ph[j])) { ph[i].next_g = (int)j; break; }
        }
    }
    p.n_phases = (int)ph.size();
}

// ---- unified-wave kernel (mcpc_steps_u.h) ---------------------------------------------------------------------------------------------
// LDS plan: FX_l, E_l, the WHOLE read-out error e_o [16][out_pad], the state rows X_l and the per-step constants of the workgroup's 16
// chains.  No plan (u.ok == false, not an error) when that does not fit 160 KiB: such networks run on the in-place kernel.
inline void plan_lds_u(const EnginePlan& e, UPlan& u) {
    u.ok = false;
    const int CT = e.ct, L = e.L;
    // two tries: everything the epilogues read per step in LDS; else the bit-packed target rows stay in global memory (the read-out's
    // epilogue requests its words in front of its row's GEMM: mcpc_steps_u.h) -- cfg-M's plan is 1 792 bytes over the 160 KiB with them
    // and fits with 64 bytes to spare without
    for (int yw_in_lds = 1; yw_in_lds >= 0 && !u.ok; --yw_in_lds) {
        StepPlan& p = u.plan = StepPlan{};
        int off = 0;
        for (int l = 0; l < L; ++l) p.lds_a[l] = p.take("fx", l, off, CT * (e.npad[l] + kLdPad));
        for (int l = 1; l < L; ++l) p.lds_e[l] = p.take("e", l, off, CT * (e.npad[l] + kLdPad));
        p.lds_red = p.take("red", -1, off, 2 * (kMaxLatent + 1) * kMaxWaves);
        p.lds_ws_sync = off;                                // (no progress counters in this kernel)
        p.lds_eo = p.take("eo", -1, off, e.has_head ? CT * (e.out_pad + kLdPad) : 0);
        p.head_ld = e.out_pad + kLdPad;
        p.lds_zero = p.take("zero", -1, off, 16);
        p.lds_spillmax = p.take("spillmax", -1, off, kSpillTensors);
        p.lds_rowexp = p.take("rowexp", -1, off, (rowexp_ring(0) + 1) * 16);      // the ids this kernel uses: FX_l, E_l and ONE read-out row word
        p.lds_yw = -1;
        take_xl(e, p, off, yw_in_lds != 0);
        p.g_first = 0;
        p.lds_bytes = off * (int)sizeof(float);
        u.ok = p.lds_bytes <= kLdsLimit;
    }
}

// Tables of the unified-wave kernel: every wave walks its OWN rows (table[w * n_phases + p]).  One step = two levels, each opened by a
// workgroup barrier:
//   forward:  read-out tiles (HEADF: out, loss error -> e_o), FWD_{L-1} .. FWD_1 (prediction errors E_l), FWD_0 -- they read the FX_l the
//             previous step's x updates left and write e_o / E_l;
//   updates:  BWD_{L-1} (GEMM over the whole e_o), BWD_{L-2} .. BWD_0 (GEMM over E_{l+1}) -- they read e_o / E_l and write X_l, FX_l.
// Inside a level the jobs are independent, and with a barrier on either side no tile belongs to a wave: a JOB is up to four consecutive
// unit tiles of one entry (one GEMM call + one epilogue call of a wave), and the jobs of a level are dealt to the eight waves by cost,
// longest first (a cost model in cycles: fixed cost per row, k-blocks x (operand split + MFMAs per tile), epilogue per tile).  Why four
// tiles where the work allows: the operand split (24 VALU instructions per k-block) and the row's fixed costs are shared by the job's
// tiles -- a GEMM of 8 tiles as 2 jobs of 4 splits its B operand twice, as 8 jobs of 1 eight times -- and heavy entries (the read-out's
// back-projection: K = n_out) are cut finer only as far as the level's balance needs.  (The one exception: the running sum of e_1 lives in
// registers of wave w for tile w of the top layer -- lean_load_e0 -- so FWD_0's tiles are pinned when that layer has at most 8.)
inline void build_phases_u(const EnginePlan& e, StepPlan& u) {
    const int L = e.L;
    auto tiles = [&](int l) { return e.npad[l] / 16; };
    auto blank = [&]() { KPhase k = blank_phase(); k.next_g = -1; k.rot = 1; return k; };
    struct Job { KPhase k; double cost; int pin; };
    // cost model (shader cycles per wave; calibrated on profiles/r06_small_net.txt).  Per k-block of a row's GEMM: 1 tile ~400, 2 tiles ~470,
    // 4 tiles ~600 -- the B split, the fragment requests and, with one tile, three dependent MFMAs -- and ~200 less when the operand arrives
    // in planes (`ps`: the read-out's back-projection; the table is built before the loss is known and assumes the Bernoulli read-out the
    // reference trains with); ~1200 before the first block; per row ~2000 for its descriptor, the next row's fragment requests and the
    // epilogue's fixed part; per tile of an epilogue: read-out ~1000, x update with the Philox kick ~1300, prediction error ~500.
    const Knobs& kn = e.knobs;
    auto gemm_cost = [&](int nt, int nkb, bool ps) { return nkb > 0 ? (double)kn.u_gemm0 + nkb * ((double)std::max(kn.u_kb - (ps ? 200 : 0), 0) + (double)kn.u_kbt * nt) : 0.0; };
    const double row_cost = (double)kn.u_row;
    auto make_jobs = [&](const KPhase& proto, int nt_total, double epi_tile, int g, std::vector<Job>& out, bool pinned, bool ps) {
        if (pinned) g = 1;
        for (int t = 0; t < nt_total; t += g) {
            Job j; j.k = proto; j.k.tile0 = t; j.k.ntiles = std::min(g, nt_total - t); j.k.rot = 1;
            if (proto.type == PH_HEADF) j.k.out_lds = proto.out_lds + 16 * t;       // (the epilogue writes columns relative to its row's first tile)
            j.cost = row_cost + gemm_cost(j.k.ntiles, (proto.flags & PHF_WS_GEMM) ? proto.nkb : 0, ps) + j.k.ntiles * epi_tile;
            j.pin = pinned ? t : -1;
            out.push_back(j);
        }
    };
    struct Entry { KPhase k; int ntiles; double epi_tile; bool pinned; bool ps; };
    std::vector<Entry> level[2];
    if (e.has_head) {
        KPhase f = blank();
        f.type = PH_HEADF; f.layer = L - 1;
        set_gemm(f, L, 16 * tiles(L - 1));
        f.b_lds = u.lds_a[L - 1]; f.ldb = e.npad[L - 1] + kLdPad;
        f.out_lds = u.lds_eo; f.out_ld = e.out_pad + kLdPad;            // (row-relative columns: the epilogue adds 16 (tile - tile0) to its row's base)
        f.b_row = rowexp_fx(L - 1); f.o_row = rowexp_ring(0);
        f.flags = PHF_WS_GEMM | PHF_WS_EPI;
        level[0].push_back({f, e.out_pad / 16, (double)kn.u_eh, false, false});
    }
    for (int l = L - 1; l >= 0; --l) {
        KPhase k = blank();
        k.type = PH_FWD; k.layer = l;
        if (l == 0) {
            k.flags = PHF_MU1 | PHF_WS_EPI;
        } else {
            set_gemm(k, l, 16 * tiles(l - 1));
            k.b_lds = u.lds_a[l - 1]; k.ldb = e.npad[l - 1] + kLdPad;
            k.out_lds = u.lds_e[l]; k.out_ld = e.npad[l] + kLdPad;
            k.b_row = rowexp_fx(l - 1); k.o_row = rowexp_e(l);
            k.flags = PHF_WS_GEMM | PHF_WS_EPI;
        }
        level[0].push_back({k, tiles(l), (double)kn.u_ef, l == 0 && tiles(0) <= kUWaves, false});
    }
    for (int l = L - 1; l >= 0; --l) {
        KPhase k = blank();
        k.type = PH_BWD; k.layer = l;
        k.out_lds = u.lds_a[l]; k.out_ld = e.npad[l] + kLdPad; k.o_row = rowexp_fx(l);
        k.flags = PHF_WS_EPI;
        if (l == L - 1) {
            k.sign = e.has_head ? 1.0f : 0.0f;
            if (e.has_head) {
                set_gemm(k, L, e.out_pad);
                k.b_lds = u.lds_eo; k.ldb = e.out_pad + kLdPad; k.b_row = rowexp_ring(0);
                k.flags |= PHF_WS_GEMM;
            }
        } else {
            set_gemm(k, l + 1, 16 * tiles(l + 1));
            k.b_lds = u.lds_e[l + 1]; k.ldb = e.npad[l + 1] + kLdPad; k.b_row = rowexp_e(l + 1); k.sign = -1.0f;
            k.flags |= PHF_WS_GEMM;
        }
        level[1].push_back({k, tiles(l), (double)kn.u_eb, false, l == L - 1 && e.has_head && e.out_pad > kShortK * kKB});
    }
    std::vector<KPhase> rows[kUWaves];
    for (int lv = 0; lv < 2; ++lv) {
        // the grain of every entry (4, 2 or 1 tiles per job) by exhaustive search: the combination whose longest-first deal has the
        // shortest makespan (at most 7 entries per level: 3^7 deals of a few dozen jobs)
        const int ne = (int)level[lv].size();
        std::vector<int> grain(ne, 4), best_grain(ne, 4);
        double best_span = 1e300;
        std::vector<Job> jobs;
        auto deal = [&](const std::vector<int>& gr, std::vector<KPhase>* mine) {
            jobs.clear();
            for (int i = 0; i < ne; ++i) make_jobs(level[lv][i].k, level[lv][i].ntiles, level[lv][i].epi_tile, gr[i], jobs, level[lv][i].pinned, level[lv][i].ps);
            std::stable_sort(jobs.begin(), jobs.end(), [](const Job& a, const Job& b) { return (a.pin >= 0) != (b.pin >= 0) ? a.pin >= 0 : a.cost > b.cost; });
            double load[kUWaves] = {0};
            for (auto& j : jobs) {
                int w = 0;
                if (j.pin >= 0) w = j.pin;
                else for (int i = 1; i < kUWaves; ++i) if (load[i] < load[w]) w = i;
                load[w] += j.cost;
                if (mine) mine[w].push_back(j.k);
            }
            double span = 0, sum = 0;
            for (double v : load) { span = std::max(span, v); sum += v; }
            return span + 1e-3 * sum;               // (ties: the deal with less work in total)
        };
        int combos = 1;
        for (int i = 0; i < ne; ++i) combos *= 3;
        for (int cidx = 0; cidx < combos; ++cidx) {
            int c = cidx;
            for (int i = 0; i < ne; ++i) { grain[i] = 4 >> (c % 3); c /= 3; }
            const double span = deal(grain, nullptr);
            if (span < best_span) { best_span = span; best_grain = grain; }
        }
        std::vector<KPhase> mine[kUWaves];
        (void)deal(best_grain, mine);
        for (int w = 0; w < kUWaves; ++w) {
            if (mine[w].empty()) { KPhase k = blank(); k.type = PH_NOP; mine[w].push_back(k); }
            mine[w][0].flags |= PHF_SYNC;                        // the level's barrier
            rows[w].insert(rows[w].end(), mine[w].begin(), mine[w].end());
        }
    }
    // the four fragment slots a row's GEMM starts from (u_prefetch), resolved here: offsets in 16-byte units from the row's A, -1 = none.
    // (dep_e, dep_g, dep_se, next_g carry them: the unified-wave kernel has no other use for those fields)
    for (int w = 0; w < kUWaves; ++w)
        for (auto& k : rows[w]) {
            int slot[4] = {-1, -1, -1, -1};
            const int nt = std::min(k.ntiles, kUNT);
            if (nt > 0 && (k.flags & PHF_WS_GEMM) && k.nkb > 0)
                for (int sl = 0; sl < 4; ++sl) {
                    const bool deep = nt <= 2;
                    const int ti = deep ? (nt == 2 ? (sl & 1) : 0) : sl, kb = deep ? (nt == 2 ? (sl >> 1) : sl) : 0;
                    if (ti < nt && kb < k.nkb) slot[sl] = (k.tile0 + k.rot * ti) * k.a_tile_stride + k.a_off0 + kb * kFragBlock;
                }
            k.dep_e = slot[0]; k.dep_g = slot[1]; k.dep_se = slot[2]; k.next_g = slot[3];
        }
    size_t R = 0;
    for (int w = 0; w < kUWaves; ++w) R = std::max(R, rows[w].size());
    for (int w = 0; w < kUWaves; ++w) {
        while (rows[w].size() < R) { KPhase k = blank(); k.type = PH_NOP; rows[w].push_back(k); }
        u.table.insert(u.table.end(), rows[w].begin(), rows[w].end());
    }
    u.n_phases = (int)R;
}

// The automatic choice between the in-place and the unified-wave kernel for an engine whose unified plan fits (tuning ws=2 / ws=3 force
// either).  Measured on one MI355X (profiles/r06_small_net.txt, us per 16-chain unit-step, MCPC / MAP / learning call):
//   20-128-128-784 (476 tile-blocks of GEMM per step)   in-place 21.3 / 23.1 / 23.9    unified 16.8 / 18.0 / 19.3
//   30-200-200-784 (877)                                  in-place 25.3                  unified 23.2            (MCPC)
//   30-224-224-784 (917)                                  in-place 25.5                  unified 26.8
//   30-256-256-784 (1 080 tile-blocks: cfg-M)            in-place 26.4 / 30.0 / 29.4    unified 27.9-29.3 / 31.0 / 32.4
// A step's fixed costs per table entry are what the unified form removes; the overlap of GEMM and epilogue waves is what it gives up, and
// at cfg-M's width that overlap is worth more.  The unit is what both scale with: (unit tile, 32-deep k-block) pairs of all GEMMs of a step.
// A ZERO-LOSS call (unclamped generation) runs on the unified kernel whatever the width: only that kernel skips the read-out on the steps
// nobody records (cfg-M's net: 16.6 against 25.3 us per step) -- use_unified decides that per run.
inline int gemm_tile_blocks(const EnginePlan& e) {
    int n = 0;
    for (int l = 1; l < e.L; ++l) n += (e.npad[l] / 16) * kblocks(e.npad[l - 1]) + (e.npad[l - 1] / 16) * kblocks(e.npad[l]);
    if (e.has_head) n += (e.out_pad / 16) * kblocks(e.npad[e.L - 1]) + (e.npad[e.L - 1] / 16) * kblocks(e.out_pad);
    return n;
}
inline bool choose_unified(const EnginePlan& e) { return gemm_tile_blocks(e) <= 900; }

// Table of the barrier kernel: every GEMM of a Langevin step with its operands, the epilogue that follows
// it and the barrier it needs.  Output tiles are handed out 16 at a time (4 waves x kNT tiles).
inline void build_phases(const EnginePlan& e, StepPlan& p) {
    std::vector<KPhase>& ph = p.table;
    const int L = e.L;
    const int span = kNT * kWaves;
    auto tiles = [&](int l) { return e.npad[l] / 16; };
    // top latent layer: its prediction is the constant mu1, no GEMM
    for (int base = 0; base < tiles(0); base += span) {
        KPhase k{};
        k.type = PH_FWD; k.layer = 0; k.tile0 = base; k.ntiles = std::min(span, tiles(0) - base);
        k.flags = PHF_MU1 | (base + span >= tiles(0) ? PHF_SYNC : 0);
        ph.push_back(k);
    }
    for (int l = 1; l < L; ++l)
        for (int base = 0; base < tiles(l); base += span) {
            KPhase k{};
            k.type = PH_FWD; k.layer = l; k.tile0 = base; k.ntiles = std::min(span, tiles(l) - base);
            set_gemm(k, l, 16 * tiles(l - 1));
            k.b_lds = p.lds_a[l - 1]; k.ldb = e.npad[l - 1] + kLdPad;
            k.flags = base + span >= tiles(l) ? PHF_SYNC : 0;
            ph.push_back(k);
        }
    if (e.has_head) {
        const int ht = e.out_pad / 16;
        for (int c0 = 0; c0 < ht; c0 += kChunkTiles) {
            const int ntc = std::min(kChunkTiles, ht - c0);
            KPhase f{};
            f.type = PH_HEADF; f.layer = L - 1; f.tile0 = c0; f.ntiles = ntc;
            set_gemm(f, L, 16 * tiles(L - 1));
            f.b_lds = p.lds_a[L - 1]; f.ldb = e.npad[L - 1] + kLdPad; f.flags = PHF_SYNC;
            f.out_lds = p.lds_eo; f.out_ld = kChunkTiles * 16 + kLdPad; f.dep_e = f.dep_g = -1;
            ph.push_back(f);
            KPhase b{};
            b.type = PH_HEADB; b.layer = L - 1; b.tile0 = 0; b.ntiles = tiles(L - 1);
            b.a_lin = L; b.a_tile_stride = kblocks(e.out_pad) * kFragBlock; b.a_off0 = (c0 * 16 / kKB) * kFragBlock;
            b.kw = ntc * 16; b.nkb = (ntc * 16 + kKB - 1) / kKB;
            b.b_lds = p.lds_eo; b.ldb = kChunkTiles * 16 + kLdPad;
            b.flags = PHF_ACC_FROM_B | PHF_ACC_TO_B | PHF_SYNC;
            ph.push_back(b);
        }
    }
    { KPhase k{}; k.type = PH_ENERGY; ph.push_back(k); }
    // x updates, bottom-up: the last latent layer first (its back-projection sits in accb)
    for (int base = 0; base < tiles(L - 1); base += span) {
        KPhase k{};
        k.type = PH_BWD; k.layer = L - 1; k.tile0 = base; k.ntiles = std::min(span, tiles(L - 1) - base);
        k.flags = e.has_head ? PHF_ACC_FROM_B : 0;
        k.sign = e.has_head ? 1.0f : 0.0f;
        ph.push_back(k);
    }
    for (int l = L - 1; l >= 1; --l)
        for (int base = 0; base < tiles(l - 1); base += span) {
            KPhase k{};
            k.type = PH_BWD; k.layer = l - 1; k.tile0 = base; k.ntiles = std::min(span, tiles(l - 1) - base);
            set_gemm(k, l, 16 * tiles(l));
            k.b_lds = p.lds_e[l]; k.ldb = e.npad[l] + kLdPad; k.sign = -1.0f;
            ph.push_back(k);
        }
    p.n_phases = (int)ph.size();
}

// ---- layer-wise kernels (mcpc_steps_lw.h) ---------------------------------------------------------------------------------------------------
// The unit-tile jobs of the two launches of a step: gridDim.y of the forward launch walks (Linear j, first unit tile) for every Linear --
// the read-out is j = L, Linear 0 (no GEMM) included -- in tiles of kLwUnitTiles x 16 units, gridDim.y of the backward launch (latent
// layer l, first unit tile); gridDim.x is the chain tile.  Every 16-unit tile of every layer is in exactly one job (tests/test_wide_cases.py
// checks that through mcpc_debug_lw_jobs).
inline void lw_job_table(int L, const int* npad, int out_pad, std::vector<LwJob>& fwd, std::vector<LwJob>& bwd) {
    fwd.clear(); bwd.clear();
    // widest first: the long GEMMs of a launch start first, the short tiles fill its tail
    auto tiles_of = [&](int j) { return (j < L ? npad[j] : out_pad) / 16; };
    auto cost_of = [&](int j) { return j == 0 ? 0 : npad[j - 1]; };
    std::vector<int> order;
    for (int j = 0; j <= L; ++j) if (tiles_of(j) > 0) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost_of(a) > cost_of(b); });
    for (int j : order)
        for (int ut = 0; ut < tiles_of(j); ut += kLwUnitTiles) fwd.push_back(LwJob{j, ut});
    auto bcost = [&](int l) { return l + 1 < L ? npad[l + 1] : out_pad; };
    std::vector<int> border;
    for (int l = 0; l < L; ++l) border.push_back(l);
    std::stable_sort(border.begin(), border.end(), [&](int a, int b) { return bcost(a) > bcost(b); });
    for (int l : border)
        for (int ut = 0; ut < npad[l] / 16; ut += kLwUnitTiles) bwd.push_back(LwJob{l, ut});
}

// The evaluators' job table (mcpc_chain_energy.h; built by mcpc_eval.hip): every (Linear, block of kLwUnitTiles unit tiles) once.  The read-out's jobs come
// first -- a call without a loss launches the table from `n_head` on -- then the latent layers, longest contraction first (the long GEMMs of the launch start first);
// the jobs of one Linear are contiguous with ascending first tile: the order mcpc_ce_finish_kernel adds them in.
inline void ce_job_table(int L, const int* npad, int out_pad, std::vector<LwJob>& jobs, int& n_head, CeFinish& F) {
    jobs.clear();
    for (int j = 0; j <= kMaxLatent; ++j) F.first[j] = F.count[j] = 0;
    auto emit = [&](int j, int tiles) {
        F.first[j] = (int)jobs.size();
        for (int ut = 0; ut < tiles; ut += kLwUnitTiles) jobs.push_back(LwJob{j, ut});
        F.count[j] = (int)jobs.size() - F.first[j];
    };
    if (out_pad > 0) emit(L, out_pad / 16);
    n_head = (int)jobs.size();
    std::vector<int> order;
    for (int j = 0; j < L; ++j) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return (a == 0 ? 0 : npad[a - 1]) > (b == 0 ? 0 : npad[b - 1]); });
    for (int j : order) emit(j, npad[j] / 16);
}

// Round schedule of the in-place kernel for a shard of U 16-chain units on C < U CUs.  One unit per CU is what the kernel is built
// for (a step is a chain of dependent hand-overs inside ONE workgroup: a second workgroup per CU does not fit the LDS, a launch of
// U > C workgroups runs as ceil(U / C) hardware rounds, the last one mostly empty).  Instead the units are dealt into k groups and a
// CYCLE is k launches of q steps; launch i runs groups i .. i+m-1 (mod k): every unit takes part in m of the k launches, in
// order, and after the cycle every unit has advanced m q steps -- k / m launch times per m q steps where the hardware rounds need
// ceil(U / C).  6000 chains = 375 units on 256 CUs: k = 3, m = 2, 250 workgroups per launch, 1.5 launch times per step instead of 2.
// (k, m): the smallest k within 3 % of the smallest k / m over k <= 16 whose launches fit C workgroups.  Chains are independent, so the trajectories are those
// of any other schedule, bitwise; in a Hebbian segment (m q <= slots of a ring part) every unit fills its own rows of all m q slots
// before the flush, which therefore sees what the plain schedule would have written.  (tests/test_round_plan.py)
inline int plan_rounds(EnginePlan& e, int n_cu) {
    const int U = e.nwg_live, C = n_cu - e.knobs.cu_slack;
    if (U <= C || C < 1) return 0;
    auto gsize = [&](int k, int g) { return (int)((int64_t)(g + 1) * U / k - (int64_t)g * U / k); };
    // best m for every k <= 16, then the SMALLEST k within 3 % of the best k / m: short cycles mean long launches (a Hebbian segment is
    // one cycle of at most `half_slots` steps) -- 300 units: (6, 5) at 1.200 rather than (13, 11) at 1.182
    int bk = 0, bm = 0, mk[17] = {0};
    for (int k = 2; k <= 16; ++k)
        for (int m = k - 1; m >= 1; --m) {
            int worst = 0;
            for (int i = 0; i < k; ++i) { int s = 0; for (int j = 0; j < m; ++j) s += gsize(k, (i + j) % k); worst = std::max(worst, s); }
            if (worst > C) continue;
            mk[k] = m;
            if (!bk || (int64_t)k * bm < (int64_t)bk * m) { bk = k; bm = m; }
            break;
        }
    for (int k = 2; bk && k < bk; ++k)
        if (mk[k] && 100.0 * k * bm <= 103.0 * bk * mk[k]) { bk = k; bm = mk[k]; break; }
    if (!bk) { bk = (U + C - 1) / C; bm = 1; }            // more than 16 rounds: plain rounds of at most C units
    const int k = bk, m = bm;
    std::vector<int>& tab = e.rr_host;
    e.rr_count.assign(k, 0); e.rr_off.assign(k, 0);
    std::vector<int> done(k, 0);                              // launches of this cycle a group has taken part in
    for (int i = 0; i < k; ++i) {
        std::vector<int> ids, rel;
        for (int j = 0; j < m; ++j) {
            const int g = (i + j) % k;
            for (int u = (int)((int64_t)g * U / k); u < (int)((int64_t)(g + 1) * U / k); ++u) { ids.push_back(u); rel.push_back(done[g]); }
        }
        for (int j = 0; j < m; ++j) ++done[(i + j) % k];
        e.rr_off[i] = (int)tab.size(); e.rr_count[i] = (int)ids.size();
        tab.insert(tab.end(), ids.begin(), ids.end());
        tab.insert(tab.end(), rel.begin(), rel.end());
    }
    for (int g = 0; g < k; ++g)
        if (done[g] != m) return fail(MCPC_EINVAL, "round schedule: unbalanced cycle");
    e.rr_k = k; e.rr_m = m; e.rr = true;
    const std::string cycle = " (round schedule: k=" + std::to_string(k) + " launches per cycle, every 16-chain unit in m=" + std::to_string(m) + " of them)";
    e.u_rr_name = "mcpc::mcpc_steps_u_kernel<true>" + cycle;
    e.rr_name = "mcpc::mcpc_steps_ws2_kernel<1, true>" + cycle;
    return 0;
}

// Names of the step kernel as a trace shows them: of one plain launch, and of the engine (mcpc_step_kernel_name) -- an engine that
// prefers the unified-wave kernel runs its fused calls, what a benchmark times, on that kernel
inline const char* plain_kernel_name(const EnginePlan& e, bool unified) {
    return e.lw ? kLwName : unified ? "mcpc::mcpc_steps_u_kernel<false>" : e.ws == 2 ? "mcpc::mcpc_steps_ws2_kernel<1, false>" : "mcpc::mcpc_steps_kernel<1, 4>";
}
inline const char* step_kernel_name(const EnginePlan& e) {
    return !e.rr || e.lw ? plain_kernel_name(e, e.u.prefer) : e.u.prefer ? e.u_rr_name.c_str() : e.rr_name.c_str();
}

inline int check_net_desc(const mcpc_net_desc* d) {
    if (d->abi_version != MCPC_ABI_VERSION) return fail(MCPC_EINVAL, "ABI version mismatch: header %d, library %d", d->abi_version, MCPC_ABI_VERSION);
    if (d->n_latent < 1 || d->n_latent > kMaxLatent) return fail(MCPC_EINVAL, "n_latent=%d out of range 1..%d", d->n_latent, kMaxLatent);
    if (d->batch < 1 || d->n_in < 1 || d->n_out < 0) return fail(MCPC_EINVAL, "bad batch/n_in/n_out (%d/%d/%d)", d->batch, d->n_in, d->n_out);
    for (int l = 0; l < d->n_latent; ++l) {
        if (d->sizes[l] < 1) return fail(MCPC_EINVAL, "sizes[%d]=%d", l, d->sizes[l]);
        if (d->acts[l] < 0 || d->acts[l] > 2) return fail(MCPC_EINVAL, "acts[%d]=%d", l, d->acts[l]);
        if (!(d->ecoef[l] > 0.f)) return fail(MCPC_EINVAL, "ecoef[%d] must be positive", l);
    }
    return 0;
}

// Everything mcpc_create decides, from a checked descriptor, the parsed knobs (e.knobs), the device's CU count and its total memory
// (read only when the descriptor gives no spill budget; 0: unknown).
// Default schedule: the in-place wave-specialised kernel (4 GEMM + 4 epilogue waves, 16 chains, one workgroup per CU; shards of
// more units than CUs on the round schedule, plan_rounds).  The barrier kernel (16 chains, 4 waves, generic epilogues) is the
// fallback when the in-place LDS plan does not fit, and the independent form the parity checks replay the default against
// (bench.py self_check, tests): tuning ws=0 forces it, ws=2 insists on the in-place kernel.
inline void plan_slabs(EnginePlan& e);       // (behind plan_hebbian, below)
inline int plan_engine(const mcpc_net_desc& d, int n_cu, size_t total_mem, EnginePlan& e) {
    const Knobs& kn = e.knobs;
    e.L = d.n_latent;
    e.has_head = d.n_out > 0;
    e.Bpad = (d.batch + kBatchPad - 1) / kBatchPad * kBatchPad;
    e.ws = kn.ws == 0 ? 0 : 2;
    e.nw = e.ws == 2 ? 2 * kWs2Pairs : kWaves;
    for (int l = 0; l < e.L; ++l) e.npad[l] = pad16(d.sizes[l]);
    e.out_pad = pad16(d.n_out);
    // The back-projection of the read-out error is accumulated in registers over the whole read-out: 16 tiles per workgroup
    // (a last latent layer of up to 256 units) in both kernels (cap_ws2 = 4 GEMM waves x 4 tiles, cap_bar = 4 waves x 4 tiles).
    const int last_tiles = e.has_head ? e.npad[e.L - 1] / 16 : 0;
    const int cap_ws2 = kWs2Pairs * kWs2NTW, cap_bar = kNT * kWaves;
    // The layer-wise kernels (mcpc_steps_lw.h) know neither limit: tuning ws=4 takes them for every run, wide=1 where the checks below fail
    e.lw = kn.ws == 4;
    if (!e.lw && (last_tiles > std::max(cap_ws2, cap_bar) || (last_tiles > cap_bar && e.ws != 2))) {
        if (!kn.wide)
            return fail(MCPC_ENOMEM, "last latent layer wider than %d units is not supported by the fused read-out (its back-projection is held in register tiles)", (e.ws == 2 ? std::max(cap_ws2, cap_bar) : cap_bar) * 16);
        e.lw = true;
    }
    if (!e.lw) {
        int rc = e.ws == 2 ? plan_lds_ws2(e, e.main) : plan_lds(e, e.main);
        if (rc && e.ws == 2 && kn.ws == -1 && last_tiles <= cap_bar) {   // no in-place plan fits: the barrier schedule
            g_err.clear();
            e.ws = 0; e.nw = kWaves;
            rc = plan_lds(e, e.main);
        }
        if (rc == MCPC_ENOMEM && kn.wide) { g_err.clear(); rc = 0; e.lw = true; }
        if (rc) return rc;
    }
    // the unified-wave kernel beside the in-place kernel, where its plan fits (mcpc_steps_u.h)
    if (!e.lw && e.ws == 2 && (kn.ws == -1 || kn.ws == 3) && !kn.no_lean && !kn.no_xl) {
        plan_lds_u(e, e.u);
        e.u.on = e.u.ok;
        e.u.prefer = e.u.ok && (kn.ws == 3 || choose_unified(e));
    }
    // (a forced unified-wave kernel whose plan does not fit: the layer-wise kernels under wide=1, MCPC_ENOMEM without it)
    if (!e.lw && kn.ws == 3 && !e.u.on) {
        if (!(kn.wide && e.ws == 2)) return fail(MCPC_ENOMEM, "tuning ws=3: the unified-wave kernel's LDS plan does not fit this network (%d bytes)", e.u.plan.lds_bytes);
        e.lw = true;
    }
    e.nwg = e.Bpad / e.ct;
    if (e.lw) {
        // no LDS plan, no step table: whole chain tiles of the layer-wise kernels, their static LDS
        e.ws = 0; e.nw = kLwWaves; e.u = UPlan{}; e.main = StepPlan{};
        e.Bpad = (d.batch + kLwChains - 1) / kLwChains * kLwChains;
        e.nwg = e.Bpad / e.ct;
        e.main.lds_bytes = kLwLdsBytes;
    }
    e.nwg_live = e.ws == 2 ? (d.batch + 15) / 16 : e.nwg;
    // Linear shapes
    const int nlin = e.L + (e.has_head ? 1 : 0);
    for (int j = 0; j < nlin; ++j) {
        Lin& ln = e.lin[j];
        ln.n_in = j == 0 ? d.n_in : d.sizes[j - 1];
        ln.n_out = j < e.L ? d.sizes[j] : d.n_out;
        ln.in_pad = j == 0 ? d.n_in : e.npad[j - 1];
        ln.out_pad = pad16(ln.n_out);
        ln.g_ld = ln.in_pad;
        // layout of the spilled operands: tile-major for the fp16 tiled kernel, row-major for the others (plan_hebbian's choice of
        // kernel depends on the shapes only)
        const int et = ln.out_pad / 16, at = ln.in_pad / 16;
        ln.spill_tm = j >= 1 && (heb_wide(et, at) || heb_narrow_in(et, at)) && !kn.heb_fp32;
    }
    // spill ring
    size_t per_slot = (size_t)e.Bpad * e.out_pad;
    for (int l = 0; l < e.L; ++l) per_slot += (size_t)e.Bpad * e.npad[l] * (l >= 1 ? 2 : 1);
    e.slot_bytes = per_slot *= sizeof(float);
    // defaults sized for 288 GB of HBM per GPU: room for `slot_cap` steps (384: Hebbian segments of 128 steps; 17 GB at cfg-M, capped
    // by the quarter of the device's memory for a shard of 48 000 chains), at least 6 GiB.  Round 2: a 2 GiB ring (segments of 24)
    // cost 1.4 % more per step at cfg-M; 6 GiB instead of 24 cost 13 % at 24 000 chains (segments of 17 steps).  Round 3 (step kernel
    // on every CU, the flush a phase of its own): 192 / 384 / 576 slots = 12 290 / 12 930 / 13 070 steps/s on the headline call.
    int64_t budget = d.spill_budget_bytes;
    if (budget <= 0) {
        const size_t total_b = total_mem ? total_mem : (size_t)64 << 30;
        budget = std::max<int64_t>((int64_t)6 << 30, std::min<int64_t>((int64_t)kn.slot_cap * (int64_t)per_slot, (int64_t)(total_b / 4)));
    }
    if (kn.spill_gb > 0) budget = (int64_t)kn.spill_gb << 30;
    e.slots = (int)std::max<int64_t>(1, std::min<int64_t>(kn.slot_cap, budget / (int64_t)per_slot));
    // `half_slots` = slots of one PART of the ring = steps of one Hebbian segment
    if (kn.no_overlap || e.slots < 2) e.half_slots = e.slots;          // serial flushes on the caller's stream: one part
    else if (e.slots >= kn.ring_parts) { e.half_slots = e.slots / kn.ring_parts; e.slots = e.half_slots * kn.ring_parts; }
    else { e.slots &= ~1; e.half_slots = e.slots / 2; }                   // fewer slots than parts: two halves
    plan_slabs(e);
    // the tables
    if (e.lw) {
        std::vector<LwJob> bwd;
        lw_job_table(e.L, e.npad, e.has_head ? e.out_pad : 0, e.lw_table, bwd);
        e.lw_nf = (int)e.lw_table.size(); e.lw_nb = (int)bwd.size();
        if (e.lw_nf > 65535 || e.lw_nb > 65535) return fail(MCPC_EINVAL, "layer-wise kernels: more than 65535 unit-tile jobs per launch");
        e.lw_table.insert(e.lw_table.end(), bwd.begin(), bwd.end());
        e.nwg_live = (e.Bpad / kLwChains) * e.lw_nf;         // workgroups of the forward launch (mcpc_query; one energy slot each)
    } else if (e.ws == 2) build_phases_ws2(e, e.main);
    else build_phases(e, e.main);
    if (e.u.on) build_phases_u(e, e.u.plan);
    if (e.ws == 2 && e.nwg_live > n_cu && kn.rr) return plan_rounds(e, n_cu);
    return 0;
}

// How the Hebbian sums of Linear j are computed for `rows` spilled rows: the LDS-tiled kernel (mcpc_hebbian.h) for wide
// Linears -- as one or two launches whose error-tile groups cover the output exactly (49 tiles = 17 + 16 + 16) -- the same
// kernel with the operands swapped for a wide Linear with a narrow input (256 x 32: the narrow side takes the TE slot),
// and the register-streaming kernel for whatever is left (few output tiles: HBM-bound whatever the tiling).
struct HebPlan {
    bool tiled = false, swapped = false;
    int ra = 0;                                    // activation tiles per wave (TA = 8 ra)
    int te[2] = {0, 0}, n_mt[2] = {0, 0};          // up to two launches: error tiles per group, number of groups
    int n_nt = 1;
    int wave_tiles = 0;                            // streaming kernel: 64 x 64 wave tiles
    int ksplit = 1, rps = 0;
    int ksplit_cap = 1;                            // upper bound of ksplit that never decreases with `rows`: sizes the slabs
                                                   // (tests/test_run_plan_host.py: every flush of a run against a whole ring part's)
};

inline HebPlan plan_hebbian(const Knobs& kn, int ne, int na, int rows) {
    HebPlan h;
    const int et = ne / 16, at = na / 16;
    const bool wide = heb_wide(et, at);
    const bool narrow_in = heb_narrow_in(et, at);       // e.g. 256 x 32
    h.tiled = wide || narrow_in;
    h.swapped = narrow_in;
    if (wide) {
        h.ra = at >= 16 ? 2 : 1;
        h.n_nt = at / (8 * h.ra);
        if (et <= 8) { h.te[0] = 8; h.n_mt[0] = 1; }
        else if (et <= 16) { h.te[0] = 16; h.n_mt[0] = 1; }
        else {
            // et = 17 b + 16 a exactly when b = et mod 16 groups of 17 fit; otherwise groups of 17 with a ragged last one
            const int b17 = et % 16, a16 = (et - 17 * b17) / 16;
            if (et - 17 * b17 >= 0) { h.te[0] = 17; h.n_mt[0] = b17; h.te[1] = 16; h.n_mt[1] = a16; }
            else { h.te[0] = 17; h.n_mt[0] = (et + 16) / 17; }
            if (h.n_mt[0] == 0) { h.te[0] = h.te[1]; h.n_mt[0] = h.n_mt[1]; h.te[1] = 0; h.n_mt[1] = 0; }
        }
    } else if (narrow_in) {
        h.ra = 2; h.n_nt = 1; h.te[0] = at; h.n_mt[0] = 1;          // E slot = activations (at tiles), A slot = errors (16 tiles)
    }
    if (h.tiled) {
        // ~48 stages of 32 rows per workgroup (0.3 ms at cfg-M): short enough that the step kernel's next segment never
        // waits long for CUs, long enough that the slab traffic stays at a few percent of the spill's
        int want = kn.dw_ksplit > 0 ? kn.dw_ksplit : std::max(1, rows / (48 * kHebKB));
        // a small flush (the reference's batch of 256: 25 600 rows, 16 splits) would run 16-48 workgroups of 48 stages on an idle chip,
        // 0.10-0.17 ms per Linear: with at least 8 stages per workgroup, split until the launch has about a workgroup per CU
        if (kn.dw_ksplit <= 0) {
            const int cols = std::max(1, (h.n_mt[0] + h.n_mt[1]) * h.n_nt);
            want = std::max(want, std::min(rows / (8 * kHebKB), (256 + cols - 1) / cols));
        }
        want = std::min(want, std::max(1, rows / kHebKB));
        h.ksplit_cap = want;
        h.rps = ((rows + want - 1) / want + kHebKB - 1) / kHebKB * kHebKB;
        h.ksplit = (rows + h.rps - 1) / h.rps;
    } else {
        h.wave_tiles = ((ne + 63) / 64) * ((na + 63) / 64);
        int ksplit = std::max(1, std::min(4096 / h.wave_tiles, rows / 64));
        h.ksplit_cap = ksplit;
        h.rps = ((rows + ksplit - 1) / ksplit + 15) / 16 * 16;
        h.ksplit = (rows + h.rps - 1) / h.rps;
    }
    return h;
}

// The split-K slabs: every Linear j >= 1 has a region of its own, sized for the most splits a flush of a whole ring part asks for --
// no shorter flush asks for more (tests/test_run_plan_host.py holds every planned flush to it)
inline void plan_slabs(EnginePlan& e) {
    e.slab_floats = 0;
    for (int j = 1; j < e.L + e.has_head; ++j) {
        Lin& ln = e.lin[j];
        ln.slab_splits = plan_hebbian(e.knobs, ln.out_pad, ln.in_pad, e.half_slots * e.Bpad).ksplit_cap;
        ln.slab_off = e.slab_floats;
        ln.slab_floats = (size_t)ln.slab_splits * ((size_t)ln.out_pad * ln.in_pad + ln.out_pad);
        e.slab_floats += ln.slab_floats;
    }
}

// ---- a Hebbian flush as data ----------------------------------------------------------------------------------------------------------------
// One launch of a flush.  The tiled kernels (HEB_F16: mcpc_heb7_kernel, HEB_FP32: mcpc_heb_kernel) run the instantiation `form` of
// kHebForms (mcpc_hebbian.h) on a grid of n_mt x n_nt x ksplit workgroups from output column col0 on; the streaming kernel (HEB_DW:
// mcpc_dw_kernel) covers the Linear with `wave_tiles` 64 x 64 wave tiles.  `stream`: which of the flush's two streams it goes to.
enum { HEB_F16 = 0, HEB_FP32 = 1, HEB_DW = 2 };
inline const char* heb_family_name(int family) { return family == HEB_F16 ? "heb7" : family == HEB_FP32 ? "heb" : "dw"; }
struct FlushLaunch { int family, form, te, ra; bool swapped; int n_mt, n_nt, col0, stream, wave_tiles; };
struct LinFlush {
    int n_launch;
    FlushLaunch launch[2];
    int ksplit, rps;
    float sign;                 // of the sums in the gradient: -1 for a latent Linear, +1 for the read-out
    int tr_cols, tr_ld;         // its weight slab is reduced transposed (ReduceJob; 0, 0: as it lies)
    char text[96];              // mcpc_last_flush_plan
};
struct FlushPlan {
    int n_slots, rows;
    bool two_streams;           // the launches are spread over two streams; else every `stream` is 0
    LinFlush lin[kMaxLatent + 1];       // per Linear j >= 1 (entry 0 is unused)
    unsigned max_blocks;        // gridDim.x of the one mcpc_reduce_jobs_kernel launch behind the GEMMs
};

// The flush of `n_slots` spilled steps: what is launched for every Linear j >= 1, in launch order.  With two streams a launch goes to
// the one with less work queued so far (output columns x input columns of the launch; kernels of one stream run one after the other,
// each leaving the idle CUs half empty while its last workgroups finish).
inline void plan_flush(const EnginePlan& e, int n_slots, bool two_streams, FlushPlan& f) {
    const Knobs& kn = e.knobs;
    f.n_slots = n_slots; f.rows = n_slots * e.Bpad; f.two_streams = two_streams; f.max_blocks = 1;
    const int tiled_family = kn.heb_fp32 ? HEB_FP32 : HEB_F16;
    double load[2] = {0.0, 0.0};
    for (int j = 1; j < e.L + e.has_head; ++j) {
        const Lin& ln = e.lin[j];
        const int ne = ln.out_pad, na = ln.in_pad;
        const HebPlan h = plan_hebbian(kn, ne, na, f.rows);
        LinFlush& lf = f.lin[j];
        lf.n_launch = 0; lf.ksplit = h.ksplit; lf.rps = h.rps;
        lf.sign = j < e.L ? -1.0f : 1.0f;
        lf.tr_cols = h.swapped ? ne : 0; lf.tr_ld = h.swapped ? na : 0;
        int len = 0;
        auto put = [&](const char* fmt, auto... v) { if (len < (int)sizeof lf.text) len += snprintf(lf.text + len, sizeof lf.text - len, fmt, v...); };
        auto add = [&](FlushLaunch l, double cost) {
            l.form = l.family == HEB_DW ? -1 : heb_form_index(l.te, l.ra, l.swapped);
            l.stream = (two_streams && load[1] < load[0]) ? 1 : 0;
            load[l.stream] += cost;
            if (l.family == HEB_DW) put("dw tiles=%d", l.wave_tiles);
            else {
                put("%s%s<%d,%d%s>x%d", lf.n_launch ? "+" : "", heb_family_name(l.family), l.te, l.ra, l.swapped ? ",T" : "", l.n_mt);
                if (l.n_nt > 1) put("*%d", l.n_nt);
            }
            lf.launch[lf.n_launch++] = l;
        };
        if (h.swapped) {
            // transposed product: the activations take the E slot (te = their tiles), the errors the A slot
            add({tiled_family, 0, h.te[0], 2, true, 1, 1, 0, 0, 0}, (double)ne * na);
        } else if (h.tiled) {
            int col = 0;
            for (int g = 0; g < 2; ++g) {
                if (h.n_mt[g] == 0) continue;
                int ra = h.ra, n_nt = h.n_nt;
                // tuning heb171=1: <17, 2>'s 136 accumulators + the rest do not fit 256 registers (19 spilled) -- 8 activation tiles per
                // workgroup instead, i.e. twice the activation groups: this group's 272 error columns are read twice (+6.5 MB per step at cfg-M)
                if (h.te[g] == 17 && ra == 2 && tiled_family == HEB_F16 && kn.heb171) { ra = 1; n_nt *= 2; }
                add({tiled_family, 0, h.te[g], ra, false, h.n_mt[g], n_nt, col, 0, 0}, (double)h.n_mt[g] * h.te[g] * 16 * na);
                col += h.n_mt[g] * h.te[g] * 16;
            }
        } else {
            add({HEB_DW, 0, 0, 0, false, 0, 0, 0, 0, h.wave_tiles}, (double)ne * na);
        }
        put(" ksplit=%d rps=%d %s", h.ksplit, h.rps, ln.spill_tm ? "tm" : "rm");
        f.max_blocks = std::max(f.max_blocks, (unsigned)std::min<size_t>(((size_t)ne * na + 255) / 256, 2048));
    }
}

// ---- the schedule of a run -----------------------------------------------------------------------------------------------------------------
// energy partials per step: one slot per workgroup; the in-place kernel indexes them by 16-chain tile
inline size_t energy_slots(const EnginePlan& e) { return e.lw ? (size_t)e.nwg_live : e.ws == 2 ? (size_t)e.Bpad / 16 : (size_t)e.nwg; }

// the lean epilogues address every [Bpad][npad] image with 32-bit lane offsets (KParams::lean_ok)
inline bool lean_ok(const EnginePlan& e) {
    int widest = e.out_pad;
    for (int l = 0; l < e.L; ++l) widest = std::max(widest, e.npad[l]);
    return e.Bpad < (1 << 24) && (uint64_t)e.Bpad * (uint64_t)widest * 4u < (1ull << 32) && !e.knobs.no_lean;
}

// The unified-wave kernel (mcpc_steps_u.h) serves the lean runs of an engine that holds its plan: fused SGD update with or without
// the Philox kick, Adam without noise.  Everything else -- gradients-only runs, injected noise -- keeps the main plan's kernel.
inline bool use_unified(const EnginePlan& e, const mcpc_run_desc& r) {
    return e.u.on && (e.u.prefer || (e.has_head && r.loss_kind == MCPC_LOSS_NONE)) && e.ws == 2 && r.update_x && lean_ok(e) &&
           ((r.xopt_kind == MCPC_XOPT_SGD && r.noise_mode != MCPC_NOISE_EXTERNAL) ||
            (r.xopt_kind == MCPC_XOPT_ADAM && r.noise_mode == MCPC_NOISE_NONE));
}

inline int check_step_range(const mcpc_run_desc& r) {
    if (r.T < 1 || r.t_begin < 0 || r.n_steps < 1 || r.t_begin + r.n_steps > r.T)
        return fail(MCPC_EINVAL, "bad step range: T=%d t_begin=%d n_steps=%d", r.T, r.t_begin, r.n_steps);
    return 0;
}

// One item of a run: steps [t0, t0 + n) as ONE plain launch (q == 0: the layer-wise pair, the unified-wave, in-place or barrier kernel,
// as the engine and the run have it) or as ONE cycle of the round schedule (q >= 1: rr_k launches of q steps, n == rr_m q).  An item
// lies wholly on one side of the accumulation window; one inside it (`acc`) is a Hebbian segment: it spills into slots
// [slot0, slot0 + n) of the ring -- part `part` -- and a flush of those n slots follows it: `flush` is its index in RunPlan::flushes (-1: none).
struct RunItem { int t0, n, q; bool acc; int part, slot0, flush; };
struct RunPlan {
    bool unified = false;           // the run is served by the unified-wave kernel (use_unified), else by the engine's main plan
    bool accumulates = false;       // some step of the run lies in the accumulation window
    bool lean_ok = false;
    bool overlap = false;           // flushes run on the auxiliary stream beside the next segment (a ring of n_parts parts), else serially
    int n_parts = 1;
    std::vector<RunItem> items;
    std::vector<FlushPlan> flushes; // one per distinct length of the run's Hebbian segments (plan_flush)
};

// What mcpc_run launches for `r`, in order: a pure function of the engine's plan and the fields of the descriptor that shape a run
// (T, t_begin, n_steps, acc_begin, acc_end, update_x, xopt_kind, noise_mode, loss_kind).  `stamps`: the diagnostic build with in-kernel
// stamps, which never uses the round schedule.  Non-accumulating stretches run as one persistent launch (on the round schedule: whole
// cycles, longest launches first, and one plain launch for fewer than rr_m steps left: hardware rounds); accumulating stretches are cut
// at the capacity of a ring part, every segment one cycle where the round schedule applies, and the flush behind a segment is planned
// once per distinct segment length (two flush streams: overlapped flushes and tuning flush_streams >= 2).  `p.items` and `p.flushes`
// keep their storage between runs.
// (tests/test_run_plan_host.py, through mcpc_debug_run_plan)
inline void plan_run(const EnginePlan& e, const mcpc_run_desc& r, bool stamps, RunPlan& p) {
    const int acc_b = std::max(r.acc_begin, 0), acc_e = std::min(r.acc_end, r.T);
    const int end = r.t_begin + r.n_steps;
    p.unified = use_unified(e, r);
    p.accumulates = acc_b < acc_e && r.t_begin < acc_e && end > acc_b;
    p.lean_ok = lean_ok(e);
    p.overlap = e.half_slots < e.slots;
    p.n_parts = std::max(1, e.slots / std::max(1, e.half_slots));
    p.items.clear();
    p.flushes.clear();
    const bool rr_ok = e.rr && r.update_x && !stamps;
    // a launch's row-exponent words carry their generation -- the step of the launch, or step x entries + entry for a ring slot -- in 24
    // bits (mcpc_kernels.h: rowexp_track): longer stretches are cut into several launches (a wrapped generation would never supersede
    // the stale word)
    const int gen_cap = ((1 << 24) - 2) / std::max(std::max(e.main.n_phases, e.u.plan.n_phases), 1);
    const int tail = e.knobs.flush_tail;
    int part = 0;                                         // part of the ring the next accumulating segment spills into
    for (int t = r.t_begin; t < end;) {
        const bool in_acc = t >= acc_b && t < acc_e;
        int n;
        if (in_acc) {
            const int rem = std::min(end, acc_e) - t;
            n = std::min(rem, e.half_slots);
            // the flush of a stretch's LAST segment has no step kernel to hide behind: keep that segment short
            if (p.overlap && tail > 0 && rem <= e.half_slots && rem >= 2 * tail && std::min(end, acc_e) == acc_e) n = rem - tail;
        }
        else n = (t < acc_b ? std::min(end, acc_b) : end) - t;
        n = std::min(n, gen_cap);
        int q = 0;
        if (rr_ok && in_acc) {
            q = n / e.rr_m;                                   // a Hebbian segment is one cycle (fewer steps than rr_m left: plain launch)
            if (q >= 1) n = q * e.rr_m;
        } else if (rr_ok) {
            while (n >= e.rr_m) {
                const int qc = std::min(std::max(1, e.knobs.rr_qmax), n / e.rr_m);
                p.items.push_back({t, qc * e.rr_m, qc, false, 0, 0, -1});
                t += qc * e.rr_m; n -= qc * e.rr_m;
            }
            if (n == 0) continue;
        }
        int flush = -1;
        for (size_t i = 0; in_acc && i < p.flushes.size(); ++i)
            if (p.flushes[i].n_slots == n) flush = (int)i;
        if (in_acc && flush < 0) {
            flush = (int)p.flushes.size();
            p.flushes.emplace_back();
            plan_flush(e, n, p.overlap && e.knobs.flush_streams >= 2, p.flushes.back());
        }
        const bool ring = in_acc && p.overlap;                // (a serial run keeps part 0, slot 0)
        p.items.push_back({t, n, q, in_acc, ring ? part : 0, ring ? part * e.half_slots : 0, flush});
        if (ring) part = (part + 1) % p.n_parts;
        t += n;
    }
}

}  // namespace mcpc

// ---- mcpc_debug_plan: a plan as JSON ------------------------------------------------------------------------------------------------------
namespace mcpc {

inline void json_add(std::string& s, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s += buf;
}

inline void json_step_plan(std::string& s, const StepPlan& p) {
    json_add(s, "{\"lds_bytes\":%d,\"xl\":%d,\"g_first\":%d,\"chunk\":%d,\"ring\":%d,\"overlay\":%d,\"head_ld\":%d,\"lds_yw\":%d,\"n_phases\":%d,\"rows\":%d,\"regions\":[",
             p.lds_bytes, p.xl ? 1 : 0, p.g_first, p.ws2_chunk, p.ws2_ring, p.ws2_overlay ? 1 : 0, p.head_ld, p.lds_yw, p.n_phases,
             p.n_phases ? (int)p.table.size() / p.n_phases : 0);
    for (size_t i = 0; i < p.regions.size(); ++i)
        json_add(s, "%s[\"%s\",%d,%d,%d]", i ? "," : "", p.regions[i].name, p.regions[i].layer, p.regions[i].off, p.regions[i].floats);
    s += "],\"fields\":[\"type\",\"layer\",\"tile0\",\"ntiles\",\"a_tile_stride\",\"a_off0\",\"nkb\",\"kw\",\"b_lds\",\"ldb\",\"flags\",\"sign\",\"out_lds\",\"out_ld\","
         "\"dep_e\",\"dep_g\",\"a_lin\",\"rot\",\"dep_se\",\"next_g\",\"b_row\",\"o_row\"],\"table\":[";
    for (size_t i = 0; i < p.table.size(); ++i) {
        const KPhase& k = p.table[i];
        json_add(s, "%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%g,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", i ? "," : "", k.type, k.layer, k.tile0, k.ntiles, k.a_tile_stride,
                 k.a_off0, k.nkb, k.kw, k.b_lds, k.ldb, k.flags, (double)k.sign, k.out_lds, k.out_ld, k.dep_e, k.dep_g, k.a_lin, k.rot, k.dep_se, k.next_g, k.b_row, k.o_row);
    }
    s += "]}";
}

inline std::string plan_json(const EnginePlan& e) {
    std::string s;
    const int nlin = e.L + (e.has_head ? 1 : 0);
    json_add(s, "{\"form\":\"%s\",\"kernel\":\"%s\",\"Bpad\":%d,\"workgroups\":%d,\"chains_per_wg\":%d,\"waves\":%d,\"out_pad\":%d,\"slots\":%d,\"half_slots\":%d,\"npad\":[",
             e.lw ? "layer-wise" : e.ws == 2 ? "in-place" : "barrier", step_kernel_name(e), e.Bpad, e.nwg_live, e.lw ? kLwChains : e.ct, e.nw, e.out_pad, e.slots, e.half_slots);
    for (int l = 0; l < e.L; ++l) json_add(s, "%s%d", l ? "," : "", e.npad[l]);
    s += "],\"spill_tm\":[";
    for (int j = 0; j < nlin; ++j) json_add(s, "%s%d", j ? "," : "", e.lin[j].spill_tm ? 1 : 0);
    json_add(s, "],\"slab_floats\":%zu,\"slabs\":[", e.slab_floats);
    for (int j = 0; j < nlin; ++j) json_add(s, "%s[%zu,%zu,%d]", j ? "," : "", e.lin[j].slab_off, e.lin[j].slab_floats, e.lin[j].slab_splits);
    s += "],\"main\":";
    json_step_plan(s, e.main);
    json_add(s, ",\"unified\":{\"ok\":%d,\"on\":%d,\"prefer\":%d,\"plan\":", e.u.ok ? 1 : 0, e.u.on ? 1 : 0, e.u.prefer ? 1 : 0);
    json_step_plan(s, e.u.plan);
    json_add(s, "},\"lw\":{\"chains\":%d,\"unit_tiles\":%d,\"n_fwd\":%d,\"n_bwd\":%d,\"jobs\":[", kLwChains, kLwUnitTiles, e.lw_nf, e.lw_nb);
    for (size_t i = 0; i < e.lw_table.size(); ++i) json_add(s, "%s[%d,%d]", i ? "," : "", e.lw_table[i].layer, e.lw_table[i].ut0);
    json_add(s, "]},\"rounds\":{\"on\":%d,\"k\":%d,\"m\":%d,\"u_kernel\":\"%s\",\"launches\":[", e.rr ? 1 : 0, e.rr_k, e.rr_m, e.u_rr_name.c_str());
    for (int i = 0; i < e.rr_k; ++i) {
        s += i ? ",[" : "[";
        const int* ids = e.rr_host.data() + e.rr_off[i];
        for (int j = 0; j < e.rr_count[i]; ++j) json_add(s, "%s[%d,%d]", j ? "," : "", ids[j], ids[e.rr_count[i] + j]);
        s += "]";
    }
    s += "]}}";
    return s;
}

// mcpc_debug_run_plan: the schedule of a run, and the planned flush (RunPlan::flushes) behind each of its Hebbian segments
inline std::string run_plan_json(const EnginePlan& e, const RunPlan& p) {
    std::string s;
    json_add(s, "{\"unified\":%d,\"accumulates\":%d,\"lean_ok\":%d,\"overlap\":%d,\"n_parts\":%d,"
                "\"fields\":[\"t0\",\"n\",\"q\",\"acc\",\"part\",\"slot0\",\"flush\"],\"items\":[",
             p.unified ? 1 : 0, p.accumulates ? 1 : 0, p.lean_ok ? 1 : 0, p.overlap ? 1 : 0, p.n_parts);
    for (size_t i = 0; i < p.items.size(); ++i) {
        const RunItem& it = p.items[i];          // ("flush": a flush of the item's n slots follows it -- every Hebbian segment, nothing else)
        json_add(s, "%s[%d,%d,%d,%d,%d,%d,%d]", i ? "," : "", it.t0, it.n, it.q, it.acc ? 1 : 0, it.part, it.slot0, it.acc ? 1 : 0);
    }
    s += "],\"flush_fields\":[\"ksplit\",\"rps\",\"ksplit_cap\"],"
         "\"launch_fields\":[\"family\",\"form\",\"te\",\"ra\",\"swapped\",\"n_mt\",\"n_nt\",\"col0\",\"stream\",\"wave_tiles\"],"
         "\"reduce_fields\":[\"sign\",\"tr_cols\",\"tr_ld\"],\"flushes\":[";
    const int nlin = e.L + (e.has_head ? 1 : 0);
    bool first = true;
    for (const RunItem& it : p.items) {
        if (it.flush < 0) continue;
        const FlushPlan& f = p.flushes[it.flush];
        json_add(s, "%s{\"rows\":%d,\"two_streams\":%d,\"max_blocks\":%u,\"lin\":[", first ? "" : ",", f.rows, f.two_streams ? 1 : 0, f.max_blocks);
        first = false;
        for (int j = 1; j < nlin; ++j) json_add(s, "%s[%d,%d,%d]", j > 1 ? "," : "", f.lin[j].ksplit, f.lin[j].rps, e.lin[j].slab_splits);
        s += "],\"launches\":[";
        for (int j = 1; j < nlin; ++j) {
            s += j > 1 ? ",[" : "[";
            for (int i = 0; i < f.lin[j].n_launch; ++i) {
                const FlushLaunch& l = f.lin[j].launch[i];
                json_add(s, "%s[\"%s\",%d,%d,%d,%d,%d,%d,%d,%d,%d]", i ? "," : "", heb_family_name(l.family), l.form, l.te, l.ra, l.swapped ? 1 : 0,
                         l.n_mt, l.n_nt, l.col0, l.stream, l.wave_tiles);
            }
            s += "]";
        }
        s += "],\"reduce\":[";
        for (int j = 1; j < nlin; ++j) json_add(s, "%s[%g,%d,%d]", j > 1 ? "," : "", (double)f.lin[j].sign, f.lin[j].tr_cols, f.lin[j].tr_ld);
        s += "],\"text\":[";
        for (int j = 1; j < nlin; ++j) json_add(s, "%s\"%s\"", j > 1 ? "," : "", f.lin[j].text);
        s += "]}";
    }
    s += "]}";
    return s;
}

}  // namespace mcpc
