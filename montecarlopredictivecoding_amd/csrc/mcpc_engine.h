// The engine behind the C handle `mcpc_engine` (include/mcpc.h), and the few functions that cross a translation-unit boundary of
// libmcpc.so (the step kernels' launchers have a header of their own: mcpc_step_forms.h).  Host declarations and small inline templates
// only: no kernel is defined here or in anything this header includes.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is loaded with dlopen on first use (no link dependency)

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "mcpc_host.h"
#include "mcpc_plan.h"

using namespace mcpc;           // (the struct is the C header's global tag; the units that include this header are the library's own)

// An engine is its plan (mcpc_plan.h: what plan_engine decided from the descriptor and the device) and the device state built from it
struct mcpc_engine : mcpc::EnginePlan {
    mcpc_net_desc d{};
    ncclComm_t comm = nullptr;      // mcpc_comm_init: the shards' communicator (RCCL), one rank per engine
    int comm_ranks = 0;
    float* x[kMaxLatent]{};
    float* m[kMaxLatent]{};
    float* v[kMaxLatent]{};
    float* e0sum = nullptr;
    float* mu1 = nullptr;
    float* ypad = nullptr;
    float* ytile = nullptr;         // tile-major copy of ypad (KHead::ytile)
    uint32_t* ybits = nullptr;      // bit-packed copy of a 0/1 target (see mcpc_pack_target_bits_kernel)
    int* y_binary = nullptr;        // device flag: the bound target is exactly 0/1 everywhere
    int ywords = 0;
    bool target_bound = false;
    // host copy of the three flag words (target_flags_on_host): requested by mcpc_bind_target behind its kernels; engines that may take a
    // specialised instantiation of the in-place kernel only
    int* y_flags_host = nullptr;    // pinned
    hipEvent_t y_flags_ev = nullptr;
    bool y_flags_pending = false;
    const float* inputs = nullptr;
    // Hebbian spill ring (EnginePlan::slots in parts of half_slots): the flush of one part runs on `aux` while the step kernel fills another
    hipStream_t aux = nullptr;
    hipEvent_t ev_steps[kMaxRingParts] = {}, ev_flush[kMaxRingParts] = {};
    hipStream_t spacer = nullptr;   // never used: see ensure_spill
    hipStream_t aux3 = nullptr;     // second low-priority stream of the overlapped flush: the GEMMs of a flush alternate between the two,
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // so that the tail of one launch is filled by the next (same-stream kernels serialise)
    bool flush_pending[kMaxRingParts] = {};
    float* spill_a[kMaxLatent]{};
    float* spill_e[kMaxLatent]{};
    float* spill_eo = nullptr;
    float* slab = nullptr;          // EnginePlan::slab_floats floats
    // energies
    double* epart = nullptr;
    size_t epart_rows = 0;
    float* adam_coef = nullptr;     // device table [steps][2]; grown buffers are retired, never freed under a running kernel
    size_t adam_cap = 0;
    float* adam_host[2] = {nullptr, nullptr};     // pinned staging, double-buffered: a run never rewrites a table whose upload may be pending
    size_t adam_host_cap[2] = {0, 0};
    hipEvent_t adam_ev[2] = {nullptr, nullptr};
    int adam_next = 0;
    struct Retired { void* p; hipEvent_t ev; };
    std::vector<Retired> retired;   // device buffers replaced by larger ones while earlier launches may still use them: each carries an event
                                    // recorded on the stream at retirement and is freed by the first later run that finds the event complete
    bool spill_ready = false;       // the spill ring, its stream/events and the slabs exist (allocated by the first accumulating run)
    int* err = nullptr;             // device error word written by the kernels
    int* wexp = nullptr;            // [kMaxLatent + 1] per Linear: the power of two its packed weights are scaled by (mcpc_wexp_kernel)
    unsigned* spillmax = nullptr;   // [kMaxRingParts][kSpillTensors]: per ring part, the largest |value| per spilled tensor of the segment
                                    // that filled it (bit patterns; written by the step kernels, read by the Hebbian GEMMs of that part)
    // layer-wise kernels (mcpc_steps_lw.h): state, activations and errors of all chains in global memory, two launches per step
    float* lw_fx[kMaxLatent]{};     // f(x_l) [Bpad][npad_l]
    float* lw_err[kMaxLatent]{};    // e_l, l >= 1
    float* lw_err_o = nullptr;      // e_o [Bpad][out_pad]
    LwJob* lw_jobs = nullptr;       // device copy of lw_table
    unsigned long long* clk = nullptr;   // profiling: {shader cycles, 100 MHz ticks} of one wave per launch (KParams::clk)
    float* dummy = nullptr;         // 4 KiB of zeros (KParams::dummy)
    int* rr_tab = nullptr;          // device copy of rr_host (round schedule)
    // per-chain energies (mcpc_chain_energy.h): the evaluator's own scratch, allocated by the first mcpc_chain_energies and grown by a
    // call that asks for a larger chunk (the old buffers are retired, like every buffer launches in the stream may still use)
    float* ce_x[kMaxLatent]{};      // x_l    [ce_rows][npad_l]
    float* ce_fx[kMaxLatent]{};     // f(x_l) [ce_rows][npad_l]
    float* ce_mu1 = nullptr;        // mu_1 of the call's inputs [Bpad][npad_0]
    double* ce_part = nullptr;      // [job][ce_rows]
    LwJob* ce_jobs = nullptr;       // device copy of the job table (ce_job_table)
    int ce_njobs = 0, ce_nhead = 0;
    CeFinish ce_finish{};
    int ce_rows = 0;                // rows the scratch holds (a multiple of kLwChains)
    // prediction errors (mcpc_pred_err.h) share that scratch; their job table is ce_table filtered to the Linears of the last call
    std::vector<LwJob> ce_table;    // host copy of ce_jobs
    LwJob* pe_jobs = nullptr;       // device copy of pe_job_table(ce_table, pe_want)
    unsigned pe_want = 0;
    int pe_njobs = 0;
    // gradients of handed-over states (mcpc_state_grad.h): the error rows beside that scratch, allocated by the first mcpc_state_gradients
    // and re-allocated whenever the evaluators' chunk grows; the backward half of lw_job_table (every engine form: not lw_jobs)
    float* sg_err[kMaxLatent]{};    // e_l [sg_rows][npad_l], l >= 1
    float* sg_err_o = nullptr;      // e_o [sg_rows][out_pad]
    int sg_rows = 0;                // rows the error rows hold (0, or ce_rows)
    LwJob* sg_bjobs = nullptr;
    int sg_nb = 0;
    RunPlan run_plan;              // the schedule of the last mcpc_run (plan_run); kept for its storage: no allocation per run
    // diagnostics, host strings set while launching (no device work): what the last mcpc_run and each Linear's last flush launched
    std::string last_step;                       // mcpc_last_step_kernel_name
    std::string last_flush[kMaxLatent + 1];      // mcpc_last_flush_plan, per Linear j >= 1
    // profiling
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // HIP events around every launch of the step kernel
    size_t events_used = 0;
    double prof_steps = 0;          // whole-shard steps covered by the bracketed launches
#ifdef MCPC_STAMPS
    unsigned long long* dbg = nullptr;
#endif
};

namespace mcpc {

// ---- device buffers of an engine (retire, free_completed_retired: mcpc_api.hip) -----------------------------------------------------------
template <typename T>
int dmalloc(T*& p, size_t count) {
    void* q = nullptr;
    hipError_t err = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (err != hipSuccess) return fail(MCPC_ENOMEM, "hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(err));
#ifdef MCPC_POISON_ALLOC      // diagnostic build: every fresh device allocation is filled with 0xFF bytes (NaN as fp32 / fp64, -1 as int), so that a
                              // read of memory nobody initialised shows on every box, not only on one whose fresh pages are not zero
    if (hipMemset(q, 0xFF, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return fail(MCPC_EHIP, "hipMemset (poison) failed");
#endif
    p = (T*)q;
    return 0;
}
// A table the planner built, copied to the device
template <typename T>
int upload(T*& dev, const std::vector<T>& host, const char* what) {
    if (const int rc = dmalloc(dev, host.size())) return rc;
    if (hipMemcpy(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return fail(MCPC_EHIP, "hipMemcpy of %s failed", what);
    return 0;
}
// A buffer that launches already in the stream may still use is not freed but retired behind an event.
void retire(mcpc_engine* e, void* p, hipStream_t stream);
// The engine gives a buffer up (retired if there is one, the pointer cleared), and replaces it by one of `count` elements: nothing waits
template <typename T>
void give_up(mcpc_engine* e, T*& p, hipStream_t stream) { if (p) retire(e, (void*)p, stream); p = nullptr; }
template <typename T>
int regrow(mcpc_engine* e, T*& p, size_t count, hipStream_t stream) { give_up(e, p, stream); return dmalloc(p, count); }
// A retired buffer is freed by a later run once its event has completed (never under a kernel that uses it)
void free_completed_retired(mcpc_engine* e);

// ---- what mcpc_run (mcpc_run.hip) shares with the evaluators (mcpc_eval.hip) and the layer-wise launcher (mcpc_steps_lw.hip) ---------------
// mcpc_api.hip -- mu_1 = inputs W0^T + b0 into `dst` [padded][npad_0] for `rows` rows of inputs: one kernel for the runs and the evaluators,
// so that all of them see the same bits
void launch_mu1(const mcpc_engine* e, const float* inputs, float* dst, int rows, int padded, hipStream_t stream);
// mcpc_run.hip -- the loss arguments of a run or of an evaluator call.  `pre` opens every message: "" for mcpc_run, "<entry>: " for an evaluator.
int check_loss_kind(const char* pre, int32_t kind);
int check_loss_values(const char* pre, const mcpc_engine* e, int32_t loss_kind, double loss_var, int32_t mask_start);
int check_loss(const char* pre, const mcpc_engine* e, int32_t loss_kind, double loss_var, int32_t mask_start);
// A launch window of a run: steps [t0, t0 + n), and the rows of the run's per-step tables (Adam coefficients, injected noise) it starts at
inline void set_window(const mcpc_engine* e, const mcpc_run_desc* r, KParams& P, int t0, int n) {
    P.t0 = t0; P.n_steps = n;
    const size_t s0 = (size_t)(t0 - r->t_begin);
    P.adam_coef = r->xopt_kind == MCPC_XOPT_ADAM ? e->adam_coef + 2 * s0 : nullptr;
    if (r->noise_mode == MCPC_NOISE_EXTERNAL)
        for (int l = 0; l < e->L; ++l) P.layer[l].ext_noise = r->ext_noise[l] + s0 * e->d.batch * e->d.sizes[l];
}

// mcpc_flush.hip -- one Hebbian flush, as planned (plan_flush): fold the spilled steps from slot `slot0` on into the gradient sums of
// every Linear j >= 1, on `stream` (and the engine's second flush stream where the plan says so).  `part`: the ring part, whose
// spilled maxima scale the fp16 operands.  Called by mcpc_run (mcpc_run.hip).
int flush_spill(mcpc_engine* e, const FlushPlan& f, int slot0, hipStream_t stream, int part);

}  // namespace mcpc
