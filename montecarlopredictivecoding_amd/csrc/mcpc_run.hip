// libmcpc.so, mcpc_run: the checks of a run descriptor, the per-run device tables, the kernel parameters, and the executor of the run's
// plan (mcpc_plan.h: plan_run) -- a plain launch or a cycle of the round schedule per item, each followed by its Hebbian flush where the
// item accumulates.  No step kernel is defined or named here: every form is launched through mcpc_step_forms.h, the flush through
// flush_spill (mcpc_flush.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "mcpc_build.h"
#include "mcpc_engine.h"
#include "mcpc_step_forms.h"
#include "mcpc_run_kernels.h"           // mcpc_dw0_kernel, mcpc_energy_reduce_kernel

using namespace mcpc;

// The loss arguments of a run or of an evaluator call (mcpc_engine.h)
int mcpc::check_loss_kind(const char* pre, int32_t kind) { return kind < 0 || kind > 2 ? fail(MCPC_EINVAL, "%sloss_kind=%d", pre, kind) : 0; }
int mcpc::check_loss_values(const char* pre, const mcpc_engine* e, int32_t loss_kind, double loss_var, int32_t mask_start) {
    if (loss_kind == MCPC_LOSS_GAUSSIAN && !(loss_var > 0.0)) return fail(MCPC_EINVAL, "%sloss_var must be positive", pre);
    if (mask_start < 0 || mask_start >= e->d.n_out) return fail(MCPC_EINVAL, "%smask_start=%d outside 0..%d", pre, mask_start, e->d.n_out - 1);
    return 0;
}
int mcpc::check_loss(const char* pre, const mcpc_engine* e, int32_t loss_kind, double loss_var, int32_t mask_start) {
    if (const int rc = check_loss_kind(pre, loss_kind)) return rc;
    if (loss_kind == MCPC_LOSS_NONE) return 0;
    if (!e->has_head) return fail(MCPC_EINVAL, "%sa loss needs a read-out Linear (n_out > 0)", pre);
    if (!e->target_bound) return fail(MCPC_ESTATE, "%sloss requested but no target bound", pre);
    return check_loss_values(pre, e, loss_kind, loss_var, mask_start);
}

namespace {

// Allocated by the first run that accumulates Hebbian sums (inference-only engines never pay for it): the spill ring, the
// slabs of the split-K partial sums (sized by plan_engine), the low-priority stream and events of the overlapped flush.
int ensure_spill(mcpc_engine* e, hipStream_t stream) {
    if (e->spill_ready) return 0;
    int rc;
    if (e->half_slots < e->slots && !e->aux) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);           // lo = least urgent
        // Streams become hardware queues in the order they are created, and the queues are dealt out over the pipes of the
        // command processor: which pipe the two flush queues share with whom is worth 0.5 % of the learning call (94.3
        // against 94.7 us per step) and can be neither asked nor requested.  One stream created in front of them -- never
        // used -- puts them where they measured best in a process whose only other compute queue is the caller's (any one
        // extra stream, of any priority, did; two did worse by 2 %: 96.6).
        if (!e->spacer) (void)hipStreamCreateWithFlags(&e->spacer, hipStreamNonBlocking);
        if (hipStreamCreateWithPriority(&e->aux, hipStreamNonBlocking, lo) != hipSuccess) return fail(MCPC_EHIP, "hipStreamCreateWithPriority failed");
        if (e->knobs.flush_streams >= 2 &&
            (hipStreamCreateWithPriority(&e->aux3, hipStreamNonBlocking, lo) != hipSuccess ||
             hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess))
            return fail(MCPC_EHIP, "second flush stream could not be created");
        for (int h = 0; h < kMaxRingParts; ++h)
            if (hipEventCreateWithFlags(&e->ev_steps[h], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&e->ev_flush[h], hipEventDisableTiming) != hipSuccess)
                return fail(MCPC_EHIP, "hipEventCreate failed");
    }
    for (int l = 0; l < e->L; ++l) {
        const size_t n = (size_t)e->slots * e->Bpad * e->npad[l];
        if (!e->spill_a[l] && (rc = dmalloc(e->spill_a[l], n))) return rc;
        if (l >= 1 && !e->spill_e[l] && (rc = dmalloc(e->spill_e[l], n))) return rc;
    }
    if (e->has_head && !e->spill_eo && (rc = dmalloc(e->spill_eo, (size_t)e->slots * e->Bpad * e->out_pad))) return rc;
    // rows of a 16-chain unit that is all padding (never launched) read as zero in every slot: the Hebbian GEMMs sum over all Bpad rows.
    // On the RUN's stream: the step kernels and (behind ev_steps) the flushes of this and every later run are ordered after it, also when
    // the caller's stream is a non-blocking one that the null stream does not synchronise with.
    if (e->nwg_live * e->ct < e->Bpad && e->ws == 2) {
        const size_t live = (size_t)e->nwg_live * 16, dead = (size_t)e->Bpad - live;
        auto zero_tail = [&](float* base, int npad) {
            return hipMemset2DAsync(base + live * npad, (size_t)e->Bpad * npad * sizeof(float), 0, dead * npad * sizeof(float), (size_t)e->slots, stream) == hipSuccess;
        };
        bool ok = true;
        for (int l = 0; l < e->L; ++l) { ok = ok && zero_tail(e->spill_a[l], e->npad[l]); if (l >= 1) ok = ok && zero_tail(e->spill_e[l], e->npad[l]); }
        if (e->has_head) ok = ok && zero_tail(e->spill_eo, e->out_pad);
        if (!ok) return fail(MCPC_EHIP, "hipMemset2D of the spill ring's padding rows failed");
    }
    if (!e->slab && (rc = dmalloc(e->slab, e->slab_floats))) return rc;
    e->spill_ready = true;
    return 0;
}

int check_run(const mcpc_engine* e, const mcpc_run_desc* r) {
    const int nlin = e->L + (e->has_head ? 1 : 0);
    for (int j = 0; j < nlin; ++j)
        if (!e->lin[j].bound) return fail(MCPC_ESTATE, "Linear %d has no bound parameters (mcpc_bind_params + mcpc_params_changed first)", j);
    if (const int rc = check_step_range(*r)) return rc;
    if (const int rc = check_loss("", e, r->loss_kind, r->loss_var, r->mask_start)) return rc;
    if (r->xopt_kind != MCPC_XOPT_SGD && r->xopt_kind != MCPC_XOPT_ADAM) return fail(MCPC_EINVAL, "xopt_kind=%d", r->xopt_kind);
    if (!(r->lr > 0.0)) return fail(MCPC_EINVAL, "lr must be positive");
    if (r->noise_mode < 0 || r->noise_mode > 2) return fail(MCPC_EINVAL, "noise_mode=%d", r->noise_mode);
    if (r->noise_mode != MCPC_NOISE_NONE && r->xopt_kind != MCPC_XOPT_SGD)
        return fail(MCPC_EINVAL, "the fused Langevin kick is defined for SGD on x only (reference utils/model.py:35-44 steps the same optimizer)");
    if (r->noise_mode != MCPC_NOISE_NONE && !(r->noise_var >= 0.0)) return fail(MCPC_EINVAL, "noise_var must be >= 0");
    if (r->noise_mode == MCPC_NOISE_EXTERNAL)
        for (int l = 0; l < e->L; ++l)
            if (!r->ext_noise[l]) return fail(MCPC_EINVAL, "ext_noise[%d] is null", l);
    if (!r->update_x)
        for (int l = 0; l < e->L; ++l)
            if (!r->xgrad[l]) return fail(MCPC_EINVAL, "update_x=0 needs xgrad[%d]", l);
    if (r->energy_mode < 0 || r->energy_mode > 2) return fail(MCPC_EINVAL, "energy_mode=%d", r->energy_mode);
    if (r->energy_mode != MCPC_ENERGY_NONE && !r->energies_out) return fail(MCPC_EINVAL, "energies_out is null");
    if (r->rec_count < 0 || (r->rec_count > 0 && r->rec_stride < 1)) return fail(MCPC_EINVAL, "bad record schedule");
    return 0;
}

// The per-run device tables, in stream order: Adam's bias corrections, room for the energy partials, mu_1, the layer-wise kernels'
// f(x_l), the spill ring of a run that accumulates (`run_accumulates`) and its cleared sums.
int prepare_run(mcpc_engine* e, const mcpc_run_desc* r, bool run_accumulates, hipStream_t stream) {
    if (r->xopt_kind == MCPC_XOPT_ADAM) {
        const size_t need = (size_t)r->n_steps * 2;
        if (need > e->adam_cap) {
            size_t cap = 1024;
            while (cap < need) cap *= 2;
            if (const int rc = regrow(e, e->adam_coef, cap, stream)) return rc;
            e->adam_cap = cap;
        }
        // pinned staging table, double-buffered; the event wait below is a no-op unless the upload issued two Adam runs ago
        // has still not executed
        const int hb = e->adam_next; e->adam_next ^= 1;
        if (!e->adam_ev[hb]) HIP_TRY(hipEventCreateWithFlags(&e->adam_ev[hb], hipEventDisableTiming));
        else HIP_TRY(hipEventSynchronize(e->adam_ev[hb]));
        if (need > e->adam_host_cap[hb]) {
            if (e->adam_host[hb]) HIP_TRY(hipHostFree(e->adam_host[hb]));
            e->adam_host[hb] = nullptr;
            void* q = nullptr;
            HIP_TRY(hipHostMalloc(&q, e->adam_cap * sizeof(float), hipHostMallocDefault));
            e->adam_host[hb] = (float*)q; e->adam_host_cap[hb] = e->adam_cap;
        }
        float* tab = e->adam_host[hb];
        for (int s = 0; s < r->n_steps; ++s) {
            const double step = (double)(r->adam_step0 + s + 1);
            const double bc1 = 1.0 - std::pow(r->beta1, step);
            const double bc2 = 1.0 - std::pow(r->beta2, step);
            tab[2 * s] = (float)(-(r->lr / bc1));         // addcdiv_'s value = -step_size, a python double rounded to fp32 once
            tab[2 * s + 1] = (float)std::sqrt(bc2);              // bias_correction2_sqrt, likewise
        }
        HIP_TRY(hipMemcpyAsync(e->adam_coef, tab, need * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(e->adam_ev[hb], stream));
        if (r->adam_step0 == 0)
            for (int l = 0; l < e->L; ++l) {
                HIP_TRY(hipMemsetAsync(e->m[l], 0, (size_t)e->Bpad * e->npad[l] * 4, stream));
                HIP_TRY(hipMemsetAsync(e->v[l], 0, (size_t)e->Bpad * e->npad[l] * 4, stream));
            }
    }
    const size_t erows = r->energy_mode == MCPC_ENERGY_ALL ? (size_t)r->T : 1, eslots = energy_slots(*e);
    if (r->energy_mode != MCPC_ENERGY_NONE && erows > e->epart_rows) {
        // geometric growth: a caller whose T creeps up call by call re-allocates O(log T) times, not every call
        const size_t cap = std::max(erows, e->epart_rows + e->epart_rows / 2);
        if (const int rc = regrow(e, e->epart, cap * eslots * (kMaxLatent + 1), stream)) return rc;
        // (the slots of a 16-chain unit that is all padding are never written: they must read as zero)
        HIP_TRY(hipMemsetAsync(e->epart, 0, cap * eslots * (kMaxLatent + 1) * sizeof(double), stream));
        e->epart_rows = cap;
    }
    launch_mu1(e, e->inputs, e->mu1, e->d.batch, e->Bpad, stream);           // constant during the run: weights only change between runs
    // layer-wise kernels: f(x_l) of the state the run starts from (the backward launches keep it current from there)
    if (e->lw) launch_lw_act(e, stream);
    if (run_accumulates) { const int rc = ensure_spill(e, stream); if (rc) return rc; }
    if (r->acc_reset && run_accumulates) {
        const int nlin = e->L + (e->has_head ? 1 : 0);
        for (int j = 0; j < nlin; ++j) {
            HIP_TRY(hipMemsetAsync(e->lin[j].G, 0, (size_t)e->lin[j].out_pad * e->lin[j].g_ld * 4, stream));
            HIP_TRY(hipMemsetAsync(e->lin[j].Gb, 0, (size_t)e->lin[j].out_pad * 4, stream));
        }
        HIP_TRY(hipMemsetAsync(e->e0sum, 0, (size_t)e->Bpad * e->npad[0] * 4, stream));
    }
    return 0;
}

// The kernel parameters of a run on the kernel form whose plan is `sp`: everything but the launch window (set_window) and the spill
// pointers of a Hebbian segment.
KParams run_params(const mcpc_engine* e, const mcpc_run_desc* r, const StepPlan& sp) {
    KParams P{};
    const int nlin = e->L + (e->has_head ? 1 : 0);
    for (int l = 0; l < e->L; ++l) {
        KLayer& K = P.layer[l];
        K.x = e->x[l]; K.m = e->m[l]; K.v = e->v[l];
        K.xgrad = r->update_x ? nullptr : r->xgrad[l];
        K.rec = r->rec_count > 0 ? r->rec_x[l] : nullptr;
        K.spill_e = l == 0 ? e->e0sum : e->spill_e[l];
        K.spill_a = e->spill_a[l];
        K.spill_e_tm = (l >= 1 && e->lin[l].spill_tm) ? 1 : 0;               // E_l is the error operand of Linear l,
        K.spill_a_tm = (l + 1 < nlin && e->lin[l + 1].spill_tm) ? 1 : 0;      // f(x_l) the activation operand of Linear l + 1
        K.ext_noise = nullptr;
        if (l >= 1) {
            K.Wf = (const f32x4*)e->lin[l].Wf; K.Wb = (const f32x4*)e->lin[l].Wb; K.bias = e->lin[l].bias_pad;
        }
        K.n = e->d.sizes[l]; K.npad = e->npad[l]; K.ntiles = e->npad[l] / 16;
        K.act = e->d.acts[l]; K.ecoef = e->d.ecoef[l];
        K.lds_a = sp.lds_a[l]; K.lds_e = sp.lds_e[l]; K.ld = e->npad[l] + kLdPad;
        K.lds_x = sp.lds_x[l]; K.lds_bias = sp.lds_bias[l];
    }
    if (e->has_head) {
        KHead& H = P.head;
        const Lin& ln = e->lin[e->L];
        H.Wf = (const f32x4*)ln.Wf; H.Wb = (const f32x4*)ln.Wb; H.bias = ln.bias_pad;
        H.ybits = e->ybits; H.y_binary = e->knobs.no_ybits ? e->y_binary + 1 : e->y_binary; H.y_bounded = e->y_binary + 2; H.ywords = e->ywords;
        H.y = e->ypad; H.ytile = e->ytile; H.rec_out = r->rec_count > 0 ? r->rec_out : nullptr; H.spill_e = e->spill_eo;
        H.spill_tm = e->lin[e->L].spill_tm ? 1 : 0;
        H.n = e->d.n_out; H.npad = e->out_pad; H.ntiles = e->out_pad / 16;
        H.loss_kind = r->loss_kind;
        H.inv_var = r->loss_kind == MCPC_LOSS_GAUSSIAN ? (float)(1.0 / r->loss_var) : 1.0f;
        H.mask_start = r->loss_kind == MCPC_LOSS_NONE ? 0 : r->mask_start;
        H.lds_eo = sp.lds_eo; H.ld = sp.head_ld;
        H.lds_bias = sp.lds_hbias; H.lds_yw = sp.lds_yw;
    }
    P.mu1 = e->mu1; P.epart = e->epart; P.epart_slots = (int)energy_slots(*e);
    P.phases = sp.dev; P.n_phases = sp.n_phases; P.wexp = e->wexp; P.spillmax = nullptr; P.lds_spillmax = sp.lds_spillmax; P.lds_rowexp = sp.lds_rowexp; P.g_first = sp.g_first;
    P.stagger_cycles = e->knobs.stagger;
    P.L = e->L; P.has_head = e->has_head; P.B = e->d.batch; P.Bpad = e->Bpad; P.T = r->T;
    P.xopt = r->xopt_kind; P.update_x = r->update_x ? 1 : 0;
    P.lr = (float)r->lr; P.beta2 = (float)r->beta2;
    P.omb1 = (float)(1.0 - r->beta1); P.omb2 = (float)(1.0 - r->beta2); P.eps = (float)r->eps;
    P.noise_mode = r->update_x ? r->noise_mode : MCPC_NOISE_NONE;
    P.noise_scale = (float)std::sqrt(r->noise_var * r->lr);
    P.seed = r->seed; P.step_base = r->step_base; P.chain_base = r->chain_base;
    P.acc_begin = std::max(r->acc_begin, 0); P.acc_end = std::min(r->acc_end, r->T);
    P.energy_mode = r->energy_mode;
    P.rec_begin = r->rec_begin; P.rec_stride = std::max(r->rec_stride, 1); P.rec_count = r->rec_count;
    P.lds_red = sp.lds_red;
    P.lds_ws_sync = sp.lds_ws_sync;
    P.ws_prio = e->knobs.ws_prio;
    P.lean_ok = lean_ok(*e);
    P.err = e->err; P.dummy = e->dummy; P.lds_floats = sp.lds_bytes / 4; P.lds_zero = sp.lds_zero;
    P.clk = e->profiling ? e->clk : nullptr;
    P.xl = sp.xl ? 1 : 0;
    P.spill_sys = e->slot_bytes > ((size_t)8 << 20) ? 1 : 0;      // beyond 8 MB (a quarter of the eight 4 MB L2s) the spill stores go out at system scope
    return P;
}

// Which instantiation of the in-place kernel a launch of this run takes (mcpc_step_forms.h: Ws2Spec).  A specialised mode fixes at compile
// time what the generic kernel decides per workgroup from KParams, so it is chosen only when EVERY workgroup of the launch decides
// that way -- the tests below are the body's own (mcpc_steps_ws2_body.inc: upd_mode, lean, xl, rowexp, ybin, y_bounded, slot), on the
// host's copies of the same values.  What differs per lane (the padding chains of a last unit: LeanLane::livem) is data, not mode.
//   lean for every workgroup: only units that hold a chain of the batch are launched (nwg_live; the round schedule deals those units)
// ws2_spec_candidate: what holds for every launch of a run, whatever the bound target is.
bool ws2_spec_candidate(const mcpc_engine* e, const KParams& P) {
#ifdef MCPC_EXP_NOLEAN
    return false;
#endif
    if (!e->y_flags_host || e->ws != 2 || e->lw) return false;                                                        // (tuning spec=0, another kernel form: never allocated)
    const bool kick = P.update_x && P.xopt == MCPC_XOPT_SGD && P.noise_mode == MCPC_NOISE_PHILOX;                     // UPD: lean SGD + Philox kick,
    const bool map = P.update_x && P.xopt == MCPC_XOPT_ADAM && P.noise_mode == MCPC_NOISE_NONE;                       // or lean Adam (the MAP warm-up)
    if (!kick && !map) return false;
    if (!P.lean_ok || !P.xl) return false;                                                                            // lean, XL (and with them ROWEXP)
    for (int l = 0; l < e->L; ++l)
        if (P.layer[l].act != MCPC_ACT_RELU) return false;                                                            // ACT
    return P.has_head && P.head.loss_kind == MCPC_LOSS_BERNOULLI && e->target_bound;                                  // HEAD, as far as the run descriptor tells
}

// HEAD needs what only the device knows when mcpc_bind_target returns: that the target is 0/1 everywhere and bounded.  The bind copies the
// three flag words to pinned host memory behind its kernels; a candidate run asks here, once.  `hot` comes back true when the words
// have landed and say so.  A run of at least `spec_wait` steps (default 0: every candidate run) WAITS for the copy (hipEventSynchronize on the bind's event: the host
// blocks until the stream has executed the bind, the GPU then idles for one launch latency -- with a target bound in front of every
// call, calls of 4 to 1000 steps end 3-7 % sooner than on the parent, and no sooner than on it without the wait, because the copy has never
// landed when the next run is queued: profiles/spec_modes.txt section 7); a shorter run only looks (hipEventQuery) and keeps the generic
// kernel while the copy is still on its way.
int target_flags_on_host(mcpc_engine* e, const KParams& P, int run_steps, bool& hot) {
    hot = false;
    if (e->y_flags_pending) {
        if (run_steps >= e->knobs.spec_wait) {
            HIP_TRY(hipEventSynchronize(e->y_flags_ev));
        } else {
            const hipError_t q = hipEventQuery(e->y_flags_ev);
            if (q == hipErrorNotReady) return 0;
            HIP_TRY(q);
        }
        e->y_flags_pending = false;
    }
    const int* const yf = e->y_flags_host;       // [0] 0/1 everywhere, [1] never set (tuning no_ybits reads it), [2] inside [-1, 2]
    hot = yf[P.head.y_binary - e->y_binary] != 0 && yf[2] != 0;
    return 0;
}

// `hot`: the run is a candidate and its target's flags hold.  `accumulating`: mcpc_run cuts its launches at the accumulation window, so
// every step of a launch lies on one side of it.  `mix`: a launch of the round schedule.
int ws2_select_mode(const KParams& P, bool hot, bool accumulating, bool mix) {
    if (!hot) return WS2_SPEC_GENERIC;
    const bool map = P.xopt == MCPC_XOPT_ADAM;
    if (map && accumulating) return WS2_SPEC_GENERIC;
    if (accumulating && !P.spill_sys) return WS2_SPEC_GENERIC;                       // (a spill that stays in the L2: no instantiation of its own)
    const int spec = map ? WS2_SPEC_MAP : !accumulating ? WS2_SPEC_HOT : WS2_SPEC_HOT_SPILL;          // SPILL
    return ws2_spec_built(spec, mix) ? spec : WS2_SPEC_GENERIC;
}

#ifdef MCPC_STAMPS
// diagnostic build: where the waves of the launch that just ran steps [t, t + n) spent their cycles (waits for the stream)
int report_stamps(mcpc_engine* e, bool use_u, int t, int n, hipStream_t stream) {
    static const char* names_ws2[16] = {"G top", "G wait deps", "G HEADB gemm", "G gemm", "G prefetch next", "G store+publish",
                                        "(launch, s_memtime)", "(launch, 100 MHz)", "E other", "E loads", "E wait block", "E epilogue FWD", "E epilogue HEADF", "E epilogue BWD", "-", "-"};
    static const char* names[16] = {"FWD prologue", "FWD gemm", "FWD epilogue", "HEADF prologue", "HEADF gemm", "HEADF epilogue",
                                    "HEADB prologue", "HEADB gemm", "HEADB (acc->b)", "BWD prologue", "BWD gemm", "BWD epilogue",
                                    "energy", "barrier", "-", "-"};
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<unsigned long long> h((size_t)e->nwg * e->nw * 16);
    HIP_TRY(hipMemcpy(h.data(), e->dbg, h.size() * 8, hipMemcpyDeviceToHost));
#ifdef MCPC_STAMPS_ENTRY
    // per table entry: mean / max over the G (q = 1, 2) or E (q = 3, 4) waves, cycles per step
    static const char* what[5] = {"", "G wait (deps)", "G total", "E wait for block", "E total"};
    static const char* tname[5] = {"FWD", "HEADF", "HEADB", "BWD", "ENERGY"};
    const std::vector<KPhase>& tab = e->main.table;
    const bool want_g = MCPC_STAMPS_ENTRY <= 2;
    fprintf(stderr, "[stamps] launch t0=%d n=%d: %s per table entry, cycles per step (mean / max over the %s waves)\n", t, n,
            what[MCPC_STAMPS_ENTRY], want_g ? "G" : "E");
    double tot = 0;
    for (int i = 0; i < 16 && i < e->main.n_phases; ++i) {
        double sum = 0, mx = 0; size_t cnt = 0;
        for (size_t w = 0; w < (size_t)e->nwg * e->nw; ++w) {
            const bool is_g = (int)(w % e->nw) < e->nw / 2;
            if (is_g != want_g) continue;
            const double v = (double)h[w * 16 + i];
            sum += v; mx = std::max(mx, v); ++cnt;
        }
        tot += sum / cnt / n;
        fprintf(stderr, "[stamps]   entry %2d %-6s layer %d tiles %2d nkb %2d  mean %8.0f  max %8.0f\n", i, tname[tab[i].type], tab[i].layer,
                tab[i].ntiles, tab[i].nkb, sum / cnt / n, mx / n);
    }
    fprintf(stderr, "[stamps]   sum over entries: %.0f cycles per step\n", tot);
#else
    double tot = 0, sum[16] = {0}, mx[16] = {0};
    for (size_t w = 0; w < (size_t)e->nwg * e->nw; ++w)
        for (int i = 0; i < 16; ++i) { sum[i] += (double)h[w * 16 + i]; mx[i] = std::max(mx[i], (double)h[w * 16 + i]); }
    static const char* names_u[16] = {"top of entry", "barrier", "gemm", "prefetch next", "epilogue", "-", "-", "presplit", "gemm fwd nt=1", "gemm fwd nt=2", "gemm fwd nt=3", "gemm fwd nt=4", "gemm bwd nt=1", "gemm bwd nt=2", "gemm bwd nt=3", "gemm bwd nt=4"};
    if (e->ws == 2 && !use_u) {
        fprintf(stderr, "[stamps] shader clock during the launch = %.3f GHz (s_memtime ticks per 100 MHz wall-clock tick)\n", sum[6] / sum[7] * 0.1);
        sum[6] = sum[7] = 0;
    }
    for (int i = 0; i < 16; ++i) tot += sum[i];
    fprintf(stderr, "[stamps] launch t0=%d n=%d: mean cycles/step/wave = %.0f\n", t, n, tot / (e->nwg * e->nw) / n);
    for (int i = 0; i < 16; ++i)
        fprintf(stderr, "[stamps]   %-18s %5.1f%%  mean %8.0f  max %8.0f cycles/step\n", (use_u ? names_u : e->ws == 2 ? names_ws2 : names)[i], 100.0 * sum[i] / tot,
                sum[i] / (e->nwg * e->nw) / n, mx[i] / n);
#endif
    return 0;
}
#endif

// What the executor of a run (mcpc_run) carries from launch to launch
struct RunCtx {
    mcpc_engine* e;
    const mcpc_run_desc* r;
    hipStream_t stream;
    const StepPlan& sp;             // the plan of the kernel form that serves the run
    bool use_u;                     // ... the unified-wave kernel's
    bool hot = false;               // the in-place kernel may take a specialised instantiation (ws2_spec_candidate, target_flags_on_host)
    bool bracket_open = false;
    // mcpc_last_step_kernel_name: which forms this run launched (bit 0 plain launch, bit 1 round schedule)
    unsigned launched = 0;
    unsigned specs_rr = 0, specs_plain = 0;               // ... and which instantiations of the in-place kernel (bit = Ws2Spec)
};

// HIP events around every launch of the step kernel (at most kMaxProfBrackets since profiling was switched on: a caller that
// leaves it on forever stops collecting, it does not accumulate HIP events without bound)
constexpr size_t kMaxProfBrackets = 1 << 16;
int prof_begin(RunCtx& c) {
    mcpc_engine* e = c.e;
    c.bracket_open = false;
    if (!e->profiling) return 0;
    if (e->events_used >= kMaxProfBrackets) return 0;
    c.bracket_open = true;
    if (e->events_used == e->events.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(MCPC_EHIP, "hipEventCreate failed");
        e->events.emplace_back(a, b);
    }
    return hipEventRecord(e->events[e->events_used].first, c.stream) == hipSuccess ? 0 : fail(MCPC_EHIP, "hipEventRecord failed");
}
int prof_end(RunCtx& c, double steps) {
    mcpc_engine* e = c.e;
    if (!e->profiling || !c.bracket_open) return 0;
    if (hipEventRecord(e->events[e->events_used].second, c.stream) != hipSuccess) return fail(MCPC_EHIP, "hipEventRecord failed");
    ++e->events_used; e->prof_steps += steps;
    return 0;
}

// one launch of the in-place kernel, on the instantiation ws2_select_mode picks for it
int run_ws2(RunCtx& c, KParams& K, bool mix, int nblocks, bool accumulating) {
    const int spec = ws2_select_mode(K, c.hot, accumulating, mix);
    (mix ? c.specs_rr : c.specs_plain) |= 1u << spec;
    return launch_ws2(spec, mix, nblocks, c.sp.lds_bytes, K, c.stream);
}

// one cycle of the round schedule (plan_rounds): rr_k launches of q steps, every unit in rr_m of them; afterwards every
// unit is at t0 + rr_m q.  `base` carries the spill pointers of the ring part in a Hebbian segment.
int run_round_cycle(RunCtx& c, const KParams& base, int t0, int q, bool accumulating) {
    mcpc_engine* e = c.e;
    c.launched |= 2u;
    KParams Q = base;
    set_window(e, c.r, Q, t0, q);
    Q.spill_t0 = t0; Q.rr_q = q;
    for (int i = 0; i < e->rr_k; ++i) {
        Q.wg_list = e->rr_tab + e->rr_off[i]; Q.wg_rel = Q.wg_list + e->rr_count[i];
        if (const int rc = prof_begin(c)) return rc;
        if (c.use_u) launch_u(true, e->rr_count[i], c.sp.lds_bytes, Q, c.stream);
        else if (const int rc = run_ws2(c, Q, true, e->rr_count[i], accumulating)) return rc;
        if (const int rc = prof_end(c, (double)q * e->rr_count[i] / e->nwg_live)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// one plain launch of steps [t0, t0 + n) on the form that serves the run; `P` holds the launch window
int run_plain(RunCtx& c, KParams& P, int t0, int n, bool accumulating) {
    mcpc_engine* e = c.e;
    if (const int rc = prof_begin(c)) return rc;
    c.launched |= 1u;
    if (e->lw) { if (const int rc = launch_lw_steps(e, c.r, P, t0, n, c.stream)) return rc; }
    else if (c.use_u) launch_u(false, e->nwg_live, c.sp.lds_bytes, P, c.stream);
    else if (e->ws == 2) { if (const int rc = run_ws2(c, P, false, e->nwg_live, accumulating)) return rc; }
    else launch_barrier(e->nwg, c.sp.lds_bytes, P, c.stream);
    return prof_end(c, (double)n);
}

// mcpc_last_step_kernel_name of the run
std::string last_step_name(const RunCtx& c) {
    // (a run on the generic instantiation alone reads as it always did; specialised launches are named behind the form they belong to)
    auto spec_tag = [](unsigned specs) -> std::string {
        if (!(specs & ~(1u << WS2_SPEC_GENERIC))) return "";
        std::string tag;
        for (int i = 0; i < WS2_SPEC_COUNT; ++i)
            if (specs & (1u << i)) tag += (tag.empty() ? "" : ", ") + std::string(ws2_spec_tag(i));
        return " [mcpc_steps_ws2_spec_kernel: " + tag + "]";
    };
    std::string name;
    if (c.launched & 2u) name = (c.use_u ? c.e->u_rr_name : c.e->rr_name) + spec_tag(c.specs_rr);
    if (c.launched & 1u) {
        if (!name.empty()) name += " + ";
        name += plain_kernel_name(*c.e, c.use_u) + spec_tag(c.specs_plain);
    }
    return name;
}

}  // namespace

extern "C" {

int mcpc_run(mcpc_engine* e, const mcpc_run_desc* r, void* stream_) {
    if (!e || !r) return fail(MCPC_EINVAL, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(e->d.device));
    if (const int rc = check_run(e, r)) return rc;
    if (!e->retired.empty()) free_completed_retired(e);
    // the schedule (mcpc_plan.h: no device work), then what it needs on the device
    RunPlan& plan = e->run_plan;
    plan_run(*e, *r, MCPC_STAMPS_BUILD != 0, plan);
    const bool run_accumulates = plan.accumulates, overlap = plan.overlap;
    if (const int rc = prepare_run(e, r, run_accumulates, stream)) return rc;
    const size_t eslots = energy_slots(*e);
    const int end = r->t_begin + r->n_steps;
    RunCtx c{e, r, stream, plan.unified ? e->u.plan : e->main, plan.unified};
    KParams P = run_params(e, r, c.sp);
#ifdef MCPC_STAMPS
    if (!e->dbg) { int rc = dmalloc(e->dbg, (size_t)e->nwg * 2 * kMaxWaves * 16); if (rc) return rc; }
    P.dbg = e->dbg;
#endif
    // (a run on the unified-wave kernel never asks: no wait, no query)
    if (!c.use_u && ws2_spec_candidate(e, P))
        if (const int rc = target_flags_on_host(e, P, r->n_steps, c.hot)) return rc;

    // ---- the plan's items, in order: a plain launch or a cycle of the round schedule each; one inside the accumulation window
    //      spills into its part of the ring and is followed by that part's Hebbian flush -----------------------------------
    for (const RunItem& it : plan.items) {
        set_window(e, r, P, it.t0, it.n);
        P.spill_t0 = it.t0;
        if (it.acc) {
            for (int l = 0; l < e->L; ++l) {
                const size_t off = (size_t)it.slot0 * e->Bpad * e->npad[l];
                P.layer[l].spill_a = e->spill_a[l] + off;
                if (l >= 1) P.layer[l].spill_e = e->spill_e[l] + off;
            }
            if (e->has_head) P.head.spill_e = e->spill_eo + (size_t)it.slot0 * e->Bpad * e->out_pad;
            // this part of the ring may still be read by the flush that was started n_parts segments ago
            if (overlap && e->flush_pending[it.part]) { HIP_TRY(hipStreamWaitEvent(stream, e->ev_flush[it.part], 0)); e->flush_pending[it.part] = false; }
            // the segment's largest |value| per spilled tensor: starts at zero, raised by the step kernel's workgroups, read by the flush
            P.spillmax = e->spillmax + (size_t)it.part * kSpillTensors;
            HIP_TRY(hipMemsetAsync(P.spillmax, 0, kSpillTensors * sizeof(unsigned), stream));
        } else {
            P.spillmax = nullptr;
        }
        if (const int rc = it.q >= 1 ? run_round_cycle(c, P, it.t0, it.q, it.acc) : run_plain(c, P, it.t0, it.n, it.acc)) return rc;
        HIP_TRY(hipGetLastError());
#ifdef MCPC_STAMPS
        if (const int rc = report_stamps(e, c.use_u, it.t0, it.n, stream)) return rc;
#endif
        if (it.acc && overlap) {
            // the Hebbian GEMMs of this part run on the low-priority stream while the next segment steps
            HIP_TRY(hipEventRecord(e->ev_steps[it.part], stream));
            HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_steps[it.part], 0));
            if (const int rc = flush_spill(e, plan.flushes[it.flush], it.slot0, e->aux, it.part)) return rc;
            HIP_TRY(hipEventRecord(e->ev_flush[it.part], e->aux));
            e->flush_pending[it.part] = true;
        } else if (it.acc) {
            if (const int rc = flush_spill(e, plan.flushes[it.flush], 0, stream, 0)) return rc;
        }
    }
    e->last_step = last_step_name(c);
    // everything that follows on the caller's stream (dw0, gradient read-out, the next run) sees finished sums
    for (int h = 0; h < kMaxRingParts; ++h)
        if (overlap && e->flush_pending[h]) { HIP_TRY(hipStreamWaitEvent(stream, e->ev_flush[h], 0)); e->flush_pending[h] = false; }
    if (run_accumulates) {
        // Linear 0 sees a constant input: fold sum_t e_1 now, then clear the running sum
        Lin& l0 = e->lin[0];
        // one block per (unit, input column | bias): a fixed-order tree over the chains
        hipLaunchKernelGGL(mcpc_dw0_kernel, dim3(l0.n_out, e->inputs != nullptr ? l0.n_in + 1 : 1), dim3(256), 0, stream, e->e0sum,
                           e->inputs, l0.G, l0.Gb, e->d.batch, l0.n_out, e->npad[0], l0.n_in, l0.g_ld);
        HIP_TRY(hipMemsetAsync(e->e0sum, 0, (size_t)e->Bpad * e->npad[0] * 4, stream));
    }
    if (r->energy_mode == MCPC_ENERGY_ALL) {
        hipLaunchKernelGGL(mcpc_energy_reduce_kernel, dim3((r->n_steps + 3) / 4), dim3(256), 0, stream,
                           e->epart + (size_t)r->t_begin * eslots * (kMaxLatent + 1),
                           r->energies_out + (size_t)r->t_begin * kEnergyCols, r->n_steps, (int)eslots, e->L);
    } else if (r->energy_mode == MCPC_ENERGY_LAST && end == r->T) {
        hipLaunchKernelGGL(mcpc_energy_reduce_kernel, dim3(1), dim3(256), 0, stream, e->epart, r->energies_out, 1, (int)eslots, e->L);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

}  // extern "C"
