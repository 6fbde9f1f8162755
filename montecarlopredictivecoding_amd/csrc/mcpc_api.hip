// Host side of libmcpc.so: the C ABI declared in include/mcpc.h, in four translation units.
//   mcpc_api.hip (this one)   the engine's life cycle and bindings, mcpc_run and its executor with every step kernel, the three evaluators
//                             that share kernels and scratch with the runs, RCCL, the normals, the query, debug and profiling entries
//   mcpc_flush.hip            the Hebbian flush of the Linears j >= 1 (flush_spill) and its kernels
//   mcpc_records.hip          the stateless reducers over recorded states (int device, no engine) and their kernels
//   mcpc_build_info.hip       mcpc_abi_version, mcpc_build_info: the one unit that is compiled with the provenance defines
// Allocation, weight packing, launch orchestration (step segments + Hebbian flushes); no torch.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is loaded with dlopen on first use (no link dependency)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "mcpc_build.h"
#include "mcpc_engine.h"
// every kernel this unit launches: the barrier step kernel and the small kernels, the in-place, unified-wave and layer-wise step
// kernels, the evaluators
#include "mcpc_kernels.h"
#include "mcpc_steps_ws2.h"
#include "mcpc_steps_u.h"
#include "mcpc_steps_lw.h"
#include "mcpc_chain_energy.h"
#include "mcpc_pred_err.h"
#include "mcpc_ancestral.h"

using namespace mcpc;

namespace {

// RCCL, bound at first use: a host that never shards the chains never loads it; inside a torch process dlopen returns the copy
// torch already mapped (same soname), so both share one HIP runtime.
struct Rccl {
    void* so = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.so) return MCPC_OK;
    void* so = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!so) so = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!so) return fail(MCPC_EHIP, "librccl.so.1 could not be loaded: %s", dlerror());
    Rccl r;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(so, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(so, "ncclCommInitRank");
    r.AllReduce = (decltype(r.AllReduce))dlsym(so, "ncclAllReduce");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(so, "ncclCommDestroy");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(so, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.CommDestroy || !r.GetErrorString) {
        dlclose(so);
        return fail(MCPC_EHIP, "librccl.so.1 lacks an entry point this library needs");
    }
    r.so = so;
    g_rccl = r;
    return MCPC_OK;
}

int free_all(mcpc_engine* e) {
    if (e->comm && g_rccl.CommDestroy) { (void)g_rccl.CommDestroy(e->comm); e->comm = nullptr; e->comm_ranks = 0; }
    auto F = [](auto*& p) { if (p) { (void)hipFree((void*)p); p = nullptr; } };
    for (int l = 0; l < kMaxLatent; ++l) { F(e->x[l]); F(e->m[l]); F(e->v[l]); F(e->spill_a[l]); F(e->spill_e[l]); }
    F(e->e0sum); F(e->mu1); F(e->ypad); F(e->ytile); F(e->ybits); F(e->y_binary); F(e->spill_eo); F(e->slab); F(e->epart); F(e->adam_coef); F(e->main.dev); F(e->err); F(e->wexp); F(e->spillmax); F(e->clk); F(e->dummy); F(e->u.plan.dev);
    for (int l = 0; l < kMaxLatent; ++l) { F(e->lw_fx[l]); F(e->lw_err[l]); }
    F(e->lw_err_o); F(e->lw_jobs);
    for (int l = 0; l < kMaxLatent; ++l) { F(e->ce_x[l]); F(e->ce_fx[l]); }
    F(e->ce_mu1); F(e->ce_part); F(e->ce_jobs); F(e->pe_jobs);
    for (auto& ln : e->lin) { F(ln.Wf); F(ln.Wb); F(ln.bias_pad); F(ln.G); F(ln.Gb); }
    for (auto& ev : e->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (int h = 0; h < kMaxRingParts; ++h) { if (e->ev_steps[h]) (void)hipEventDestroy(e->ev_steps[h]); if (e->ev_flush[h]) (void)hipEventDestroy(e->ev_flush[h]); e->ev_steps[h] = e->ev_flush[h] = nullptr; }
    if (e->aux) { (void)hipStreamDestroy(e->aux); e->aux = nullptr; }
    if (e->aux3) { (void)hipStreamDestroy(e->aux3); e->aux3 = nullptr; }
    if (e->spacer) { (void)hipStreamDestroy(e->spacer); e->spacer = nullptr; }
    if (e->ev_fork) { (void)hipEventDestroy(e->ev_fork); e->ev_fork = nullptr; }
    if (e->ev_join) { (void)hipEventDestroy(e->ev_join); e->ev_join = nullptr; }
    if (e->y_flags_ev) { (void)hipEventDestroy(e->y_flags_ev); e->y_flags_ev = nullptr; }
    if (e->y_flags_host) { (void)hipHostFree(e->y_flags_host); e->y_flags_host = nullptr; }
    F(e->rr_tab);
    for (auto& q : e->retired) { (void)hipFree(q.p); if (q.ev) (void)hipEventDestroy(q.ev); }
    e->retired.clear();
    for (int i = 0; i < 2; ++i) {
        if (e->adam_host[i]) { (void)hipHostFree(e->adam_host[i]); e->adam_host[i] = nullptr; }
        if (e->adam_ev[i]) { (void)hipEventDestroy(e->adam_ev[i]); e->adam_ev[i] = nullptr; }
    }
    e->events.clear();
    return 0;
}

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

// A buffer that launches already in the stream may still use is not freed but retired behind an event.
void retire(mcpc_engine* e, void* p, hipStream_t stream) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, stream) != hipSuccess) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;                                  // no event: the buffer waits for mcpc_destroy
    }
    e->retired.push_back({p, ev});
}
// The engine gives a buffer up (retired if there is one, the pointer cleared), and replaces it by one of `count` elements: nothing waits
template <typename T>
void give_up(mcpc_engine* e, T*& p, hipStream_t stream) { if (p) retire(e, (void*)p, stream); p = nullptr; }
template <typename T>
int regrow(mcpc_engine* e, T*& p, size_t count, hipStream_t stream) { give_up(e, p, stream); return dmalloc(p, count); }
// A retired buffer is freed by a later run once its event has completed (never under a kernel that uses it)
void free_completed_retired(mcpc_engine* e) {
    size_t keep = 0;
    for (size_t i = 0; i < e->retired.size(); ++i) {
        auto& q = e->retired[i];
        if (q.ev && hipEventQuery(q.ev) == hipSuccess) { (void)hipFree(q.p); (void)hipEventDestroy(q.ev); }
        else e->retired[keep++] = q;
    }
    e->retired.resize(keep);
    (void)hipGetLastError();                           // hipEventQuery's hipErrorNotReady is not an error of this run
}
#ifdef MCPC_STAMPS
void print_u_table(const StepPlan& u) {
    static const char* tn[6] = {"FWD", "HEADF", "HEADB", "BWD", "ENERGY", "NOP"};
    for (int w = 0; w < kUWaves; ++w) {
        fprintf(stderr, "[u-table] wave %d:", w);
        for (int i = 0; i < u.n_phases; ++i) {
            const KPhase& k = u.table[(size_t)w * u.n_phases + i];
            fprintf(stderr, " %s%s(l%d t%d+%d kb%d)", (k.flags & PHF_SYNC) ? "|" : "", tn[k.type], k.layer, k.tile0, k.ntiles, (k.flags & PHF_WS_GEMM) ? k.nkb : 0);
        }
        fprintf(stderr, "\n");
    }
}
#endif

// A table the planner built, copied to the device
template <typename T>
int upload(T*& dev, const std::vector<T>& host, const char* what) {
    if (const int rc = dmalloc(dev, host.size())) return rc;
    if (hipMemcpy(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return fail(MCPC_EHIP, "hipMemcpy of %s failed", what);
    return 0;
}

// A step table, bound to the packed weights and uploaded: a GEMM over Linear a_lin reads its forward image in FWD / HEADF entries (the
// Linear predicts the entry's units) and its backward image in HEADB / BWD entries (the error is projected back through it).
int upload_table(mcpc_engine* e, StepPlan& p) {
    for (KPhase& k : p.table)
        if (k.a_lin >= 1) k.A = (k.type == PH_FWD || k.type == PH_HEADF) ? e->lin[k.a_lin].Wf : e->lin[k.a_lin].Wb;
    return upload(p.dev, p.table, "the phase table");
}

// The round schedule's tables, and its form of the in-place kernel
hipError_t allow_lds(const void* fn, int bytes) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }
int upload_rounds(mcpc_engine* e) {
    if (const int rc = upload(e->rr_tab, e->rr_host, "the round-schedule tables")) return rc;
    for (const Ws2SpecEntry& sp : kWs2Specs)
        if (sp.fn[1] && allow_lds(sp.fn[1], e->main.lds_bytes) != hipSuccess) return fail(MCPC_EHIP, "hipFuncSetAttribute failed for the round schedule");
    return 0;
}

// A launch window of a run: steps [t0, t0 + n), and the rows of the run's per-step tables (Adam coefficients, injected noise) it starts at
void set_window(const mcpc_engine* e, const mcpc_run_desc* r, KParams& P, int t0, int n) {
    P.t0 = t0; P.n_steps = n;
    const size_t s0 = (size_t)(t0 - r->t_begin);
    P.adam_coef = r->xopt_kind == MCPC_XOPT_ADAM ? e->adam_coef + 2 * s0 : nullptr;
    if (r->noise_mode == MCPC_NOISE_EXTERNAL)
        for (int l = 0; l < e->L; ++l) P.layer[l].ext_noise = r->ext_noise[l] + s0 * e->d.batch * e->d.sizes[l];
}

// mu_1 = inputs W0^T + b0 into `dst` [Bpad][npad_0]: one kernel for the runs and the evaluators, so that all of them see the same bits
void launch_mu1(const mcpc_engine* e, const float* inputs, float* dst, hipStream_t stream) {
    const Lin& l0 = e->lin[0];
    const size_t total = (size_t)e->Bpad * e->npad[0];
    hipLaunchKernelGGL(mcpc_mu1_kernel, dim3(grid_for(total)), dim3(256), 0, stream, inputs, l0.W, l0.bias, dst,
                       e->d.batch, e->d.n_in, e->d.sizes[0], e->Bpad, e->npad[0]);
}

// steps [t0, t0 + n) of a run on the layer-wise kernels: two launches per step on the caller's stream.  `P` carries the segment's spill
// pointers (spill_t0 = t0); what changes from step to step travels in the launch arguments.
int launch_lw_steps(mcpc_engine* e, const mcpc_run_desc* r, const KParams& P, int t0, int n, hipStream_t stream) {
    LwParams Q{};
    Q.P = P;
    for (int l = 0; l < e->L; ++l) { Q.fx[l] = e->lw_fx[l]; Q.err[l] = e->lw_err[l]; }
    Q.err_o = e->lw_err_o;
    const dim3 gf(e->Bpad / kLwChains, e->lw_nf), gb(e->Bpad / kLwChains, e->lw_nb);
    for (int t = t0; t < t0 + n; ++t) {
        Q.t = t;
        Q.slot = (t >= P.acc_begin && t < P.acc_end) ? t - P.spill_t0 : -1;
        Q.rec_idx = -1;
        if (P.rec_count > 0 && t >= P.rec_begin) {
            const int k = (t - P.rec_begin) / P.rec_stride;
            if (k < P.rec_count && P.rec_begin + k * P.rec_stride == t) Q.rec_idx = k;
        }
        Q.do_energy = (P.energy_mode == MCPC_ENERGY_ALL || (P.energy_mode == MCPC_ENERGY_LAST && t == P.T - 1)) ? 1 : 0;
        Q.erow = P.energy_mode == MCPC_ENERGY_ALL ? t : 0;
        set_window(e, r, Q.P, t, 1);
        Q.jobs = e->lw_jobs;
        hipLaunchKernelGGL(mcpc_lw_fwd_kernel, gf, dim3(kLwThreads), 0, stream, Q);
        Q.jobs = e->lw_jobs + e->lw_nf;
        hipLaunchKernelGGL(mcpc_lw_bwd_kernel, gb, dim3(kLwThreads), 0, stream, Q);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char* mcpc_last_error(void) { return g_err.c_str(); }

int mcpc_create(const mcpc_net_desc* d, mcpc_engine** out) {
    if (!d || !out) return fail(MCPC_EINVAL, "null argument");
    *out = nullptr;
    if (const int rc = check_net_desc(d)) return rc;
    // the device: present, its CU count, and -- only when the descriptor leaves the spill budget to the library -- its memory
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (d->device < 0 || d->device >= ndev) return fail(MCPC_EINVAL, "device %d not present (%d devices)", d->device, ndev);
    HIP_TRY(hipSetDevice(d->device));
    int n_cu = 256;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, d->device) != hipSuccess || n_cu <= 0) n_cu = 256;
    size_t free_b = 0, total_b = 0;
    if (d->spill_budget_bytes <= 0 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;

    // plan (mcpc_plan.h: no device work), then allocate what the plan needs
    mcpc_engine* e = new mcpc_engine();
    e->d = *d;
    e->d.tuning = nullptr;                   // the caller's string is not kept
    int rc = parse_tuning(d->tuning, e->knobs);
    if (!rc) rc = plan_engine(*d, n_cu, total_b, *e);
    if (rc) { delete e; return rc; }
    auto bail = [&](int code) { free_all(e); delete e; return code; };
    auto zeroed = [&](auto*& p, size_t count) -> int {
        if (const int rc2 = dmalloc(p, count)) return rc2;
        return hipMemset(p, 0, count * sizeof(*p)) == hipSuccess ? 0 : fail(MCPC_EHIP, "hipMemset failed");
    };
    for (int l = 0; l < e->L; ++l) {
        const size_t n = (size_t)e->Bpad * e->npad[l];
        if ((rc = zeroed(e->x[l], n)) || (rc = dmalloc(e->m[l], n)) || (rc = dmalloc(e->v[l], n))) return bail(rc);
    }
    if ((rc = zeroed(e->e0sum, (size_t)e->Bpad * e->npad[0])) || (rc = dmalloc(e->mu1, (size_t)e->Bpad * e->npad[0]))) return bail(rc);
    if (e->has_head) {
        if ((rc = zeroed(e->ypad, (size_t)e->Bpad * e->out_pad)) || (rc = dmalloc(e->ytile, (size_t)e->Bpad * e->out_pad))) return bail(rc);
        e->ywords = (e->out_pad + 31) / 32;
        if ((rc = dmalloc(e->ybits, (size_t)e->Bpad * e->ywords)) || (rc = zeroed(e->y_binary, 3))) return bail(rc);   // [1] stays 0; [2]: target in [-1, 2]
        // (only an engine whose lean runs stay on the in-place kernel can take one of its specialised instantiations: ws2_spec_candidate)
        if (e->ws == 2 && !e->lw && !e->u.prefer && e->knobs.spec) {
            if (hipHostMalloc((void**)&e->y_flags_host, 3 * sizeof(int), hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&e->y_flags_ev, hipEventDisableTiming) != hipSuccess)
                return bail(fail(MCPC_EHIP, "pinned copy of the target flags: allocation failed"));
            e->y_flags_host[0] = e->y_flags_host[1] = e->y_flags_host[2] = 0;
        }
    }
    // gradient sums and packed weights of every Linear
    const int nlin = e->L + (e->has_head ? 1 : 0);
    for (int j = 0; j < nlin; ++j) {
        Lin& ln = e->lin[j];
        if ((rc = zeroed(ln.G, (size_t)ln.out_pad * ln.g_ld)) || (rc = zeroed(ln.Gb, (size_t)ln.out_pad))) return bail(rc);
        if (j >= 1) {
            // packed fragments (floats): tiles x k-blocks x kFragBlock 16-byte units, forward and backward
            const size_t pkf = (size_t)(ln.out_pad / 16) * kblocks(ln.in_pad) * kFragBlock * 4;
            const size_t pkb = (size_t)(ln.in_pad / 16) * kblocks(ln.out_pad) * kFragBlock * 4;
            if ((rc = dmalloc(ln.Wf, pkf)) || (rc = dmalloc(ln.Wb, pkb)) || (rc = dmalloc(ln.bias_pad, (size_t)ln.out_pad))) return bail(rc);
        }
    }
    // (the spill ring itself is allocated by the first run that accumulates Hebbian sums: ensure_spill)
    // the form's tables, bound to the weights; the layer-wise kernels' images of f(x_l) and the errors
    if (e->lw) {
        for (int l = 0; l < e->L; ++l) {
            const size_t n = (size_t)e->Bpad * e->npad[l];
            if ((rc = dmalloc(e->lw_fx[l], n))) return bail(rc);
            if (l >= 1 && (rc = dmalloc(e->lw_err[l], n))) return bail(rc);
        }
        if (e->has_head && (rc = dmalloc(e->lw_err_o, (size_t)e->Bpad * e->out_pad))) return bail(rc);
        if ((rc = upload(e->lw_jobs, e->lw_table, "the layer-wise job table"))) return bail(rc);
    } else if ((rc = upload_table(e, e->main))) return bail(rc);
    if (e->u.on && (rc = upload_table(e, e->u.plan))) return bail(rc);
#ifdef MCPC_STAMPS
    if (e->u.on) print_u_table(e->u.plan);
#endif
    if ((rc = zeroed(e->err, 1)) || (rc = zeroed(e->spillmax, (size_t)kMaxRingParts * kSpillTensors)) || (rc = zeroed(e->wexp, kMaxLatent + 1)) ||
        (rc = zeroed(e->clk, 2)) || (rc = zeroed(e->dummy, 1024)))
        return bail(rc);
    // every kernel the engine may launch is allowed its plan's LDS
    const void* kfn = e->ws == 2 ? (const void*)mcpc_steps_ws2_kernel<1> : (const void*)mcpc_steps_kernel<1, 4>;
    hipError_t herr = e->lw ? hipSuccess : allow_lds(kfn, e->main.lds_bytes);
    for (int i = WS2_SPEC_GENERIC + 1; i < WS2_SPEC_COUNT && herr == hipSuccess && e->ws == 2 && !e->lw; ++i)      // (the in-place kernel's specialised instantiations)
        if (kWs2Specs[i].fn[0]) herr = allow_lds(kWs2Specs[i].fn[0], e->main.lds_bytes);
    if (herr != hipSuccess) return bail(fail(MCPC_EHIP, "hipFuncSetAttribute(%d bytes LDS) failed: %s", e->main.lds_bytes, hipGetErrorString(herr)));
    if (e->rr && (rc = upload_rounds(e))) return bail(rc);
    if (e->u.on && (allow_lds((const void*)mcpc_steps_u_kernel<false>, e->u.plan.lds_bytes) != hipSuccess ||
                    allow_lds((const void*)mcpc_steps_u_kernel<true>, e->u.plan.lds_bytes) != hipSuccess))
        return bail(fail(MCPC_EHIP, "hipFuncSetAttribute failed for the unified-wave kernel (%d bytes LDS)", e->u.plan.lds_bytes));
    // The zero fills above are hipMemset on the NULL stream, which the caller's stream does not wait for when it is a non-blocking one
    // (every stream torch creates is): without this wait the first mcpc_params_changed on such a stream can be overtaken by the fill of
    // `wexp`, and the step kernels then read exponent 0 under weights packed with another one
    // (tests/test_gpu_engine.py::test_two_engines_on_two_streams_run_concurrently: E_2 of 1.9e11 for 441).
    if (hipStreamSynchronize(nullptr) != hipSuccess) return bail(fail(MCPC_EHIP, "the zero fills of the engine's buffers failed"));
    *out = e;
    return MCPC_OK;
}

int mcpc_destroy(mcpc_engine* e) {
    if (!e) return MCPC_OK;
    (void)hipSetDevice(e->d.device);
    (void)hipDeviceSynchronize();
    free_all(e);
    delete e;
    return MCPC_OK;
}

int mcpc_bind_params(mcpc_engine* e, int j, const float* W, const float* bias) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    const int nlin = e->L + (e->has_head ? 1 : 0);
    if (j < 0 || j >= nlin) return fail(MCPC_EINVAL, "Linear index %d out of range 0..%d", j, nlin - 1);
    if (!W) return fail(MCPC_EINVAL, "null weight pointer for Linear %d", j);
    e->lin[j].W = W;
    e->lin[j].bias = bias;
    e->lin[j].bound = true;
    return MCPC_OK;
}

int mcpc_params_changed(mcpc_engine* e, void* stream_) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(e->d.device));
    const int nlin = e->L + (e->has_head ? 1 : 0);
    for (int j = 0; j < nlin; ++j)
        if (!e->lin[j].bound) return fail(MCPC_ESTATE, "Linear %d has no bound parameters", j);
    for (int j = 1; j < nlin; ++j) {
        Lin& ln = e->lin[j];
        const size_t total = (size_t)ln.out_pad * ln.in_pad;
        const int grid = std::max(grid_for(total), (ln.out_pad + 255) / 256);
        // the exponent the fp16 planes of this Linear are scaled by (from max |W|), then the planes themselves
        hipLaunchKernelGGL(mcpc_wexp_kernel, dim3(1), dim3(1024), 0, stream, ln.W, (size_t)ln.n_out * ln.n_in, e->wexp + j);
        hipLaunchKernelGGL(mcpc_pack_kernel, dim3(grid), dim3(256), 0, stream, ln.W, ln.bias, ln.Wf, ln.Wb, ln.bias_pad,
                           ln.n_out, ln.n_in, ln.out_pad / 16, ln.in_pad / 16, (const int*)(e->wexp + j));
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_bind_inputs(mcpc_engine* e, const float* inputs, void* /*stream*/) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    e->inputs = inputs;
    return MCPC_OK;
}

int mcpc_bind_target(mcpc_engine* e, const float* target, void* stream_) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    if (!e->has_head) return fail(MCPC_EINVAL, "network has no read-out: no target to bind");
    if (!target) return fail(MCPC_EINVAL, "null target");
    HIP_TRY(hipSetDevice(e->d.device));
    const size_t total = (size_t)e->Bpad * e->out_pad;
    hipLaunchKernelGGL(mcpc_pad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream_, target, e->ypad,
                       e->d.batch, e->d.n_out, e->Bpad, e->out_pad);
    hipLaunchKernelGGL(mcpc_tile_major_kernel, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream_, e->ypad, e->ytile, e->Bpad, e->out_pad);
    // a 0/1 target (the Bernoulli read-out's usual one) is also kept bit-packed; the flag tells the step kernel which to read
    HIP_TRY(hipMemsetAsync(e->y_binary, 0xff, sizeof(int), (hipStream_t)stream_));
    HIP_TRY(hipMemsetAsync(e->y_binary + 2, 0xff, sizeof(int), (hipStream_t)stream_));      // cleared by the first value outside [-1, 2] (headb_fixed_exp)
    hipLaunchKernelGGL(mcpc_pack_target_bits_kernel, dim3(grid_for((size_t)e->Bpad * e->ywords)), dim3(256), 0, (hipStream_t)stream_,
                       e->ypad, e->ybits, e->y_binary, e->Bpad, e->out_pad, e->ywords);
    HIP_TRY(hipGetLastError());
    // what the kernels found goes to the host as well: a run chooses its instantiation of the in-place kernel from it (ws2_select_mode)
    // (engines that can take a specialised instantiation only.  A copy still on its way from an earlier bind is simply followed by this
    // one, in stream order, and the event re-recorded behind it: whoever asks waits for, or looks at, the latest.  No host wait here.)
    if (e->y_flags_host && e->y_flags_ev) {
        HIP_TRY(hipMemcpyAsync(e->y_flags_host, e->y_binary, 3 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream_));
        HIP_TRY(hipEventRecord(e->y_flags_ev, (hipStream_t)stream_));
        e->y_flags_pending = true;
    }
    e->target_bound = true;
    return MCPC_OK;
}

int mcpc_load_state(mcpc_engine* e, const float* const* x, void* stream_) {
    if (!e || !x) return fail(MCPC_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    for (int l = 0; l < e->L; ++l) {
        if (!x[l]) return fail(MCPC_EINVAL, "null state pointer for layer %d", l);
        const size_t total = (size_t)e->Bpad * e->npad[l];
        hipLaunchKernelGGL(mcpc_pad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream_, x[l], e->x[l],
                           e->d.batch, e->d.sizes[l], e->Bpad, e->npad[l]);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_store_state(mcpc_engine* e, float* const* x, void* stream_) {
    if (!e || !x) return fail(MCPC_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    for (int l = 0; l < e->L; ++l) {
        if (!x[l]) return fail(MCPC_EINVAL, "null state pointer for layer %d", l);
        const size_t total = (size_t)e->d.batch * e->d.sizes[l];
        hipLaunchKernelGGL(mcpc_unpad_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream_, e->x[l], x[l],
                           e->d.batch, e->d.sizes[l], e->npad[l]);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_store_adam_state(mcpc_engine* e, float* const* m, float* const* v, void* stream_) {
    if (!e || !m || !v) return fail(MCPC_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    for (int l = 0; l < e->L; ++l) {
        if (!m[l] || !v[l]) return fail(MCPC_EINVAL, "null Adam state pointer for layer %d", l);
        const size_t total = (size_t)e->d.batch * e->d.sizes[l];
        hipLaunchKernelGGL(mcpc_unpad_adam_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream_, e->m[l], m[l],
                           e->d.batch, e->d.sizes[l], e->npad[l]);
        hipLaunchKernelGGL(mcpc_unpad_adam_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream_, e->v[l], v[l],
                           e->d.batch, e->d.sizes[l], e->npad[l]);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

}  // extern "C"

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


}  // namespace

namespace {

// The loss arguments of a run or of an evaluator call.  `pre` opens every message: "" for mcpc_run, "<entry>: " for an evaluator.
int check_loss_kind(const char* pre, int32_t kind) { return kind < 0 || kind > 2 ? fail(MCPC_EINVAL, "%sloss_kind=%d", pre, kind) : 0; }
int check_loss_values(const char* pre, const mcpc_engine* e, int32_t loss_kind, double loss_var, int32_t mask_start) {
    if (loss_kind == MCPC_LOSS_GAUSSIAN && !(loss_var > 0.0)) return fail(MCPC_EINVAL, "%sloss_var must be positive", pre);
    if (mask_start < 0 || mask_start >= e->d.n_out) return fail(MCPC_EINVAL, "%smask_start=%d outside 0..%d", pre, mask_start, e->d.n_out - 1);
    return 0;
}
int check_loss(const char* pre, const mcpc_engine* e, int32_t loss_kind, double loss_var, int32_t mask_start) {
    if (const int rc = check_loss_kind(pre, loss_kind)) return rc;
    if (loss_kind == MCPC_LOSS_NONE) return 0;
    if (!e->has_head) return fail(MCPC_EINVAL, "%sa loss needs a read-out Linear (n_out > 0)", pre);
    if (!e->target_bound) return fail(MCPC_ESTATE, "%sloss requested but no target bound", pre);
    return check_loss_values(pre, e, loss_kind, loss_var, mask_start);
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
    launch_mu1(e, e->inputs, e->mu1, stream);             // constant during the run: weights only change between runs
    // layer-wise kernels: f(x_l) of the state the run starts from (the backward launches keep it current from there)
    if (e->lw)
        for (int l = 0; l < e->L; ++l) {
            const size_t total4 = (size_t)e->Bpad * e->npad[l] / 4;
            hipLaunchKernelGGL(mcpc_lw_act_kernel, dim3(grid_for(total4)), dim3(256), 0, stream, (const float*)e->x[l], e->lw_fx[l], total4, e->d.acts[l]);
        }
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

// Which instantiation of the in-place kernel a launch of this run takes (mcpc_steps_ws2.h: kWs2Specs).  A specialised mode fixes at compile
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
    return kWs2Specs[spec].fn[mix ? 1 : 0] ? spec : WS2_SPEC_GENERIC;
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

int launch_ws2(RunCtx& c, KParams& K, bool mix, int nblocks, bool accumulating) {
    const int spec = ws2_select_mode(K, c.hot, accumulating, mix);
    (mix ? c.specs_rr : c.specs_plain) |= 1u << spec;
    void* args[] = {&K};
    HIP_TRY(hipLaunchKernel(kWs2Specs[spec].fn[mix ? 1 : 0], dim3(nblocks), dim3(kWs2Threads), args, c.sp.lds_bytes, c.stream));
    return 0;
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
        if (c.use_u) hipLaunchKernelGGL((mcpc_steps_u_kernel<true>), dim3(e->rr_count[i]), dim3(kUThreads), c.sp.lds_bytes, c.stream, Q);
        else if (const int rc = launch_ws2(c, Q, true, e->rr_count[i], accumulating)) return rc;
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
    else if (c.use_u) hipLaunchKernelGGL((mcpc_steps_u_kernel<false>), dim3(e->nwg_live), dim3(kUThreads), c.sp.lds_bytes, c.stream, P);
    else if (e->ws == 2) { if (const int rc = launch_ws2(c, P, false, e->nwg_live, accumulating)) return rc; }
    else hipLaunchKernelGGL((mcpc_steps_kernel<1, 4>), dim3(e->nwg), dim3(256), c.sp.lds_bytes, c.stream, P);
    return prof_end(c, (double)n);
}

// mcpc_last_step_kernel_name of the run
std::string last_step_name(const RunCtx& c) {
    // (a run on the generic instantiation alone reads as it always did; specialised launches are named behind the form they belong to)
    auto spec_tag = [](unsigned specs) -> std::string {
        if (!(specs & ~(1u << WS2_SPEC_GENERIC))) return "";
        std::string tag;
        for (int i = 0; i < WS2_SPEC_COUNT; ++i)
            if (specs & (1u << i)) tag += (tag.empty() ? "" : ", ") + std::string(kWs2Specs[i].tag);
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

int mcpc_read_param_grads(mcpc_engine* e, int j, float* dW, float* db, float scale, int accumulate, void* stream_) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    const int nlin = e->L + (e->has_head ? 1 : 0);
    if (j < 0 || j >= nlin) return fail(MCPC_EINVAL, "Linear index %d out of range", j);
    if (!dW) return fail(MCPC_EINVAL, "null dW");
    HIP_TRY(hipSetDevice(e->d.device));
    const Lin& ln = e->lin[j];
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(mcpc_export_grad_kernel, dim3(grid_for((size_t)ln.n_out * ln.n_in)), dim3(256), 0, stream, ln.G, dW,
                       ln.n_out, ln.n_in, ln.g_ld, scale, accumulate);
    if (db)
        hipLaunchKernelGGL(mcpc_export_grad_kernel, dim3(grid_for((size_t)ln.n_out)), dim3(256), 0, stream, ln.Gb, db,
                           ln.n_out, 1, 1, scale, accumulate);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

// ---- multi-GPU: the one collective of a learning call ---------------------------------------------
int mcpc_comm_unique_id(void* id_out) {
    static_assert(sizeof(ncclUniqueId) == MCPC_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    if (!id_out) return fail(MCPC_EINVAL, "null id buffer");
    if (const int rc = rccl_load()) return rc;
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(MCPC_EHIP, "ncclGetUniqueId: %s", g_rccl.GetErrorString(r));
    std::memcpy(id_out, &id, sizeof(id));
    return MCPC_OK;
}

int mcpc_comm_init(mcpc_engine* e, int n_ranks, int rank, const void* id_in) {
    if (!e || !id_in) return fail(MCPC_EINVAL, "null argument");
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MCPC_EINVAL, "rank %d of %d", rank, n_ranks);
    if (e->comm) return fail(MCPC_ESTATE, "the engine already has a communicator (mcpc_comm_destroy first)");
    if (const int rc = rccl_load()) return rc;
    HIP_TRY(hipSetDevice(e->d.device));
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    const ncclResult_t r = g_rccl.CommInitRank(&e->comm, n_ranks, id, rank);
    if (r != ncclSuccess) { e->comm = nullptr; return fail(MCPC_EHIP, "ncclCommInitRank(%d of %d): %s", rank, n_ranks, g_rccl.GetErrorString(r)); }
    e->comm_ranks = n_ranks;
    return MCPC_OK;
}

int mcpc_allreduce_grads(mcpc_engine* e, float* flat, int64_t n_floats, void* stream_) {
    if (!e || !flat) return fail(MCPC_EINVAL, "null argument");
    if (!e->comm) return fail(MCPC_ESTATE, "mcpc_allreduce_grads before mcpc_comm_init");
    if (n_floats != mcpc_param_count(e)) return fail(MCPC_EINVAL, "bucket of %lld floats, the engine's parameters have %lld", (long long)n_floats, (long long)mcpc_param_count(e));
    HIP_TRY(hipSetDevice(e->d.device));
    const ncclResult_t r = g_rccl.AllReduce(flat, flat, (size_t)n_floats, ncclFloat, ncclSum, e->comm, (hipStream_t)stream_);
    if (r != ncclSuccess) return fail(MCPC_EHIP, "ncclAllReduce: %s", g_rccl.GetErrorString(r));
    return MCPC_OK;
}

int mcpc_comm_destroy(mcpc_engine* e) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    if (e->comm) {
        (void)hipSetDevice(e->d.device);
        const ncclResult_t r = g_rccl.CommDestroy(e->comm);
        e->comm = nullptr; e->comm_ranks = 0;
        if (r != ncclSuccess) return fail(MCPC_EHIP, "ncclCommDestroy: %s", g_rccl.GetErrorString(r));
    }
    return MCPC_OK;
}

int64_t mcpc_param_count(const mcpc_engine* e) {
    if (!e) return 0;
    const int nlin = e->L + (e->has_head ? 1 : 0);
    int64_t n = 0;
    for (int j = 0; j < nlin; ++j) n += (int64_t)e->lin[j].n_out * e->lin[j].n_in + (e->lin[j].bias ? e->lin[j].n_out : 0);
    return n;
}

int mcpc_read_param_grads_flat(mcpc_engine* e, float* flat, int64_t n_floats, float scale, void* stream_) {
    if (!e || !flat) return fail(MCPC_EINVAL, "null argument");
    if (n_floats != mcpc_param_count(e)) return fail(MCPC_EINVAL, "flat buffer holds %lld floats, parameters need %lld", (long long)n_floats, (long long)mcpc_param_count(e));
    const int nlin = e->L + (e->has_head ? 1 : 0);
    int64_t off = 0;
    for (int j = 0; j < nlin; ++j) {
        const Lin& ln = e->lin[j];
        float* dW = flat + off; off += (int64_t)ln.n_out * ln.n_in;
        float* db = nullptr;
        if (ln.bias) { db = flat + off; off += ln.n_out; }
        int rc = mcpc_read_param_grads(e, j, dW, db, scale, 0, stream_);
        if (rc) return rc;
    }
    return MCPC_OK;
}

int mcpc_philox_normals(int device, uint64_t seed, uint64_t step, int layer, uint64_t chain_base, int batch, int n_units,
                        float* out, int raw, void* stream_) {
    if (!out || batch < 1 || n_units < 1 || layer < 0 || layer > 255) return fail(MCPC_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(device));
    const size_t total = (size_t)batch * ((n_units + 3) / 4);
    hipLaunchKernelGGL(mcpc_philox_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream_, seed, step, layer, chain_base,
                       batch, n_units, out, raw);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_box_muller(int device, const uint32_t* a, const uint32_t* b, int64_t n, float* z0, float* z1, void* stream_) {
    if (n < 0) return fail(MCPC_EINVAL, "box_muller: n=%lld, must not be negative", (long long)n);
    if (!a || !b) return fail(MCPC_EINVAL, "box_muller: a or b is null");
    if (!z0 || !z1) return fail(MCPC_EINVAL, "box_muller: z0 or z1 is null");
    if (n == 0) return MCPC_OK;
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(mcpc_box_muller_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream_, a, b, (size_t)n, z0, z1);
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}


namespace {
// The front the two evaluators share (mcpc_chain_energies, mcpc_prediction_errors).  What a call reads and launches over:
struct EvalCall {
    unsigned layers;        // bit l: latent layer l is read -- x_rec[l] is required, and prepared chunk by chunk
    unsigned lins;          // bit j (bit L: the read-out): Linear j is evaluated -- it must be bound; Linear 0 needs mu_1 of the call's inputs
    unsigned pe_table;      // the Linears of the prediction-error job table the call launches over; 0: it launches over the chain-energy table
    bool with_loss;         // the read-out's error is the loss's (its kind and mask reach the kernels)
};

// The evaluators' job tables, mu_1 buffer and scratch for chunks of `chunk` rows
int ce_ensure_scratch(mcpc_engine* e, int chunk, unsigned pe_table, hipStream_t stream) {
    if (!e->ce_jobs) {
        std::vector<LwJob>& jobs = e->ce_table;
        ce_job_table(e->L, e->npad, e->has_head ? e->out_pad : 0, jobs, e->ce_nhead, e->ce_finish);
        if (jobs.size() > 65535) return fail(MCPC_EINVAL, "chain energies: more than 65535 unit-tile jobs");
        if (const int rc = upload(e->ce_jobs, jobs, "the chain-energy job table")) return rc;
        e->ce_njobs = (int)jobs.size();
        if (const int rc = dmalloc(e->ce_mu1, (size_t)e->Bpad * e->npad[0])) return rc;
    }
    if (chunk > e->ce_rows) {
        // everything is given up before the first new allocation: one that fails leaves a consistent, empty scratch
        for (int l = 0; l < e->L; ++l) { give_up(e, e->ce_x[l], stream); give_up(e, e->ce_fx[l], stream); }
        give_up(e, e->ce_part, stream);
        e->ce_rows = 0;
        for (int l = 0; l < e->L; ++l) {
            int rc;
            if ((rc = dmalloc(e->ce_x[l], (size_t)chunk * e->npad[l])) || (rc = dmalloc(e->ce_fx[l], (size_t)chunk * e->npad[l]))) return rc;
        }
        if (const int rc = dmalloc(e->ce_part, (size_t)e->ce_njobs * chunk)) return rc;
        e->ce_rows = chunk;
    }
    if (pe_table && pe_table != e->pe_want) {
        std::vector<LwJob> jobs;
        pe_job_table(e->ce_table, pe_table, jobs);
        give_up(e, e->pe_jobs, stream);
        e->pe_want = 0;                  // (an upload that fails leaves no table, and no set of Linears it would be the table of)
        if (const int rc = upload(e->pe_jobs, jobs, "the prediction-error job table")) return rc;
        e->pe_want = pe_table;
        e->pe_njobs = (int)jobs.size();
    }
    return MCPC_OK;
}

// The checks of a call, before anything of the device is touched; `pre` ("<entry>: ") opens every message
int eval_check_call(const char* pre, const mcpc_engine* e, const float* const* x_rec, int32_t n_rec, int32_t max_rows) {
    if (!e) return fail(MCPC_EINVAL, "%snull engine", pre);
    if (!x_rec) return fail(MCPC_EINVAL, "%sx_rec is null", pre);
    if (n_rec < 0) return fail(MCPC_EINVAL, "%sn_rec=%d, must not be negative", pre, n_rec);
    if (max_rows < 0) return fail(MCPC_EINVAL, "%smax_rows=%d, must not be negative (0 = default)", pre, max_rows);
    return 0;
}
int eval_check_reads(const char* pre, const mcpc_engine* e, const float* const* x_rec, const EvalCall& c) {
    for (int l = 0; l < e->L; ++l)
        if (((c.layers >> l) & 1u) && !x_rec[l]) return fail(MCPC_EINVAL, "%sx_rec[%d] is null", pre, l);
    for (int j = 0; j < e->L + (e->has_head ? 1 : 0); ++j)
        if (((c.lins >> j) & 1u) && !e->lin[j].bound)
            return fail(MCPC_ESTATE, "%sLinear %d has no bound parameters (mcpc_bind_params + mcpc_params_changed first)", pre, j);
    return 0;
}

// An accepted call of R rows: the chunk, the scratch and the tables for it, mu_1 where it is read, and what the two kernels' parameters share
int eval_setup(mcpc_engine* e, const EvalCall& c, const float* inputs, int64_t R, int32_t max_rows, int32_t loss_kind, double loss_var,
               int32_t mask_start, hipStream_t stream, CeParams& Q) {
    HIP_TRY(hipSetDevice(e->d.device));
    // the chunk: a multiple of the 64-row tile, no longer than the call
    const int64_t want = max_rows > 0 ? max_rows : kCeDefaultRows;
    const int chunk = (int)(std::min<int64_t>((want + kLwChains - 1) / kLwChains, (R + kLwChains - 1) / kLwChains) * kLwChains);
    if (const int rc = ce_ensure_scratch(e, chunk, c.pe_table, stream)) return rc;
    free_completed_retired(e);
    if (c.lins & 1u) launch_mu1(e, inputs, e->ce_mu1, stream);      // mu_1 of THESE inputs (the step kernels' own kernel: the same bits)
    const int nlin = e->L + (e->has_head ? 1 : 0);
    for (int l = 0; l < e->L; ++l) { Q.x[l] = e->ce_x[l]; Q.fx[l] = e->ce_fx[l]; Q.npad[l] = e->npad[l]; Q.ecoef[l] = e->d.ecoef[l]; }
    for (int j = 1; j < nlin; ++j) { Q.Wf[j] = e->lin[j].Wf; Q.bias[j] = e->lin[j].bias_pad; }
    Q.npad[e->L] = e->has_head ? e->out_pad : 0;
    Q.mu1 = e->ce_mu1; Q.y = e->ypad; Q.wexp = e->wexp;
    Q.L = e->L; Q.B = e->d.batch; Q.n_out = e->d.n_out; Q.chunk = chunk;
    Q.loss_kind = c.with_loss ? loss_kind : MCPC_LOSS_NONE; Q.mask_start = c.with_loss ? mask_start : 0;
    Q.inv_var = loss_kind == MCPC_LOSS_GAUSSIAN ? (float)(1.0 / loss_var) : 1.0f;
    return MCPC_OK;
}

// The chunk loop: x_l and f(x_l) of the layers the call reads go to the scratch, then `launch(r0, rows, padded)` launches the entry's own
// kernels for rows [r0, r0 + rows) of the call, with Q.rows and Q.row_base set (padded: the rows of the tiles that hold one)
int eval_chunks(const mcpc_engine* e, const EvalCall& c, const float* const* x_rec, int64_t R, CeParams& Q, hipStream_t stream,
                const std::function<void(int64_t, int, int)>& launch) {
    for (int64_t r0 = 0; r0 < R; r0 += Q.chunk) {
        const int rows = (int)std::min<int64_t>(Q.chunk, R - r0);
        const int padded = (rows + kLwChains - 1) / kLwChains * kLwChains;
        for (int l = 0; l < e->L; ++l) {
            if (!((c.layers >> l) & 1u)) continue;
            const size_t total4 = (size_t)padded * e->npad[l] / 4;
            hipLaunchKernelGGL(mcpc_ce_prep_kernel, dim3(grid_for(total4)), dim3(256), 0, stream, x_rec[l] + (size_t)r0 * e->d.sizes[l],
                               e->ce_x[l], e->ce_fx[l], rows, padded, e->d.sizes[l], e->npad[l], e->d.acts[l]);
        }
        Q.rows = rows;
        Q.row_base = (int)(r0 % e->d.batch);
        launch(r0, rows, padded);
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}
}  // namespace

int mcpc_chain_energies(mcpc_engine* e, const float* inputs, const float* const* x_rec, int32_t n_rec, int32_t loss_kind, double loss_var,
                        int32_t mask_start, double* out, int32_t max_rows, void* stream_) {
    static const char pre[] = "chain energies: ";
    if (const int rc = eval_check_call(pre, e, x_rec, n_rec, max_rows)) return rc;
    if (!out) return fail(MCPC_EINVAL, "chain energies: out is null");
    // every layer is read and every Linear evaluated
    const bool with_loss = loss_kind != MCPC_LOSS_NONE;
    const EvalCall c{(1u << e->L) - 1u, (1u << (e->L + (e->has_head ? 1 : 0))) - 1u, 0u, with_loss};
    if (const int rc = eval_check_reads(pre, e, x_rec, c)) return rc;
    if (const int rc = check_loss(pre, e, loss_kind, loss_var, mask_start)) return rc;
    const int64_t R = (int64_t)n_rec * e->d.batch;
    if (R == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    CeParams Q{};
    if (const int rc = eval_setup(e, c, inputs, R, max_rows, loss_kind, loss_var, mask_start, stream, Q)) return rc;
    Q.part = e->ce_part;
    Q.job0 = with_loss ? 0 : e->ce_nhead;
    Q.jobs = e->ce_jobs + Q.job0;
    const int njobs = e->ce_njobs - Q.job0;
    return eval_chunks(e, c, x_rec, R, Q, stream, [&](int64_t r0, int rows, int padded) {
        hipLaunchKernelGGL(mcpc_ce_kernel, dim3(padded / kLwChains, njobs), dim3(kLwThreads), 0, stream, Q);
        hipLaunchKernelGGL(mcpc_ce_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, (const double*)e->ce_part, out, e->ce_finish,
                           e->L, with_loss ? 1 : 0, rows, Q.chunk, (size_t)r0);
    });
}

int mcpc_prediction_errors(mcpc_engine* e, const float* inputs, const float* const* x_rec, int32_t n_rec, int32_t loss_kind, double loss_var,
                           int32_t mask_start, float* const* err, float* const* pred, float* err_out, float* pred_out, int32_t max_rows,
                           void* stream_) {
    static const char pre[] = "prediction errors: ";
    if (const int rc = eval_check_call(pre, e, x_rec, n_rec, max_rows)) return rc;
    const int L = e->L;
    // the Linears asked for (bit j; bit L = the read-out) and the latent layers their predictions read
    unsigned want = 0;
    for (int l = 0; l < L; ++l)
        if ((err && err[l]) || (pred && pred[l])) want |= 1u << l;
    if (err_out || pred_out) want |= 1u << L;
    if (!want) return fail(MCPC_EINVAL, "prediction errors: nothing is asked for (every destination is null)");
    if ((err_out || pred_out) && !e->has_head) return fail(MCPC_EINVAL, "prediction errors: err_out / pred_out need a read-out Linear (n_out > 0)");
    if (const int rc = check_loss_kind(pre, loss_kind)) return rc;
    if (err_out && loss_kind == MCPC_LOSS_NONE) return fail(MCPC_EINVAL, "prediction errors: err_out needs a loss (loss_kind is MCPC_LOSS_NONE)");
    if (err_out)
        if (const int rc = check_loss_values(pre, e, loss_kind, loss_var, mask_start)) return rc;
    const EvalCall c{pe_layers_read(want, L), want, want, err_out != nullptr};
    if (const int rc = eval_check_reads(pre, e, x_rec, c)) return rc;
    if (err_out && !e->target_bound) return fail(MCPC_ESTATE, "prediction errors: err_out requested but no target bound");
    const int64_t R = (int64_t)n_rec * e->d.batch;
    if (R == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    PeParams P{};
    CeParams& Q = P.ce;
    if (const int rc = eval_setup(e, c, inputs, R, max_rows, loss_kind, loss_var, mask_start, stream, Q)) return rc;
    Q.jobs = e->pe_jobs;
    for (int l = 0; l < L; ++l) P.n[l] = e->d.sizes[l];
    P.n[L] = e->d.n_out;
    // 16-byte stores where every row of a destination starts on a 16-byte boundary
    auto vec_ok = [](const float* p, int n) { return p && n % 4 == 0 && ((uintptr_t)p & 15u) == 0; };
    for (int j = 0; j <= L; ++j) {
        const float* const ep = j < L ? (err ? err[j] : nullptr) : err_out;
        const float* const pp = j < L ? (pred ? pred[j] : nullptr) : pred_out;
        if (vec_ok(ep, P.n[j])) P.vec_err |= 1u << j;
        if (vec_ok(pp, P.n[j])) P.vec_pred |= 1u << j;
    }
    return eval_chunks(e, c, x_rec, R, Q, stream, [&](int64_t r0, int /*rows*/, int padded) {
        // (a chunk starts at a multiple of kLwChains rows: r0 * n_l floats keeps the 16-byte alignment where n_l % 4 == 0)
        for (int j = 0; j <= L; ++j) {
            float* const ep = j < L ? (err ? err[j] : nullptr) : err_out;
            float* const pp = j < L ? (pred ? pred[j] : nullptr) : pred_out;
            P.err[j] = ep ? ep + (size_t)r0 * P.n[j] : nullptr;
            P.pred[j] = pp ? pp + (size_t)r0 * P.n[j] : nullptr;
        }
        hipLaunchKernelGGL(mcpc_pe_kernel, dim3(padded / kLwChains, e->pe_njobs), dim3(kLwThreads), 0, stream, P);
    });
}

int mcpc_sample_prior(mcpc_engine* e, const float* inputs, int64_t n, uint64_t seed, uint64_t step, uint64_t sample_base, int32_t loss_kind,
                      double loss_var, int32_t readout, float* const* x_out, float* out, int32_t max_rows, void* stream_) {
    static const char pre[] = "sample prior: ";
    if (!e) return fail(MCPC_EINVAL, "%snull engine", pre);
    if (n < 0) return fail(MCPC_EINVAL, "%sn=%lld, must not be negative", pre, (long long)n);
    constexpr uint64_t kChains = 1ull << 32;            // the Philox chain word is 32 bits
    if (sample_base > kChains || (uint64_t)n > kChains - sample_base)
        return fail(MCPC_EINVAL, "%ssample_base=%llu + n=%lld passes 2^32 (the generator's chain word is 32 bits)", pre,
                    (unsigned long long)sample_base, (long long)n);
    if (max_rows < 0) return fail(MCPC_EINVAL, "%smax_rows=%d, must not be negative (0 = default)", pre, max_rows);
    if (readout != MCPC_SAMPLE_HIDDEN && readout != MCPC_SAMPLE_MEAN && readout != MCPC_SAMPLE_DRAW)
        return fail(MCPC_EINVAL, "%sunknown readout %d", pre, readout);
    if (const int rc = check_loss_kind(pre, loss_kind)) return rc;
    const int L = e->L;
    if (out && !e->has_head) return fail(MCPC_EINVAL, "%sout needs a read-out Linear (n_out > 0)", pre);
    // the Linears to run: up to the read-out, or to the last latent layer asked for
    int last = out ? L : -1;
    if (!out && x_out)
        for (int l = 0; l < L; ++l)
            if (x_out[l]) last = l;
    if (last < 0) return fail(MCPC_EINVAL, "%snothing is asked for (every destination is null)", pre);
    if (out && readout != MCPC_SAMPLE_HIDDEN) {
        if (loss_kind == MCPC_LOSS_NONE) return fail(MCPC_EINVAL, "%sthe mean or a draw of the read-out needs a loss (loss_kind is MCPC_LOSS_NONE)", pre);
        if (readout == MCPC_SAMPLE_DRAW && loss_kind == MCPC_LOSS_GAUSSIAN && !(loss_var > 0.0))
            return fail(MCPC_EINVAL, "%sloss_var=%g, must be positive", pre, loss_var);
    }
    // (every ecoef is positive: mcpc_create refuses an engine with another one, so 1 / sqrt(ecoef) below is finite)
    for (int j = 0; j <= last; ++j)
        if (!e->lin[j].bound)
            return fail(MCPC_ESTATE, "%sLinear %d has no bound parameters (mcpc_bind_params + mcpc_params_changed first)", pre, j);
    if (n == 0) return MCPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(e->d.device));
    // the chunk: a multiple of the 64-row tile, no longer than the call; the scratch and the job table are the evaluators'
    const int64_t want = max_rows > 0 ? max_rows : kCeDefaultRows;
    const int chunk = (int)(std::min<int64_t>((want + kLwChains - 1) / kLwChains, (n + kLwChains - 1) / kLwChains) * kLwChains);
    if (const int rc = ce_ensure_scratch(e, chunk, 0u, stream)) return rc;
    free_completed_retired(e);
    int mode = kSpLogits;
    if (readout == MCPC_SAMPLE_MEAN && loss_kind == MCPC_LOSS_BERNOULLI) mode = kSpSigmoid;
    if (readout == MCPC_SAMPLE_DRAW) mode = loss_kind == MCPC_LOSS_BERNOULLI ? kSpBernoulli : kSpGaussian;
    const Lin& l0 = e->lin[0];
    const int n_in = e->d.n_in;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int rows = (int)std::min<int64_t>(chunk, n - r0);
        const int padded = (rows + kLwChains - 1) / kLwChains * kLwChains;
        // mu_1 of the chunk's inputs, by the runs' and the evaluators' own kernel, in the scratch no launch of this call reads as x_0
        hipLaunchKernelGGL(mcpc_mu1_kernel, dim3(grid_for((size_t)padded * e->npad[0])), dim3(256), 0, stream,
                           inputs ? inputs + (size_t)r0 * n_in : nullptr, l0.W, l0.bias, e->ce_x[0], rows, n_in, e->d.sizes[0], padded, e->npad[0]);
        for (int j = 0; j <= last; ++j) {
            const bool head = j == L;
            SpParams P{};
            P.fx_in = j > 0 ? e->ce_fx[j - 1] : nullptr;
            P.fx_out = j < last ? e->ce_fx[j] : nullptr;
            P.Wf = j > 0 ? e->lin[j].Wf : nullptr;
            P.bias = j > 0 ? e->lin[j].bias_pad : nullptr;
            P.mu1 = e->ce_x[0];
            P.wexp = e->wexp;
            P.jobs = e->ce_jobs + e->ce_finish.first[j];
            P.seed = seed; P.step = step; P.g0 = sample_base + (uint64_t)r0;
            P.kw = j > 0 ? e->npad[j - 1] : 0;
            P.npad = head ? e->out_pad : e->npad[j];
            P.n = head ? e->d.n_out : e->d.sizes[j];
            P.act = head ? 0 : e->d.acts[j];
            P.rows = rows;
            P.mode = head ? mode : kSpLatent;
            P.scale = head ? (mode == kSpGaussian ? (float)std::sqrt(loss_var) : 1.0f) : (float)(1.0 / std::sqrt((double)e->d.ecoef[j]));
            float* const base = head ? out : (x_out ? x_out[j] : nullptr);
            // (a chunk starts at a multiple of kLwChains rows: r0 * n floats keeps the 16-byte alignment where n % 4 == 0)
            P.dst = base ? base + (size_t)r0 * P.n : nullptr;
            P.vec = base && P.n % 4 == 0 && ((uintptr_t)base & 15u) == 0;
            hipLaunchKernelGGL(mcpc_sp_kernel, dim3(padded / kLwChains, e->ce_finish.count[j]), dim3(kLwThreads), 0, stream, P);
        }
    }
    HIP_TRY(hipGetLastError());
    return MCPC_OK;
}

int mcpc_query(const mcpc_engine* e, int32_t* lds_bytes, int32_t* chains_per_wg, int32_t* n_workgroups, int32_t* spill_slots) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    if (lds_bytes) *lds_bytes = e->main.lds_bytes;
    if (chains_per_wg) *chains_per_wg = e->lw ? kLwChains : e->ct;
    if (n_workgroups) *n_workgroups = e->nwg_live;
    if (spill_slots) *spill_slots = e->slots;
    return MCPC_OK;
}

const char* mcpc_step_kernel_name(const mcpc_engine* e) { return e ? step_kernel_name(*e) : ""; }

const char* mcpc_last_step_kernel_name(const mcpc_engine* e) {
    return e ? e->last_step.c_str() : "";
}

const char* mcpc_last_flush_plan(const mcpc_engine* e, int j) {
    if (!e || j < 0 || j >= e->L + (e->has_head ? 1 : 0)) return "";
    return e->last_flush[j].c_str();
}

int mcpc_sync_check(mcpc_engine* e, void* stream_) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->d.device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream_));
    int flag = 0;
    HIP_TRY(hipMemcpy(&flag, e->err, sizeof(int), hipMemcpyDeviceToHost));
    if (flag != 0) {
        (void)hipMemset(e->err, 0, sizeof(int));
        return fail(MCPC_ESTATE, "the step kernel reported error word 0x%x (a workgroup-internal progress wait ran out): results of the last run are invalid", flag);
    }
    return MCPC_OK;
}

int mcpc_last_shader_clock_ghz(mcpc_engine* e, float* ghz) {
    if (!e || !ghz) return fail(MCPC_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipMemcpy(h, e->clk, sizeof h, hipMemcpyDeviceToHost));              // (waits for the device)
    *ghz = h[1] ? (float)((double)h[0] / (double)h[1] * 0.1) : 0.f;
    return MCPC_OK;
}

// ---- diagnostic: poison the LDS of every CU (include/mcpc.h: mcpc_debug_poison_lds) -------------------------------------------
}  // extern "C"
namespace {
// One workgroup per CU at a time (it takes the whole 160 KiB of LDS): fills it with `word`, then holds its CU for ~20 us so that
// the dispatcher has to place the other workgroups of the launch on the other CUs.  `seen[xcc * 64 + cu]` counts the visits.
__global__ __launch_bounds__(256) void mcpc_poison_lds_kernel(uint32_t word, int* seen) {
    extern __shared__ uint32_t poison_lds[];
    for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) poison_lds[i] = word;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        // HW_ID: cu_id bits 11:8, sh_id bit 12, se_id bits 15:13 (gfx9)
        const int cu = (int)((hw >> 8) & 0xff);
        atomicAdd(&seen[(xcc & 7) * 256 + cu], 1);
        const unsigned long long t_end = wall_clock64() + 2000;          // 100 MHz ticks: 20 us
        while (wall_clock64() < t_end) __builtin_amdgcn_s_sleep(32);
    }
    __syncthreads();
    // keep the stores observable: a read the compiler cannot drop
    if (poison_lds[(threadIdx.x * 97) % (160 * 1024 / 4)] != word) atomicAdd(&seen[8 * 256], 1);
}
}  // namespace
extern "C" {

int mcpc_debug_poison_lds(int device, uint32_t word, void* stream_) {
    HIP_TRY(hipSetDevice(device));
    int n_cu = 256;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cu <= 0) n_cu = 256;
    static bool attr_set[16] = {false};
    if (device >= 0 && device < 16 && !attr_set[device]) {
        HIP_TRY(hipFuncSetAttribute((const void*)mcpc_poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set[device] = true;
    }
    int* seen = nullptr;
    HIP_TRY(hipMalloc((void**)&seen, (8 * 256 + 1) * sizeof(int)));
    hipStream_t stream = (hipStream_t)stream_;
    int rc = MCPC_OK;
    // two passes of four workgroups per CU: a CU that was still draining another kernel during the first is caught by the second
    for (int pass = 0; pass < 2 && rc == MCPC_OK; ++pass) {
        if (hipMemsetAsync(seen, 0, (8 * 256 + 1) * sizeof(int), stream) != hipSuccess) { rc = fail(MCPC_EHIP, "hipMemsetAsync failed"); break; }
        hipLaunchKernelGGL(mcpc_poison_lds_kernel, dim3(4 * n_cu), dim3(256), 160 * 1024, stream, word, seen);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) rc = fail(MCPC_EHIP, "the LDS poison kernel failed");
    }
    if (rc == MCPC_OK) {
        std::vector<int> h(8 * 256 + 1);
        if (hipMemcpy(h.data(), seen, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MCPC_EHIP, "hipMemcpy failed");
        else {
            int visited = 0;
            for (int i = 0; i < 8 * 256; ++i) visited += h[i] > 0;
            if (visited < n_cu) rc = fail(MCPC_ESTATE, "LDS poison reached %d of %d compute units", visited, n_cu);
            else if (h[8 * 256] != 0) rc = fail(MCPC_ESTATE, "LDS poison read-back mismatch");
        }
    }
    (void)hipFree(seen);
    return rc;
}

int mcpc_debug_lw_jobs(int32_t n_latent, const int32_t* sizes, int32_t n_out, int32_t* fwd, int32_t* bwd, int32_t cap,
                       int32_t* n_fwd, int32_t* n_bwd, int32_t* tile) {
    if (n_latent < 1 || n_latent > kMaxLatent || !sizes || n_out < 0) return fail(MCPC_EINVAL, "bad network");
    int npad[kMaxLatent];
    for (int l = 0; l < n_latent; ++l) { if (sizes[l] < 1) return fail(MCPC_EINVAL, "sizes[%d]=%d", l, sizes[l]); npad[l] = pad16(sizes[l]); }
    std::vector<LwJob> f, b;
    lw_job_table(n_latent, npad, pad16(n_out), f, b);
    for (int i = 0; i < (int)f.size() && i < cap && fwd; ++i) { fwd[2 * i] = f[i].layer; fwd[2 * i + 1] = f[i].ut0; }
    for (int i = 0; i < (int)b.size() && i < cap && bwd; ++i) { bwd[2 * i] = b[i].layer; bwd[2 * i + 1] = b[i].ut0; }
    if (n_fwd) *n_fwd = (int32_t)f.size();
    if (n_bwd) *n_bwd = (int32_t)b.size();
    if (tile) { tile[0] = kLwChains; tile[1] = kLwUnitTiles; }
    return MCPC_OK;
}

int mcpc_debug_chain_energy_jobs(int32_t n_latent, const int32_t* sizes, int32_t n_out, int32_t* jobs, int32_t cap, int32_t* n_jobs,
                                 int32_t* n_head, int32_t* tile) {
    if (n_latent < 1 || n_latent > kMaxLatent || !sizes || n_out < 0) return fail(MCPC_EINVAL, "bad network");
    int npad[kMaxLatent];
    for (int l = 0; l < n_latent; ++l) { if (sizes[l] < 1) return fail(MCPC_EINVAL, "sizes[%d]=%d", l, sizes[l]); npad[l] = pad16(sizes[l]); }
    std::vector<LwJob> t;
    int nh = 0;
    CeFinish F;
    ce_job_table(n_latent, npad, pad16(n_out), t, nh, F);
    for (int i = 0; i < (int)t.size() && i < cap && jobs; ++i) { jobs[2 * i] = t[i].layer; jobs[2 * i + 1] = t[i].ut0; }
    if (n_jobs) *n_jobs = (int32_t)t.size();
    if (n_head) *n_head = nh;
    if (tile) { tile[0] = kLwChains; tile[1] = kLwUnitTiles; }
    return MCPC_OK;
}

int mcpc_debug_plan(const mcpc_net_desc* d, int32_t n_cu, int64_t total_mem, char* out, int64_t cap, int64_t* needed) {
    if (!d || n_cu < 1 || total_mem < 0 || cap < 0 || (cap > 0 && !out)) return fail(MCPC_EINVAL, "bad argument");
    if (const int rc = check_net_desc(d)) return rc;
    EnginePlan plan;
    if (const int rc = parse_tuning(d->tuning, plan.knobs)) return rc;
    if (const int rc = plan_engine(*d, n_cu, (size_t)total_mem, plan)) return rc;
    const std::string s = plan_json(plan);
    if (needed) *needed = (int64_t)s.size() + 1;
    if (cap > 0) { const size_t n = std::min<size_t>(s.size(), (size_t)cap - 1); std::memcpy(out, s.data(), n); out[n] = 0; }
    return MCPC_OK;
}

int mcpc_debug_run_plan(const mcpc_net_desc* d, int32_t n_cu, int64_t total_mem, const mcpc_run_desc* r, char* out, int64_t cap, int64_t* needed) {
    if (!d || !r || n_cu < 1 || total_mem < 0 || cap < 0 || (cap > 0 && !out)) return fail(MCPC_EINVAL, "bad argument");
    if (const int rc = check_net_desc(d)) return rc;
    EnginePlan plan;
    if (const int rc = parse_tuning(d->tuning, plan.knobs)) return rc;
    if (const int rc = plan_engine(*d, n_cu, (size_t)total_mem, plan)) return rc;
    if (const int rc = check_step_range(*r)) return rc;
    RunPlan run;
    plan_run(plan, *r, MCPC_STAMPS_BUILD != 0, run);
    const std::string s = run_plan_json(plan, run);
    if (needed) *needed = (int64_t)s.size() + 1;
    if (cap > 0) { const size_t n = std::min<size_t>(s.size(), (size_t)cap - 1); std::memcpy(out, s.data(), n); out[n] = 0; }
    return MCPC_OK;
}

int mcpc_set_profiling(mcpc_engine* e, int enable) {
    if (!e) return fail(MCPC_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->d.device));
    e->profiling = enable != 0;
    e->events_used = 0;
    e->prof_steps = 0;
    if (enable) HIP_TRY(hipMemset(e->clk, 0, 2 * sizeof(unsigned long long)));      // (synchronises with the device: a diagnostic call)
    return MCPC_OK;
}

namespace {
int sum_events(const std::vector<std::pair<hipEvent_t, hipEvent_t>>& ev, size_t used, float* total) {
    *total = 0.f;
    for (size_t i = 0; i < used; ++i) {
        HIP_TRY(hipEventSynchronize(ev[i].second));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[i].first, ev[i].second));
        *total += t;
    }
    return 0;
}
}  // namespace

int mcpc_last_step_kernel_ms(mcpc_engine* e, float* ms, int32_t* n_launches, int64_t* n_steps) {
    if (!e || !ms) return fail(MCPC_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(e->d.device));
    const int rc = sum_events(e->events, e->events_used, ms);
    if (rc) return rc;
    if (n_launches) *n_launches = (int32_t)e->events_used;
    if (n_steps) *n_steps = (int64_t)std::llround(e->prof_steps);
    return MCPC_OK;
}

}  // extern "C"
