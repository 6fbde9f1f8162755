// Host side of libmcpc.so: the C ABI declared in include/mcpc.h, in ten translation units.
//   mcpc_api.hip (this one)    the engine's life cycle and bindings, gradient read-out, RCCL, the normals, the query, debug and profiling
//                              entries, with the small kernels they launch (mcpc_engine_kernels.h)
//   mcpc_run.hip               mcpc_run: its checks, the per-run tables and the executor of the run's plan; no step kernel
//   mcpc_steps_ws2.hip         the in-place step kernel, generic: mcpc_steps_ws2_kernel<1, *>, and the launchers of all its instantiations
//   mcpc_steps_ws2_spec.hip    ... specialised: mcpc_steps_ws2_spec_kernel for the hot, hot+spill and MAP modes
//   mcpc_steps_u.hip           the unified-wave step kernel mcpc_steps_u_kernel<*>
//   mcpc_steps_lw.hip          the two fallback forms: the layer-wise kernels and the barrier kernel mcpc_steps_kernel<1, 4>
//   mcpc_eval.hip              the evaluators (chain energies, prediction errors) and the ancestral sampler, with their kernels
//   mcpc_flush.hip             the Hebbian flush of the Linears j >= 1 (flush_spill) and its kernels
//   mcpc_records.hip           the stateless reducers over recorded states (int device, no engine) and their kernels
//   mcpc_build_info.hip        mcpc_abi_version, mcpc_build_info: the one unit that is compiled with the provenance defines
// A kernel is launched by host code of the unit that defines it; what crosses a unit boundary is declared in mcpc_step_forms.h (the step
// kernels' launchers) and mcpc_engine.h (the engine, its buffers, flush_spill, launch_mu1, the loss checks).  No torch.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is loaded with dlopen on first use (no link dependency)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mcpc_build.h"
#include "mcpc_engine.h"
#include "mcpc_step_forms.h"
#include "mcpc_engine_kernels.h"        // the small kernels this unit launches

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
    for (int l = 0; l < kMaxLatent; ++l) F(e->sg_err[l]);
    F(e->sg_err_o); F(e->sg_bjobs);
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

// A step table, bound to the packed weights and uploaded: a GEMM over Linear a_lin reads its forward image in FWD / HEADF entries (the
// Linear predicts the entry's units) and its backward image in HEADB / BWD entries (the error is projected back through it).
int upload_table(mcpc_engine* e, StepPlan& p) {
    for (KPhase& k : p.table)
        if (k.a_lin >= 1) k.A = (k.type == PH_FWD || k.type == PH_HEADF) ? e->lin[k.a_lin].Wf : e->lin[k.a_lin].Wb;
    return upload(p.dev, p.table, "the phase table");
}

// The round schedule's tables, and its forms of the in-place kernel
int upload_rounds(mcpc_engine* e) {
    if (const int rc = upload(e->rr_tab, e->rr_host, "the round-schedule tables")) return rc;
    if (ws2_allow_lds(true, e->main.lds_bytes) != hipSuccess) return fail(MCPC_EHIP, "hipFuncSetAttribute failed for the round schedule");
    return 0;
}

}  // namespace

// (mcpc_engine.h)
void mcpc::retire(mcpc_engine* e, void* p, hipStream_t stream) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, stream) != hipSuccess) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;                                  // no event: the buffer waits for mcpc_destroy
    }
    e->retired.push_back({p, ev});
}
void mcpc::free_completed_retired(mcpc_engine* e) {
    size_t keep = 0;
    for (size_t i = 0; i < e->retired.size(); ++i) {
        auto& q = e->retired[i];
        if (q.ev && hipEventQuery(q.ev) == hipSuccess) { (void)hipFree(q.p); (void)hipEventDestroy(q.ev); }
        else e->retired[keep++] = q;
    }
    e->retired.resize(keep);
    (void)hipGetLastError();                           // hipEventQuery's hipErrorNotReady is not an error of this run
}

// (mcpc_engine.h)
void mcpc::launch_mu1(const mcpc_engine* e, const float* inputs, float* dst, int rows, int padded, hipStream_t stream) {
    const Lin& l0 = e->lin[0];
    const size_t total = (size_t)padded * e->npad[0];
    hipLaunchKernelGGL(mcpc_mu1_kernel, dim3(grid_for(total)), dim3(256), 0, stream, inputs, l0.W, l0.bias, dst,
                       rows, e->d.n_in, e->d.sizes[0], padded, e->npad[0]);
}

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
    hipError_t herr = e->lw ? hipSuccess : e->ws == 2 ? ws2_allow_lds(false, e->main.lds_bytes) : barrier_allow_lds(e->main.lds_bytes);
    if (herr != hipSuccess) return bail(fail(MCPC_EHIP, "hipFuncSetAttribute(%d bytes LDS) failed: %s", e->main.lds_bytes, hipGetErrorString(herr)));
    if (e->rr && (rc = upload_rounds(e))) return bail(rc);
    if (e->u.on && u_allow_lds(e->u.plan.lds_bytes) != hipSuccess)
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

extern "C" {

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
