// libmcpc.so, the Hebbian flush: the launches that fold a segment of spilled steps into the gradient sums of the Linears j >= 1, with
// their kernels (mcpc_hebbian.h: the only unit that includes them).  What to launch was decided on the host (mcpc_plan.h: plan_flush);
// mcpc_run (mcpc_run.hip) calls flush_spill once per accumulating segment.
#include <hip/hip_runtime.h>

#include "mcpc_engine.h"
#include "mcpc_hebbian.h"

using namespace mcpc;

namespace {

// The tiled Hebbian kernels, family (HEB_F16, HEB_FP32: mcpc_plan.h) x form (kHebForms: mcpc_heb_forms.h): every instantiation the
// library holds, with its dynamic LDS.  A planned launch names its entry; nothing else chooses a kernel.
struct HebKernel { void (*fn)(HebArgs); int lds_bytes; bool attr_set[16]; };      // (attr_set: per device)
#define MCPC_HEB7_ROW(te, ra, sw) {mcpc_heb7_kernel<te, ra, sw>, heb7_lds_bytes(te), {false}},
#define MCPC_HEB_ROW(te, ra, sw) {mcpc_heb_kernel<te, ra, sw>, heb_lds_bytes(te, ra), {false}},
HebKernel g_heb_kernels[2][kNumHebForms] = {{MCPC_HEB_FORMS(MCPC_HEB7_ROW)}, {MCPC_HEB_FORMS(MCPC_HEB_ROW)}};
#undef MCPC_HEB7_ROW
#undef MCPC_HEB_ROW

int launch_heb(const FlushLaunch& l, const HebArgs& a, hipStream_t stream) {
    if ((l.family != HEB_F16 && l.family != HEB_FP32) || l.form < 0 || l.form >= kNumHebForms)
        return fail(MCPC_ESTATE, "internal: no Hebbian kernel %s<%d,%d%s> (form %d)", heb_family_name(l.family), l.te, l.ra, l.swapped ? ",T" : "", l.form);
    HebKernel& k = g_heb_kernels[l.family][l.form];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 16 && !k.attr_set[dev]) {
        if (hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes) != hipSuccess)
            return fail(MCPC_EHIP, "hipFuncSetAttribute failed for the Hebbian kernel");
        k.attr_set[dev] = true;
    }
    hipLaunchKernelGGL(k.fn, dim3(a.n_mt * a.n_nt * a.ksplit), dim3(kHebThreads), k.lds_bytes, stream, a);
    return 0;
}

}  // namespace

// One Hebbian flush, as planned (mcpc_plan.h: plan_flush): fold the spilled steps from slot `slot0` on into the gradient sums of every
// Linear j >= 1.  Every Linear has its own slab region, so the GEMMs of a flush are independent launches and ONE reduction launch
// follows them.  An overlapped flush spreads them over two low-priority streams (`stream` and aux3); the reduction joins them.
int mcpc::flush_spill(mcpc_engine* e, const FlushPlan& f, int slot0, hipStream_t stream, int part) {
    const unsigned* const smax = e->spillmax + (size_t)part * kSpillTensors;      // largest |value| per spilled tensor of this segment
    if (f.two_streams && !e->aux3) return fail(MCPC_ESTATE, "internal: a flush planned for two streams on an engine that has one");
    hipStream_t const streams[2] = {stream, f.two_streams ? e->aux3 : stream};
    if (f.two_streams) { HIP_TRY(hipEventRecord(e->ev_fork, stream)); HIP_TRY(hipStreamWaitEvent(e->aux3, e->ev_fork, 0)); }
    ReduceJobs jobs{};
    for (int j = 1; j < e->L + e->has_head; ++j) {
        const Lin& ln = e->lin[j];
        const LinFlush& lf = f.lin[j];
        const int ne = ln.out_pad, na = ln.in_pad;
        const float* E = (j < e->L ? e->spill_e[j] : e->spill_eo) + (size_t)slot0 * e->Bpad * ne;
        const float* A = e->spill_a[j - 1] + (size_t)slot0 * e->Bpad * na;
        const unsigned* const e_max = smax + (j < e->L ? spill_id_e(j) : kSpillIdEo), * const a_max = smax + spill_id_a(j - 1);
        float* slab = e->slab + ln.slab_off;
        float* slab_b = slab + (size_t)lf.ksplit * ne * na;
        for (int i = 0; i < lf.n_launch; ++i) {
            const FlushLaunch& l = lf.launch[i];
            if (l.family == HEB_DW) {
                hipLaunchKernelGGL(mcpc_dw_kernel, dim3((l.wave_tiles + 3) / 4, lf.ksplit), dim3(256), 0, streams[l.stream], E, A, slab, slab_b,
                                   f.rows, ne, na, lf.rps);
                continue;
            }
            // (swapped: the transposed product -- the activations take the E slot, the errors the A slot; slab = [split][na][ne])
            const bool sw = l.swapped;
            const HebArgs a{sw ? A : E, sw ? E : A, slab, slab_b, f.rows, sw ? na : ne, sw ? ne : na, lf.rps, l.n_mt, l.n_nt, lf.ksplit, l.col0,
                            sw ? a_max : e_max, sw ? e_max : a_max};
            if (const int rc = launch_heb(l, a, streams[l.stream])) return rc;
        }
        e->last_flush[j] = lf.text;
        jobs.job[jobs.n_jobs++] = ReduceJob{slab, ln.G, ne * na, lf.ksplit, lf.sign, lf.tr_cols, lf.tr_ld};
        jobs.job[jobs.n_jobs++] = ReduceJob{slab_b, ln.Gb, ne, lf.ksplit, lf.sign, 0, 0};
    }
    if (f.two_streams) { HIP_TRY(hipEventRecord(e->ev_join, e->aux3)); HIP_TRY(hipStreamWaitEvent(stream, e->ev_join, 0)); }
    if (jobs.n_jobs > 0)
        hipLaunchKernelGGL(mcpc_reduce_jobs_kernel, dim3(f.max_blocks, jobs.n_jobs), dim3(256), 0, stream, jobs);
    HIP_TRY(hipGetLastError());
    return 0;
}
