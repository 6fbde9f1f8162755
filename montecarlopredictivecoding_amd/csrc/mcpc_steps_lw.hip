// libmcpc.so, the two fallback forms of the step kernel, neither LDS-resident in the in-place kernel's way: the layer-wise kernels
// (mcpc_steps_lw.h: networks too wide for any LDS plan) and the barrier kernel mcpc_steps_kernel<1, 4> (mcpc_steps_barrier.h: where no
// in-place plan fits), with their launchers (mcpc_step_forms.h).
#include <hip/hip_runtime.h>

#include "mcpc_engine.h"
#include "mcpc_step_forms.h"
#include "mcpc_steps_barrier.h"
#include "mcpc_steps_lw.h"

using namespace mcpc;

hipError_t mcpc::barrier_allow_lds(int bytes) {
    return hipFuncSetAttribute((const void*)mcpc_steps_kernel<1, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
void mcpc::launch_barrier(int nblocks, int lds_bytes, const KParams& K, hipStream_t stream) {
    hipLaunchKernelGGL((mcpc_steps_kernel<1, 4>), dim3(nblocks), dim3(256), lds_bytes, stream, K);
}

void mcpc::launch_lw_act(const mcpc_engine* e, hipStream_t stream) {
    for (int l = 0; l < e->L; ++l) {
        const size_t total4 = (size_t)e->Bpad * e->npad[l] / 4;
        hipLaunchKernelGGL(mcpc_lw_act_kernel, dim3(grid_for(total4)), dim3(256), 0, stream, (const float*)e->x[l], e->lw_fx[l], total4, e->d.acts[l]);
    }
}

int mcpc::launch_lw_steps(mcpc_engine* e, const mcpc_run_desc* r, const KParams& P, int t0, int n, hipStream_t stream) {
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
