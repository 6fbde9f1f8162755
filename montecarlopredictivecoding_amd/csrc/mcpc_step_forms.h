// What the host knows of the step kernels without seeing them: one launcher per kernel form, defined in the unit that holds the form's
// kernels.  mcpc_run's executor (mcpc_run.hip) and mcpc_create (mcpc_api.hip) reach every step kernel through this header alone; no
// kernel pointer crosses a unit boundary.  Host declarations only, like mcpc_heb_forms.h for the Hebbian flush.
#pragma once
#include <hip/hip_runtime.h>

#include "mcpc_types.h"

struct mcpc_engine;

namespace mcpc {

// ---- the in-place kernel (mcpc_steps_ws2.h) -----------------------------------------------------------------------------------------------
// Its instantiations: the generic kernel (mcpc_steps_ws2.hip) and the ones with a launch's decisions fixed at compile time
// (mcpc_steps_ws2_spec.hip; ws2_select_mode in mcpc_run.hip picks one per launch).  `mix`: the round schedule's form.
enum Ws2Spec { WS2_SPEC_GENERIC = 0, WS2_SPEC_HOT, WS2_SPEC_HOT_SPILL, WS2_SPEC_MAP, WS2_SPEC_COUNT };
bool ws2_spec_built(int spec, bool mix);             // (a build with MCPC_EXP_NOLEAN holds the generic kernel only)
const char* ws2_spec_tag(int spec);                  // what mcpc_last_step_kernel_name adds to the generic kernel's name
hipError_t ws2_allow_lds(bool mix, int bytes);       // every instantiation built, generic first, is allowed `bytes` of dynamic LDS
int launch_ws2(int spec, bool mix, int nblocks, int lds_bytes, KParams& K, hipStream_t stream);

// ---- the unified-wave kernel (mcpc_steps_u.h, mcpc_steps_u.hip) ---------------------------------------------------------------------------
hipError_t u_allow_lds(int bytes);                   // both forms
void launch_u(bool mix, int nblocks, int lds_bytes, const KParams& K, hipStream_t stream);

// ---- the two fallback forms (mcpc_steps_lw.hip) -------------------------------------------------------------------------------------------
// the barrier kernel mcpc_steps_kernel<1, 4> (mcpc_steps_barrier.h)
hipError_t barrier_allow_lds(int bytes);
void launch_barrier(int nblocks, int lds_bytes, const KParams& K, hipStream_t stream);
// the layer-wise kernels (mcpc_steps_lw.h).  launch_lw_act: f(x_l) of the state a run starts from, one launch per layer.  launch_lw_steps:
// steps [t0, t0 + n) of a run, two launches per step on the caller's stream.  `P` carries the segment's spill pointers (spill_t0 = t0); what
// changes from step to step travels in the launch arguments.
void launch_lw_act(const mcpc_engine* e, hipStream_t stream);
int launch_lw_steps(mcpc_engine* e, const mcpc_run_desc* r, const KParams& P, int t0, int n, hipStream_t stream);

}  // namespace mcpc
