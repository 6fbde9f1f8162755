// libmcpc.so, the in-place step kernel (mcpc_steps_ws2.h): its generic instantiation mcpc_steps_ws2_kernel<1, MIX>, and the launchers
// through which the host reaches every instantiation (mcpc_step_forms.h) -- the specialised ones are compiled in a unit of their own,
// mcpc_steps_ws2_spec.hip, so that the eight instantiations of the body build side by side.
#include <hip/hip_runtime.h>

#include "mcpc_step_forms.h"
#include "mcpc_steps_ws2.h"

using namespace mcpc;

namespace {
const Ws2SpecEntry kGeneric = {{(const void*)mcpc_steps_ws2_kernel<1, false>, (const void*)mcpc_steps_ws2_kernel<1, true>}, "generic"};
}  // namespace

bool mcpc::ws2_spec_built(int spec, bool mix) { return spec == WS2_SPEC_GENERIC || ws2_specialised_built(spec, mix); }
const char* mcpc::ws2_spec_tag(int spec) { return spec == WS2_SPEC_GENERIC ? kGeneric.tag : ws2_specialised_tag(spec); }
hipError_t mcpc::ws2_allow_lds(bool mix, int bytes) {
    const hipError_t err = ws2_entry_allow_lds(kGeneric, mix, bytes);
    return err != hipSuccess ? err : ws2_specialised_allow_lds(mix, bytes);
}
int mcpc::launch_ws2(int spec, bool mix, int nblocks, int lds_bytes, KParams& K, hipStream_t stream) {
    return spec == WS2_SPEC_GENERIC ? ws2_entry_launch(kGeneric, mix, nblocks, lds_bytes, K, stream)
                                    : ws2_specialised_launch(spec, mix, nblocks, lds_bytes, K, stream);
}
