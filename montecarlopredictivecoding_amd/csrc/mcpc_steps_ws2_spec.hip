// libmcpc.so, the in-place step kernel (mcpc_steps_ws2.h) with a launch's decisions fixed at compile time: the instantiations of
// mcpc_steps_ws2_spec_kernel the library holds, listed ONCE, below.  ws2_select_mode (mcpc_run.hip) picks one per launch; the launchers
// of mcpc_steps_ws2.hip hand a specialised spec on to this unit.
#include <hip/hip_runtime.h>

#include "mcpc_step_forms.h"
#include "mcpc_steps_ws2.h"

using namespace mcpc;

namespace {

// The hot set: what every script of the reference runs per step on a ReLU network with a Bernoulli read-out -- lean SGD with the fused
// Philox kick, state and constants in LDS, row words, a bit-packed 0/1 target -- apart by whether the launch accumulates (its spill
// stores then go out at system scope).
template <int SPILL> using Ws2HotMode = Ws2Mode<WS2_UPD_SGD_PHILOX, 1, 1, SPILL, WS2_HEAD_BERNOULLI_BITS, MCPC_ACT_RELU>;
// The MAP warm-up of the same networks: Adam on x without noise, nothing accumulated.
using Ws2MapMode = Ws2Mode<WS2_UPD_ADAM, 1, 1, WS2_SPILL_OFF, WS2_HEAD_BERNOULLI_BITS, MCPC_ACT_RELU>;

#ifndef MCPC_EXP_NOLEAN
#define WS2_SPEC_ROW(mode, tag) {{(const void*)mcpc_steps_ws2_spec_kernel<mode, 1, false>, (const void*)mcpc_steps_ws2_spec_kernel<mode, 1, true>}, tag}
const Ws2SpecEntry kSpecs[WS2_SPEC_COUNT] = {
    {{nullptr, nullptr}, ""},           // WS2_SPEC_GENERIC: mcpc_steps_ws2.hip
    WS2_SPEC_ROW(Ws2HotMode<WS2_SPILL_OFF>, "hot"),
    WS2_SPEC_ROW(Ws2HotMode<WS2_SPILL_SYS>, "hot+spill"),
    // (a spill that stays in the L2 -- a small shard, a narrow network: KParams::spill_sys == 0 -- keeps the generic kernel: the in-place
    // kernel serves such shards only under tuning ws=2, and no measurement asked for an instantiation of their own)
    WS2_SPEC_ROW(Ws2MapMode, "map"),
};
#undef WS2_SPEC_ROW
#else       // (timing build without the lean epilogues: the generic kernel everywhere)
const Ws2SpecEntry kSpecs[WS2_SPEC_COUNT] = {{{nullptr, nullptr}, ""}, {{nullptr, nullptr}, ""}, {{nullptr, nullptr}, ""}, {{nullptr, nullptr}, ""}};
#endif

}  // namespace

bool mcpc::ws2_specialised_built(int spec, bool mix) { return kSpecs[spec].fn[mix] != nullptr; }
const char* mcpc::ws2_specialised_tag(int spec) { return kSpecs[spec].tag; }
hipError_t mcpc::ws2_specialised_allow_lds(bool mix, int bytes) {
    hipError_t err = hipSuccess;
    for (int i = 0; i < WS2_SPEC_COUNT && err == hipSuccess; ++i) err = ws2_entry_allow_lds(kSpecs[i], mix, bytes);
    return err;
}
int mcpc::ws2_specialised_launch(int spec, bool mix, int nblocks, int lds_bytes, KParams& K, hipStream_t stream) {
    return ws2_entry_launch(kSpecs[spec], mix, nblocks, lds_bytes, K, stream);
}
