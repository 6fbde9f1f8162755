// libmcpc.so, the unified-wave step kernel (mcpc_steps_u.h): mcpc_steps_u_kernel<false> for a plain launch, <true> for a launch of the
// round schedule, with their launcher (mcpc_step_forms.h).
#include <hip/hip_runtime.h>

#include "mcpc_step_forms.h"
#include "mcpc_steps_u.h"

using namespace mcpc;

hipError_t mcpc::u_allow_lds(int bytes) {
    const hipError_t err = hipFuncSetAttribute((const void*)mcpc_steps_u_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return err != hipSuccess ? err : hipFuncSetAttribute((const void*)mcpc_steps_u_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
void mcpc::launch_u(bool mix, int nblocks, int lds_bytes, const KParams& K, hipStream_t stream) {
    if (mix) hipLaunchKernelGGL((mcpc_steps_u_kernel<true>), dim3(nblocks), dim3(kUThreads), lds_bytes, stream, K);
    else hipLaunchKernelGGL((mcpc_steps_u_kernel<false>), dim3(nblocks), dim3(kUThreads), lds_bytes, stream, K);
}
