// Definition of one __global__ form of the in-place step kernel around the shared body (mcpc_steps_ws2_body.inc).  Included by
// mcpc_steps_ws2.h once per kernel name, with WS2_KERNEL_TEMPLATE (its template head: MIX among the parameters, and an int CTT that
// is part of the symbol and always 1), WS2_KERNEL_NAME and WS2_MODE (the body's compile-time mode, a Ws2Mode) defined; all three are
// undefined again here.
WS2_KERNEL_TEMPLATE
__global__ __launch_bounds__(kWs2Threads, MCPC_WS2_WAVES_PER_EU) void WS2_KERNEL_NAME(const KParams P) {
    static_assert(CTT == 1, "part of the symbol: one chain tile per workgroup");
    extern __shared__ __attribute__((aligned(16))) float lds[];
#define WS2_BLOCK blockIdx.x
#define WS2_NBLOCKS gridDim.x
#include "mcpc_steps_ws2_body.inc"
#undef WS2_BLOCK
#undef WS2_NBLOCKS
}
#undef WS2_KERNEL_TEMPLATE
#undef WS2_KERNEL_NAME
#undef WS2_MODE
