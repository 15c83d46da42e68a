// relay_kernels.hip — relay min-sum: flooding min-sum with a
// per-variable memory strength, run as a chain of legs that each start from
// the previous leg's posteriors, keeping the lightest of the solutions found.
//
// One wavefront decodes one half-shot start to finish, graph image and state
// in LDS, as decode_kernel does; the check node and the column sum are
// decode_generic.h's device functions (cn_ms_uniform / cn_update,
// ms_colsum). A translation unit of its own, so the objects of every other
// kernel are built exactly as without it.
//
// The kernel's body is relay_kernel_body.inc, shared with relay_vprior_kernel
// (relay_vprior_kernels.hip).
#include "relay_common.h"

namespace qldpc {

template <int DC>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) relay_ms_kernel(RelayArgs ra) {
  constexpr bool VP = false;
  constexpr const long long* wgt = nullptr;
  constexpr int cost = 0;
#include "relay_kernel_body.inc"
}

const void* select_relay_kernel(int dc, const char** name) {
  static const char* names[3] = {"relay_ms_kernel<0>", "relay_ms_kernel<7>", "relay_ms_kernel<8>"};
  if (name) *name = names[dc == 7 ? 1 : (dc == 8 ? 2 : 0)];
  switch (dc) {
    case 7: return (const void*)&relay_ms_kernel<7>;
    case 8: return (const void*)&relay_ms_kernel<8>;
    default: return (const void*)&relay_ms_kernel<0>;
  }
}

hipError_t launch_relay(const void* kernel, const RelayArgs& args, int grid, int block, int lds_bytes,
                        hipStream_t stream) {
  void* params[] = {(void*)&args};
  return hipLaunchKernel(kernel, dim3(grid), dim3(block), params, (size_t)lds_bytes, stream);
}

hipError_t configure_relay_kernel(const void* kernel, int lds_bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

}  // namespace qldpc
