// relay_vprior_kernels.hip — relay min-sum with one prior per variable
// (DESIGN.md §3.18): relay_ms_kernel's body (relay_kernel_body.inc) with L
// replaced by the row entry L_j, which each workgroup keeps in LDS behind the
// graph image, and, under cost 1, solutions weighed by the fixed-point priors
// W_j instead of counted. A translation unit of its own, so the objects of
// every other kernel, relay_ms_kernel's among them, are built exactly as
// without it.
#include "relay_common.h"

namespace qldpc {

template <int DC>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) relay_vprior_kernel(RelayVpriorArgs va) {
  constexpr bool VP = true;
  const RelayArgs& ra = va.r;
  const long long* wgt = va.wgt;
  const int cost = va.cost;
#include "relay_kernel_body.inc"
}

const void* select_relay_vprior_kernel(int dc, const char** name) {
  static const char* names[3] = {"relay_vprior_kernel<0>", "relay_vprior_kernel<7>", "relay_vprior_kernel<8>"};
  if (name) *name = names[dc == 7 ? 1 : (dc == 8 ? 2 : 0)];
  switch (dc) {
    case 7: return (const void*)&relay_vprior_kernel<7>;
    case 8: return (const void*)&relay_vprior_kernel<8>;
    default: return (const void*)&relay_vprior_kernel<0>;
  }
}

hipError_t launch_relay_vprior(const void* kernel, const RelayVpriorArgs& args, int grid, int block, int lds_bytes,
                               hipStream_t stream) {
  void* params[] = {(void*)&args};
  return hipLaunchKernel(kernel, dim3(grid), dim3(block), params, (size_t)lds_bytes, stream);
}

}  // namespace qldpc
