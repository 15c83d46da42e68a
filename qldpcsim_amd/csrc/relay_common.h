// relay_common.h — device functions of the relay kernels (relay_kernels.hip,
// relay_vprior_kernels.hip), whose shared body is relay_kernel_body.inc.
#pragma once
#include <type_traits>

#include "decode_generic.h"
#include "relay_kernels.h"

namespace qldpc {

// Lam_j: the prior blended with the previous posterior (-ffp-contract=off
// keeps the two products and the add apart)
__device__ __forceinline__ double relay_blend(double g, double L, double M) {
  const double a = (1.0 - g) * L;
  const double b = g * M;
  return a + b;
}

// sum of x over the wave's 64 lanes, in every lane (exact: integers)
__device__ __forceinline__ long long relay_wave_sum(long long x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

}  // namespace qldpc
