// decoder_kernels.hip — batched BP / normalized Min-Sum decoding on MI355X (gfx950).
//
// Replaces the per-shot message loops of albertogp71/qLDPCsim
//   MS_decoder  qLDPCsim/decoders.py:110-182
//   BP_decoder  qLDPCsim/decoders.py:189-290
// for a batch of syndromes (one "half-shot" = one decode of one syndrome).
//
// Execution model:
//  * One wavefront decodes one half-shot start to finish. All of its message
//    state lives in that wave's slice of LDS:
//        post  f64[n]          posterior LLR per variable  (decoders.py:173 / :276)
//        c2v   f32[E] (MS) or f64[E] (BP), stored in CSC (variable-major) order
//        syn / parity bit-words (layered schedule only)
//    so HBM traffic is the syndrome in (m B), ê out (n B), iterations/flags.
//  * The Tanner graph (CSR check->(var, csc position), CSC pointers, layer
//    lists) is one read-only blob staged into LDS once per workgroup.
//  * Check-node phase: lane owns whole checks; min1/min2/first-argmin/sign
//    product (MS) or the tanh product (BP) are folded in-lane over the
//    check's edges in ascending variable order — no cross-lane traffic.
//  * Variable-node phase: lane owns whole variables; the column sum runs over
//    the contiguous CSC segment in ascending check order — the exact order of
//    NumPy's axis-0 reduction (MS, float32) or np.sum's pairwise rule (BP).
//  * Persistent: each wave strides over half-shots; the grid is sized to the
//    occupancy the LDS budget allows (host side, capi_decode.cpp).
//
// Numerics: MS c2v = fl32(beta * min) formed in float64;
// VN sum float32 sequential; posterior and v2c float64; first layer of the
// first iteration sees float32(L). BP float64; tanh/atanh from
// include/qldpc_libm.h (basic IEEE ops only: identical on GPU and CPU oracle).
// Compiled with -ffp-contract=off: no FMA contraction may change a rounding.

//
// This translation unit holds decode_kernel and ms_layered_kernel, their
// selectors and the launch helpers. The BP team kernels and the flooding
// min-sum kernel are instantiated in translation units of their own
// (bp_team_kernels.hip, built without SLP vectorization; ms_flood_kernels.hip,
// built with the max-ILP machine scheduler), and so are the two-level-prior
// kernels (decode_prior_kernels.hip), the per-variable-prior kernels
// (decode_vprior_kernels.hip) and relay min-sum (relay_kernels.hip,
// relay_vprior_kernels.hip). Each
// includes its family's header (bp_team.h, ms_flood.h, ms_layered.h,
// decode_generic.h) over decoder_common.h and wave_common.h.

#include "decode_generic.h"
#include "ms_layered.h"

namespace qldpc {

// ---------------------------------------------------------------------------
// Host-side launch helpers (called from capi_decode.cpp)
// ---------------------------------------------------------------------------
int ms_flood_max_waves(int kc) { return (kc >= 8 ? 512 : 256) / 64; }

const void* select_ms_layered_kernel(int dc, int g, const char** name) {
#define QLDPC_MSL(D, Gn) if (dc == D && g == Gn) QLDPC_NAMED((&ms_layered_kernel<D, Gn>), "ms_layered_kernel<" #D ", " #Gn ">");
  QLDPC_MSL(7, 0) QLDPC_MSL(8, 0) QLDPC_MSL(7, 1) QLDPC_MSL(8, 1) QLDPC_MSL(7, 2) QLDPC_MSL(8, 2)
  QLDPC_MSL(7, 4) QLDPC_MSL(8, 4) QLDPC_MSL(7, 8) QLDPC_MSL(8, 8)
#undef QLDPC_MSL
  return nullptr;
}

QLDPC_GENERIC_SELECTOR(select_kernel, decode_kernel)

hipError_t launch_decode(const void* kernel, const DecodeArgs& args, int grid, int block,
                         int lds_bytes, hipStream_t stream) {
  void* params[] = {(void*)&args};
  return hipLaunchKernel(kernel, dim3(grid), dim3(block), params, (size_t)lds_bytes, stream);
}

hipError_t configure_kernel(const void* kernel, int lds_bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

}  // namespace qldpc
