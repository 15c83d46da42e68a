// hbm_kernels.hip — min-sum / BP decoding with the message state in HBM, for
// codes the LDS-resident kernels cannot hold (per-half-shot state beyond a
// CU's LDS, or tables past the 16-bit formats). Same arithmetic as the
// LDS kernels and the oracle, bit for bit (decoders.py:110-182, :189-290).
//
// Layout and execution:
//  * one workgroup = one TILE of 64 half-shot slots: lane l of every wave
//    works on slot l, and the workgroup's W waves split each layer's rows
//    (check nodes) and adjacent variables (variable nodes) between them, with
//    a workgroup barrier between the two phases. A tile's state is contiguous
//    in HBM, element-major inside the tile: c2v[g][p][64] (CSC position p),
//    posterior[g][v][64], syndrome[g][c][64] — every message access is one
//    coalesced 256 / 512-byte row, and all the waves of a CU touch the same
//    ~20 MB (a handful of 2 MB pages: the CU's address-translation working set
//    stays small; one thread per half-shot with slot-major rows over the whole
//    grid made every access a translation miss);
//  * graph tables are read wave-uniformly (scalar loads);
//  * min-sum keeps the float32 column sum S per variable (posterior = L +
//    (f64)S, decoders.py:172-173, rebuilt on read): 4-byte rows, SURVEY.md
//    §8(d)'s w = 4; BP keeps the float64 posterior;
//  * slots recycle: a slot whose decode stops (or reaches max_iter) writes its
//    outputs and takes the next half-shot from a global ticket counter at the
//    next iteration boundary, so early-stopping decodes keep the tile busy;
//  * no state initialisation pass when the layers partition the rows (always
//    for the reference's schedules): in a slot's first iteration, a message
//    of a check its layer has not reached yet reads as 0 and a posterior no
//    variable node has written yet as L (per-edge / per-variable "first layer"
//    tables) — the same values the reference's freshly zeroed arrays hold;
//  * stop test after every layer (decoders.py:175-176, :283-285): 32 parity
//    filters (F == B, kept current from the hard-decision flips the variable
//    nodes see, combined over the waves through LDS) gate the exact check over
//    all rows, as in ms_layered_kernel.
// HBM traffic per executed half-shot iteration is SURVEY.md §8(d)'s model
// (flooding MS: 4(3E + 2n) bytes + the old-posterior read for the flip test).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "decoder_kernels.h"
#include "hbm_kernels.h"
#include "../../include/qldpc_libm.h"

namespace qldpc {

__constant__ qldpc_libm_tab qldpc_libm_hbm_dev = QLDPC_LIBM_TAB_INIT;

// NumPy's DOUBLE_pairwise_sum (np.sum of a 1-D float64 array) over a strided
// column of the c2v rows: 0.0 + pairwise(all), 8 accumulators for d >= 8
// (decoders.py:269, :276); entries with zero[t] read as +0.0.
template <typename Get>
__device__ __forceinline__ double np_pairwise_strided(int d, Get get) {
  if (d < 8) {
    double res = -0.0;
    for (int i = 0; i < d; ++i) res += get(i);
    return 0.0 + res;
  }
  double r0 = get(0), r1 = get(1), r2 = get(2), r3 = get(3), r4 = get(4), r5 = get(5), r6 = get(6), r7 = get(7);
  int i = 8;
  const int nb = d - (d % 8);
  for (; i < nb; i += 8) {
    r0 += get(i + 0); r1 += get(i + 1); r2 += get(i + 2); r3 += get(i + 3);
    r4 += get(i + 4); r5 += get(i + 5); r6 += get(i + 6); r7 += get(i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < d; ++i) res += get(i);
  return 0.0 + res;
}

// Graph tables are read-only for the whole launch: reading them through the
// constant address space lets the compiler use scalar loads (wave-uniform
// indices) — through a generic pointer it must assume the kernel's own stores
// may alias them and issues a vector load + readfirstlane per table word.
template <typename T>
__device__ __forceinline__ T tb(const T* p, int i) {
  return ((const __attribute__((address_space(4))) T*)p)[i];
}

// np.sum of a column of more than 128 entries, for the BP instances of
// hbm_tile_kernel and hbm_tile_vprior_kernel alike: there DOUBLE_pairwise_sum
// halves the range (the left half a multiple of 8) and adds the halves' sums;
// a leaf of 64..128 entries is the 8-accumulator block.
// Walked leaf by leaf, left to right: the node in hand is a depth and a word of
// turns (bit k: right at depth k), its range found again from the root each
// time (uniform scalar work: d is the wave's), and the one per-lane state is
// the sum of the left sibling pending at each depth: stack[(k - 1) * stride],
// k = 1 .. hbm_column_depth(d), in the launch's dynamic LDS (hbm_kernels.h).
// (np_pairwise_strided above runs the 8 accumulators over the whole column: it
// is NumPy's association up to 128 entries and is called for those alone.)
template <typename Get>
__device__ __forceinline__ double np_pairwise_deep(int d, Get get, double* stack, int stride) {
  uint32_t turns = 0;
  int sp = 0;
  double ret;
  for (;;) {
    int o = 0, n = d;
    for (int k = 1; k <= sp; ++k) {                  // the node at (turns, sp)
      int n2 = n / 2;
      n2 -= n2 % 8;
      if ((turns >> k) & 1u) o += n2, n -= n2;
      else n = n2;
    }
    while (n > 128) {                                // down to its leftmost leaf
      int n2 = n / 2;
      n2 -= n2 % 8;
      n = n2;
      ++sp;
    }
    double r0 = get(o), r1 = get(o + 1), r2 = get(o + 2), r3 = get(o + 3), r4 = get(o + 4), r5 = get(o + 5),
           r6 = get(o + 6), r7 = get(o + 7);
    int i = 8;
    const int nb = n - (n % 8);
    for (; i < nb; i += 8) {
      r0 += get(o + i + 0); r1 += get(o + i + 1); r2 += get(o + i + 2); r3 += get(o + i + 3);
      r4 += get(o + i + 4); r5 += get(o + i + 5); r6 += get(o + i + 6); r7 += get(o + i + 7);
    }
    ret = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) ret += get(o + i);
    while (sp > 0 && ((turns >> sp) & 1u)) {         // a right child done: its parent's sum
      ret = stack[(sp - 1) * stride] + ret;
      turns &= ~(1u << sp);
      --sp;
    }
    if (sp == 0) break;
    stack[(sp - 1) * stride] = ret;                  // a left child done: on to its sibling
    turns |= 1u << sp;
  }
  return 0.0 + ret;
}

// combine one word per wave and lane through LDS: every wave writes its
// partial, a barrier, every wave reads all W partials. `buf` [W][64] may be
// rewritten only after the next workgroup barrier (all readers passed it).
template <int W, typename Op>
__device__ __forceinline__ uint32_t wg_combine(uint32_t* buf, uint32_t x, int wave, int lane, Op op) {
  buf[wave * 64 + lane] = x;
  __syncthreads();
  uint32_t r = buf[lane];
#pragma unroll
  for (int w = 1; w < W; ++w) r = op(r, buf[w * 64 + lane]);
  return r;
}

// hbm_tile_kernel and its per-variable-prior twin hbm_tile_vprior_kernel (pr.Lv,
// pr.filt0; a.L and a.L32 are unread: DESIGN.md §3.17) share one body,
// hbm_tile_body.inc, included into each kernel.
template <int ALGO, int DCMAX, int W>
__global__ void __launch_bounds__(64 * W) hbm_tile_kernel(HbmArgs a, const int32_t* __restrict__ fl_var,
                                                        const int32_t* __restrict__ fl_pos, int lazy) {
#define QLDPC_HBM_VPRIOR 0
#include "hbm_tile_body.inc"
#undef QLDPC_HBM_VPRIOR
}

template <int ALGO, int DCMAX, int W>
__global__ void __launch_bounds__(64 * W) hbm_tile_vprior_kernel(HbmArgs a, const int32_t* __restrict__ fl_var,
                                                               const int32_t* __restrict__ fl_pos, int lazy,
                                                               HbmPrior pr) {
#define QLDPC_HBM_VPRIOR 1
#include "hbm_tile_body.inc"
#undef QLDPC_HBM_VPRIOR
}

// kernel names as rocprofv3 reports them (ALGO_MS = 0, ALGO_BP = 1)
#define QLDPC_HBM(ALG, A, D)                                                                   \
  if (algo == ALG && dcmax <= D) {                                                             \
    if (name) *name = "hbm_tile_kernel<" #A ", " #D ", 4>";                                    \
    return (const void*)&hbm_tile_kernel<ALG, D, kHbmWaves>;                                   \
  }
// (rows past 64 edges take the 64-wide instance's two-pass cn_wide)
const void* select_hbm_kernel(int algo, int dcmax, const char** name) {
  QLDPC_HBM(ALGO_MS, 0, 8) QLDPC_HBM(ALGO_MS, 0, 16) QLDPC_HBM(ALGO_MS, 0, 32)
  QLDPC_HBM(ALGO_BP, 1, 8) QLDPC_HBM(ALGO_BP, 1, 16) QLDPC_HBM(ALGO_BP, 1, 32)
  if (name) *name = algo == ALGO_MS ? "hbm_tile_kernel<0, 64, 4>" : "hbm_tile_kernel<1, 64, 4>";
  return algo == ALGO_MS ? (const void*)&hbm_tile_kernel<ALGO_MS, 64, kHbmWaves>
                         : (const void*)&hbm_tile_kernel<ALGO_BP, 64, kHbmWaves>;
}
#undef QLDPC_HBM

// the same choice for hbm_tile_vprior_kernel (rows past 64 edges: cn_wide)
#define QLDPC_HBM_VP(ALG, A, D)                                                                \
  if (algo == ALG && (dcmax <= D || D == 64)) {                                                \
    if (name) *name = "hbm_tile_vprior_kernel<" #A ", " #D ", 4>";                             \
    return (const void*)&hbm_tile_vprior_kernel<ALG, D, kHbmWaves>;                            \
  }
const void* select_hbm_vprior_kernel(int algo, int dcmax, const char** name) {
  QLDPC_HBM_VP(ALGO_MS, 0, 8) QLDPC_HBM_VP(ALGO_MS, 0, 16) QLDPC_HBM_VP(ALGO_MS, 0, 32) QLDPC_HBM_VP(ALGO_MS, 0, 64)
  QLDPC_HBM_VP(ALGO_BP, 1, 8) QLDPC_HBM_VP(ALGO_BP, 1, 16) QLDPC_HBM_VP(ALGO_BP, 1, 32) QLDPC_HBM_VP(ALGO_BP, 1, 64)
  if (name) *name = "";
  return nullptr;                                    // (algo is MS or BP: not reached)
}
#undef QLDPC_HBM_VP

hipError_t launch_hbm(const void* kernel, const HbmArgs& a, int tiles, const int32_t* fl_var, const int32_t* fl_pos,
                      int lazy, size_t lds, hipStream_t stream) {
  void* params[] = {(void*)&a, (void*)&fl_var, (void*)&fl_pos, (void*)&lazy};
  return hipLaunchKernel(kernel, dim3(tiles), dim3(64 * kHbmWaves), params, lds, stream);
}

hipError_t launch_hbm_vprior(const void* kernel, const HbmArgs& a, const HbmPrior& pr, int tiles, const int32_t* fl_var,
                             const int32_t* fl_pos, int lazy, size_t lds, hipStream_t stream) {
  void* params[] = {(void*)&a, (void*)&fl_var, (void*)&fl_pos, (void*)&lazy, (void*)&pr};
  return hipLaunchKernel(kernel, dim3(tiles), dim3(64 * kHbmWaves), params, lds, stream);
}

}  // namespace qldpc
