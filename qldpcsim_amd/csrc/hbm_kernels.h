// hbm_kernels.h — the HBM-resident decoder (codes whose per-half-shot state
// does not fit a CU's LDS, or whose tables overflow the 16-bit LDS formats).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tuning.h"

namespace qldpc {

// One workgroup of kHbmWaves waves = one tile of 64 half-shot slots (lane l =
// slot l); every lane of a wave walks the same check / variable at the same
// time, so graph reads are wave-uniform (scalar loads) and message reads are
// coalesced: tile g's element i of slot l at [g][i][64].
constexpr int kHbmWaves = QLDPC_HBM_WAVES;   // (kernel names in hbm_kernels.hip spell out 4)
struct HbmArgs {
  // graph (relabeled variables, int32, global)
  const int32_t* row_ptr;   // [m+1] CSR
  const int32_t* row_var;   // [E]   relabeled variable of CSR edge e (ascending original variable)
  const int32_t* row_pos;   // [E]   CSC position of CSR edge e
  const int32_t* col_ptr;   // [n+1] CSC over relabeled variables (ascending check inside a column)
  const int32_t* vinv;      // [n]   original column -> relabeled variable
  const uint32_t* wc;       // [m]   stop-test filter word per check
  const uint32_t* avar;     // [n]   filter word per relabeled variable
  uint32_t filt_all;
  // schedule
  const int32_t* lay_ptr;   // [L+1]
  const int32_t* lay_rows;  // [*]
  const int32_t* adj_ptr;   // [L+1]
  const int32_t* adj_vars;  // [*]   relabeled variables adjacent to the layer's rows, ascending
  int n_layers;
  int m, n, E;
  // workspace (tile-major: [tiles][elements][64 slots])
  void* c2v;                // [tiles][E][64]  float (MS) / double (BP)
  void* post;               // [tiles][n][64]  float32 column sum S (MS) / float64 posterior (BP)
  uint8_t* synT;            // [tiles][m][64]
  // batch
  const uint8_t* syn;       // [batch][m] bytes, or uint64 [batch][wm] words
  uint8_t* ehat;            // [batch][n] bytes, or uint64 [batch][wn] words
  int32_t* iters;
  double* out_post;         // [batch][n] original order, or null
  int32_t* flags;
  int syn_bits, eh_bits, wm, wn;
  long long batch;
  uint32_t* queue;          // shot ticket counter (zeroed before the launch)
  double L, beta, eps;
  float L32;
  int max_iter;
};
// What hbm_tile_vprior_kernel takes on top (HbmArgs::L and L32 are then
// unread): one prior per variable. Kernel parameters of their own, not HbmArgs
// fields: with the struct two fields longer the scalar min-sum instances
// compiled to other register allocations.
struct HbmPrior {
  const double* Lv;         // [n]   L_v of relabeled variable v (qldpc_prior::d_L)
  uint32_t filt0;           // XOR of avar[v] over the variables with Lv[v] < 0: a slot's filter word at start
};

// dcmax: row degree bound of the instantiation (8, 16, 32 or 64)
const void* select_hbm_kernel(int algo, int dcmax, const char** name);
// hbm_tile_vprior_kernel<algo, D, 4>, chosen by the row degree in the same way
const void* select_hbm_vprior_kernel(int algo, int dcmax, const char** name);
// fl_var / fl_pos: first layer reaching each variable / CSC position; lazy =
// the layers partition the rows (no state initialisation pass); lds: the
// plan's hbm_vprior_lds (BP with a column past 128 entries; else 0)
hipError_t launch_hbm(const void* kernel, const HbmArgs& a, int tiles, const int32_t* fl_var, const int32_t* fl_pos,
                      int lazy, size_t lds, hipStream_t stream);
// NumPy's pairwise summation splits a column of more than 128 entries in two,
// again and again: the levels below the root for d entries (0 up to 128). The
// BP instances of both kernels keep one pending sum per level and lane in dynamic
// LDS, hbm_vprior_lds(deepest column of the code) bytes (0 for most codes).
inline int hbm_column_depth(int d) {
  if (d <= 128) return 0;
  int n2 = d / 2;
  n2 -= n2 % 8;
  const int left = hbm_column_depth(n2), right = hbm_column_depth(d - n2);
  return 1 + (left > right ? left : right);
}
inline size_t hbm_vprior_lds(int depth) { return (size_t)depth * 64 * kHbmWaves * sizeof(double); }
// lds: hbm_vprior_lds of the plan (BP; min-sum sums its columns in sequence: 0)
hipError_t launch_hbm_vprior(const void* kernel, const HbmArgs& a, const HbmPrior& pr, int tiles, const int32_t* fl_var,
                             const int32_t* fl_pos, int lazy, size_t lds, hipStream_t stream);

}  // namespace qldpc
