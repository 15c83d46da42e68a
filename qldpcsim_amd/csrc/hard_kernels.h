// hard_kernels.h — the hard-decision decoders (naive greedy, bit flipping):
// shared between hard_kernels.hip and the C-ABI host code (capi_hard.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

enum { ALGO_NG = 2, ALGO_BF = 3 };
constexpr int kHardMaxWaves = 8;   // waves per workgroup the kernels are compiled for

// Kernel arguments (by value). The graph tables are 16-bit and live in global
// memory, in ORIGINAL variable labels (NG's tie rule and both outputs are in
// original order); LDS holds only each wave's state slice:
//   bf_kernel  syndrome words | residual words | estimate words
//   ng_kernel  scores u16[npad] | residual words | estimate words
// (words: 32-bit, 2 ceil(len / 64) of them; npad = n rounded up to 128).
struct HardArgs {
  const uint16_t* row_ptr;   // [m + 1] CSR
  const uint16_t* row_var;   // [E]     variables of each row, ascending
  const uint16_t* col_ptr;   // [n + 1] CSC
  const uint16_t* col_chk;   // [E]     checks of each column, ascending
  const uint16_t* row_ell;   // [m][8]  the first 8 variables of each row, padded with 0 (16-byte aligned)
  const uint16_t* col_ell;   // [n][8]  the first 8 checks of each column
  int m, n, wm, wn;          // wm = ceil(m / 64), wn = ceil(n / 64)
  int npad;
  int wave_bytes;            // per-wave LDS slice (multiple of 16)
  int off_res, off_est;      // inside a slice (syndrome words / scores at 0)
  const void* syn;           // uint8 [batch][m] or uint64 [batch][wm]
  void* ehat;                // uint8 [batch][n] or uint64 [batch][wn]
  int32_t* iters;            // [batch] BF iterations / NG steps
  int32_t* flags;            // [batch] or null
  int syn_bits, eh_bits;
  long long batch;
  int max_iter;              // BF
  uint32_t* queue;           // half-shot work queue (zeroed before the launch), or null = static stride
};

// `name` receives the kernel's name as rocprofv3 reports it
const void* select_hard_kernel(int algo, const char** name);
hipError_t configure_hard_kernel(const void* kernel, int lds_bytes);
hipError_t launch_hard(const void* kernel, const HardArgs& args, int grid, int block, int lds_bytes,
                       hipStream_t stream);

}  // namespace qldpc
