// osd_kernels.h — batched GPU OSD (decoders.py:299-370): what osd_kernels.hip
// shares with capi_osd_device.cpp — argument structs, selectors, LDS sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tuning.h"

namespace qldpc {

struct OsdArgs {
  const int32_t* row_ptr;  // [m+1] CSR of H (original columns)
  const int32_t* col_idx;  // [E]
  const int32_t* perm;     // [count][n] reliability order (NumPy argsort, decoders.py:325)
  const uint8_t* syn;      // [count][m]
  uint8_t* ehat;           // [count][n] in/out
  int32_t* status;         // [count] 0 ok, 1 = reference IndexError case, 2 = order left to the host
                           // (3 = internal: osd_block_kernel hands the shot to osd_kernel)
  const int32_t* tiepos;   // [count] or null: osd_order_kernel's verdict; -1 = the order is
                           // left to NumPy on the host: the shot is left untouched (status 2)
  const double* post;      // [count][n] posteriors (spilled for status-2 shots), with tiepos
  int m, n, rank, order;
  // status-2 spill (optional): a shot left to the host also copies its
  // posterior row to spill_post[slot] and its index to spill_idx[slot],
  // slot = atomicAdd(spill_count, 1) (< spill_cap), so the host can fetch
  // exactly those rows with one DMA copy, no gather kernel
  double* spill_post;      // [spill_cap][n]
  int32_t* spill_idx;      // [spill_cap] shot index within the call
  int32_t* spill_count;    // [1]
  long long spill_cap, shot_base;
  unsigned long long* prof; // QLDPC_OSD_TIMING builds only: per-phase cycle sums
  uint32_t* cu_tickets;    // [kOsdCuSlots] per-CU workgroup tickets (engine SIMD choice), or null
  int redo;                // osd_kernel only: process just the shots whose status is 3
                           // (left by osd_block_kernel: syndrome outside H's column space)
  int cs_lambda;           // osd_block_kernel's OSD-CS instances only: pairs among the first
                           // min(cs_lambda, |T|) information positions (0 .. 64); `order` is 0
  const int64_t* cs_w;     // osd_block_cs_prior_kernel only: weight of each original column
                           // (qldpc_prior::d_Wo, |w| < 2^30), the cost in place of the Hamming weight
};

// Reliability order on the device (decoders.py:320-325): NumPy's exact order
// (osd_order_kernel); tiepos = n, or -1 where the host's NumPy must decide.
struct OrderArgs {
  const double* post;      // [count][n]
  int32_t* perm;           // [count][n]
  int32_t* tiepos;         // [count]
  int n;                   // <= 2048
};
constexpr int kOsdCuSlots = 16 * 256;  // XCC id (4 bits) x HW_ID bits 8-15 (CU, SH, SE)
hipError_t launch_osd_order(const OrderArgs& a, long long count, hipStream_t stream);
size_t osd_order_lds(int n);

// osd_hbm_kernel (any m, n): each shot's working matrix lives in a global
// scratch slice instead of VGPRs / LDS. Per shot, at `scratch + shot *
// stride` (shot = the launch's blockIdx.x): R [nwr][mp] u64 (word-major: word
// q of the row at REF position p at q * mp + p; nwr = ceil((n + 1) / 64), mp =
// m rounded up to 64), then inv_perm [n] i32 at off_inv, the J list [m + 2]
// i32 at off_jl, inJ [n] bytes at off_inj and the CPython set table (order 1)
// at off_table. LDS: the current word of every row [mp] u64 + 3 [nwr] u64 + 160 B.
struct OsdHbmArgs {
  unsigned char* scratch;
  long long stride;
  int nwr, mp, off_inv, off_jl, off_inj, off_table;
};
inline size_t osd_hbm_lds(int m, int nwr) { return 8 * (size_t)((m + 63) / 64 * 64) + 24 * (size_t)nwr + 160; }

// Selectors: the kernel, and through `name` (may be null) its name as
// rocprofv3 prints it. nw = the NW instance for a row of `words` 64-bit words
// incl. the syndrome column (osd_nw_of; 0 past 33 words).
int osd_nw_of(int words);
const void* osd_hbm_kernel_ptr(const char** name);   // __global__ osd_hbm_kernel(OsdArgs, OsdHbmArgs)
const void* select_osd_kernel(int nw, const char** name);
// block elimination (the default), or null: osd_kernel runs alone. cs: 0 order 0 / 1, kOsdCsHamming or
// kOsdCsPrior the OSD-CS instance of that cost
constexpr int kOsdCsHamming = 1, kOsdCsPrior = 2;
const void* select_osd_block_kernel(int nw, int m, int cs, int* rows_per_thread, const char** name);

// Dynamic LDS bytes of osd_kernel<nw> and osd_block_kernel<nw, ..>: one term per array, in the order the
// kernels carve them (osd_column.h, osd_block_body.inc). mr = the block kernel's row slots, table_ints =
// CPython's set table (order 1, else 0). Both start with inv_perm [n] i32 | J list [m + 2] i32 | inJ [n] bytes:
inline size_t osd_head_lds(size_t m, size_t n) { return (4 * n + 4 * (m + 2) + n + 15) & ~(size_t)15; }
inline size_t osd_column_lds(int m, int n, size_t nw, size_t table_ints) {
  return osd_head_lds(m, n) + 8 * nw               // emask [NW] u64
         + 8 * 2 * 16 * nw + 8 * 2 * nw            // candidate rows [2][16][NW], xrow rows [2][NW] u64
         + 4 * 32 + 4 * 4                          // candidate ids [2][16], misc [4] i32
         + 4 * table_ints;                         // set table
}
// the block loop's arrays, which the OSD-CS epilogue reuses (osd_cs_lds bytes of them: osd_cs_epilogue's carve)
inline size_t osd_block_cs_room(size_t nw, size_t mr) {
  return 8 * mr + 8 * mr                           // Wd [MR], Cm [MR] u64
         + 8 * 64 * nw + (QLDPC_OSD_PAIRS ? 8 * 32 * nw : 0) + 8 * 64;   // PW [64][NW], PX [32][NW], CT [64] u64
}
inline size_t osd_cs_lds(int nw, int mr) { return 8 * (size_t)mr + (size_t)mr / 8 + 264 * (size_t)nw + 272; }
// osd_cs_prior_epilogue's carve of the same room: colv [64][MR / 64] u64 | cnt [64 NW] i64 | tmask [NW] u64 |
// red [2] u64 | sw [MR] i32 | tl [64] i32
inline size_t osd_cs_prior_lds(int nw, int mr) { return 12 * (size_t)mr + 520 * (size_t)nw + 272; }
inline size_t osd_block_lds(int m, int n, size_t nw, size_t mr, size_t table_ints) {
  return osd_head_lds(m, n) + 8 * nw               // emask [NW] u64
         + osd_block_cs_room(nw, mr)               // Wd | Cm | PW | PX | CT
         + 4 * 3 * mr + 4 * 64 + 4 * 16            // pkof, pidx, crow [MR], pk [64], misc [16] i32
         + 4 * table_ints;                         // set table
}

}  // namespace qldpc
