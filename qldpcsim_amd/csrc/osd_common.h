// osd_common.h — what the elimination kernels of osd_kernels.hip share (osd_column.h, osd_block.h, osd_hbm.h).
#pragma once
#include "osd_kernels.h"

namespace qldpc {

// a status-2 shot's posterior row into the spill buffer (OsdArgs), whole
// workgroup; `slot` is an LDS int the block may overwrite
__device__ __forceinline__ void spill_shot(const OsdArgs& a, long long shot, int n, int* slot) {
  if (!a.spill_count) return;
  if (threadIdx.x == 0) *slot = atomicAdd(a.spill_count, 1);
  __syncthreads();
  const long long q = *slot;
  if (q >= a.spill_cap) return;
  const double* src = a.post + shot * (long long)n;
  double* dst = a.spill_post + q * (long long)n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) a.spill_idx[q] = (int32_t)(a.shot_base + shot);
}

// Shots whose reliability order the device leaves to NumPy on the host
// (osd_order_kernel's tiepos -1: a NaN posterior, or x86-simd-sort's
// std::sort fallback): status 2, posteriors spilled, before any elimination.
__device__ __forceinline__ bool osd_host_shot(const OsdArgs& a, long long shot, int n, int* slot) {
  if (!a.tiepos || a.tiepos[shot] >= 0) return false;        // uniform per workgroup
  if (threadIdx.x == 0) a.status[shot] = 2;
  spill_shot(a, shot, n, slot);
  return true;
}

// s_getreg immediates: (size - 1) << 11 | offset << 6 | register id
constexpr int kHwRegHwId = (31 << 11) | 4;    // HW_ID: SIMD bits 4-5, CU 8-11, SH 12, SE 13-15
constexpr int kHwRegXccId = (31 << 11) | 20;  // XCC_ID: bits 0-3

// CPython setobject.c emulation (set_difference -> set_add_entry with
// resize; LINEAR_PROBES 9, PERTURB_SHIFT 5) for small-int keys, one thread.
__device__ int first_setdiff(int n, const unsigned char* inJ, int nJ, int* table) {
  if ((n >> 2) > nJ) {
    for (int i = 0; i < n; ++i)
      if (!inJ[i]) return i;
    return -1;
  }
  unsigned mask = 7, fill = 0, used = 0;
  for (unsigned s = 0; s <= mask; ++s) table[s] = -1;
  for (int key = 0; key < n; ++key) {
    if (inJ[key]) continue;
    unsigned perturb = (unsigned)key, i = (unsigned)key & mask;
    while (true) {
      unsigned probes = (i + 9 <= mask) ? 9 : 0, k = i;
      bool placed = false;
      while (true) {
        if (table[k] < 0) { table[k] = key; placed = true; break; }
        if (probes-- == 0) break;
        ++k;
      }
      if (placed) break;
      perturb >>= 5;
      i = (i * 5 + 1 + perturb) & mask;
    }
    ++fill;
    ++used;
    if (fill * 5 >= mask * 3) {
      const unsigned minused = used > 50000 ? used * 2 : used * 4;
      unsigned newsize = 8;
      while (newsize <= minused) newsize <<= 1;
      // re-insert (old table order) into the new one: copy old entries to the
      // upper half of the scratch first (newsize > 2*(mask+1) always here)
      int* old = table + newsize;
      for (unsigned s = 0; s <= mask; ++s) old[s] = table[s];
      for (unsigned s = 0; s < newsize; ++s) table[s] = -1;
      const unsigned nmask = newsize - 1;
      for (unsigned s = 0; s <= mask; ++s) {
        const int kk = old[s];
        if (kk < 0) continue;
        unsigned pt = (unsigned)kk, j = (unsigned)kk & nmask;
        while (true) {
          if (table[j] < 0) { table[j] = kk; break; }
          bool ok = false;
          if (j + 9 <= nmask) {
            for (int q = 0; q < 9; ++q) {
              ++j;
              if (table[j] < 0) { table[j] = kk; ok = true; break; }
            }
          }
          if (ok) break;
          pt >>= 5;
          j = (j * 5 + 1 + pt) & nmask;
        }
      }
      mask = nmask;
    }
  }
  for (unsigned s = 0; s <= mask; ++s)
    if (table[s] >= 0) return table[s];
  return -1;
}

}  // namespace qldpc
