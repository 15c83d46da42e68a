// dem_kernels.h — device shot source and outcome counter of a detector error
// model, shared with capi_dem.cpp.
//
// A DEM is N independent mechanisms; mechanism J fires with probability p_J
// and flips the detectors of column J of H [M, N] and the observables of
// column J of L [K, N]. Both kernels see the stacked matrix A = [H; L] column
// by column (CSC): the list of column J holds the bit positions its firing
// flips in a shot's row of 64 (MW + KW) bits, detector d at bit d, observable
// k at bit 64 MW + k (MW = ceil(M/64), KW = ceil(K/64)), so the detector words
// and the observable words of the row are contiguous and word-aligned.
//
// Limits (QLDPC_EUNSUP before any launch): 64 (MW + KW) <= kDemMaxRowBits,
// N <= kDemMaxColumns, and a workgroup's LDS (kDemWaves rows and the counter's
// partial sums) within the device's. The tables stay in global memory, so
// neither N, the number of edges (< 2^31) nor any row or column degree is
// bounded by LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

constexpr int kDemWaves = 4;                 // waves per workgroup (one shot per wave at a time)
constexpr int kDemCounters = 4;
constexpr int kDemMaxRowBits = 1 << 18;      // 32 KiB of LDS per wave
constexpr int kDemMaxColumns = 1 << 24;

struct DemTabs {
  const uint32_t* thr;   // [N] column J fires iff its 32-bit draw u < thr[J] (p < 1: floor(p 2^32) < 2^32)
  const int32_t* cp;     // [N + 1] column pointers into tg
  const void* tg;        // [edges] bit positions: uint16 while 64 (MW + KW) <= 65536, else uint32
  int M, K, N;
  int MW, KW, NW;        // 64-bit words of M, K, N bits
  int wide;              // tg holds uint32
};

struct DemSampleArgs {
  DemTabs t;
  uint8_t* det;          // [batch][M] bytes (det_bits: uint64 [batch][MW])
  int det_bits;
  uint64_t* obs;         // [batch][KW]
  uint64_t* fired;       // [batch][NW] the fired row; may be null
  long long batch;
  uint64_t shot0;
  uint32_t key0, key1;
};

struct DemCountArgs {
  DemTabs t;
  const uint8_t* det;    // as the sampler wrote them
  int det_bits;
  const uint64_t* obs;   // [batch][KW]
  const uint8_t* ehat;   // [batch][N] bytes (eh_bits: uint64 [batch][NW])
  int eh_bits;
  const int32_t* iters;  // [batch]
  unsigned long long* acc;  // [4] accumulated: failures, logical errors, successes, iteration sum
  uint8_t* cls;          // [batch] 0 success, 1 logical error, 2 decoder failure; may be null
  uint64_t* flips;       // [batch][KW] L ehat ^ obs; may be null
  long long batch;
};

enum DemKernel { kDemSample = 0, kDemCount = 1 };
// kind: a DemKernel (QLDPC_DEM_* of qldpc_decoder.h). The instance's name,
// "dem_sample_kernel<16>" / "dem_count_kernel<32>" (the width of a list
// entry); false for an unknown kind. No HIP call.
bool dem_kernel_name(int kind, bool wide, char* buf, int len);

// LDS bytes of a workgroup of either kernel
long long dem_lds_bytes(const DemTabs& t);
hipError_t launch_dem_sample(const DemSampleArgs& a, int grid, hipStream_t stream);
hipError_t launch_dem_count(const DemCountArgs& a, int grid, hipStream_t stream);

}  // namespace qldpc
