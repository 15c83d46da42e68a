// phenom_kernels.h — device shot source, outcome counter and sliding-window
// step of the phenomenological noise model (multi-round space-time decoding
// of one CSS half), shared with capi_phenom.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

// CSR of the half's H (original column order), as qldpc_code holds it on the
// device, and the space-time shape it spans over `rounds` rounds.
struct PhenomTabs {
  const int32_t* rp;
  const int32_t* ci;
  int m, n, e;   // rows, columns, edges of H
  int udeg;      // row degree shared by every row of H, else 0
  int W;         // 64-bit words of an n-bit vector
  int rounds;    // T
  int N, M;      // T n + (T-1) m columns, T m detector rows
  int NW, MW;    // 64-bit words of an N-bit / M-bit vector
};

struct PhenomSampleArgs {
  PhenomTabs t;
  uint8_t* det;      // [batch][M] bytes (det_bits: uint64 [batch][MW])
  int det_bits;
  uint64_t* E;       // [batch][W] XOR of the rounds' data errors
  uint64_t* fired;   // [batch][NW] the whole fired row; may be null
  long long batch;
  uint64_t shot0;
  uint32_t key0, key1;
  uint64_t thr_data, thr_meas;  // a column fires iff its 32-bit draw u < thr
};

struct PhenomCountArgs {
  PhenomTabs t;
  const uint8_t* det;    // as the sampler wrote them
  int det_bits;
  const uint64_t* E;     // [batch][W]
  const uint8_t* ehat;   // [batch][N] bytes (eh_bits: uint64 [batch][NW])
  int eh_bits;
  const int32_t* iters;  // [batch]
  const uint64_t* tab;   // L, word-major [W][kp]: word w of logical row i at w * kp + i
  int k, kp;             // logical rows; k padded to a multiple of 64 (padding rows are zero)
  int tab_lds;           // the table is staged into LDS, else read from global memory
  unsigned long long* acc;  // [4] accumulated: failures, logical errors, successes, iteration sum
  uint8_t* cls;          // [batch] 0 success, 1 logical error, 2 decoder failure; may be null
  uint64_t* flips;       // [batch][kp / 64] L r mod 2; may be null
  uint64_t* resid;       // [batch][W] r = E ^ fold(ehat); may be null
  long long batch;
};

// One step of sliding-window decoding: commit the decoded
// window's first columns into the full estimate, add its iteration counts,
// and cut the next window's syndrome out of the detector row, its first round
// corrected by the committed measurement estimate. Every buffer is bytes or
// 64-bit words on its own flag.
struct PhenomWindowArgs {
  int n, m;              // H's shape
  int N, M;              // the full space-time shape (T rounds)
  // the window just decoded (has_done), already checked against [0, T)
  int has_done;
  int commit_off;        // a (n+m): first destination column
  int commit_len;        // committed columns: C (n+m), closed: R n + (R-1) m
  int west_len;          // the window estimate's columns N_w
  int corr_off;          // (C-1) (n+m) + n: the committed measurement estimate u_{a'-1} in west
  const uint8_t* west;   // [batch][west_len] bytes (west_bits: uint64 [batch][ceil(west_len/64)])
  int west_bits;
  const int32_t* witers; // [batch]
  uint8_t* ehat;         // [batch][N] bytes (eh_bits: uint64 [batch][ceil(N/64)]), merged in place
  int eh_bits;
  int32_t* iters;        // [batch] += witers
  // the next window (has_next)
  int has_next;
  int syn_off;           // a' m: first detector of the next window
  int syn_len;           // R' m
  const uint8_t* det;    // [batch][M] bytes (det_bits: uint64 [batch][ceil(M/64)])
  int det_bits;
  uint8_t* syn;          // [batch][syn_len] bytes (syn_bits: uint64 [batch][ceil(syn_len/64)])
  int syn_bits;
  long long batch;
};

constexpr int kPhenomWaves = 4;  // waves per workgroup (one shot per wave at a time)
constexpr int kPhenomCounters = 4;

// Which instantiation of the sampler and the counter runs a half: H's row
// degree if every row has it and it is 6, 7 or 8 (unrolled row reads), else 0
// (generic CSR loop). No HIP call; the launchers and qldpc_phenom_kernel_name
// read it.
int phenom_choice(const PhenomTabs& t);
enum PhenomKernel { kPhenomSample = 0, kPhenomCount = 1 };
// kind: a PhenomKernel (QLDPC_PHENOM_* of qldpc_decoder.h). The name of that
// kernel's instance, "phenom_count_kernel<8>"; false for an unknown kind.
bool phenom_kernel_name(int kind, int deg, char* buf, int len);

// LDS bytes of a workgroup of each kernel
long long phenom_sample_lds_bytes(const PhenomTabs& t);
long long phenom_count_lds_bytes(const PhenomTabs& t, int kp, bool tab_lds);
hipError_t launch_phenom_sample(const PhenomSampleArgs& a, int grid, hipStream_t stream);
hipError_t launch_phenom_count(const PhenomCountArgs& a, int grid, hipStream_t stream);
hipError_t launch_phenom_window(const PhenomWindowArgs& a, int grid, hipStream_t stream);

}  // namespace qldpc
