// channel_kernels.h — device depolarizing sampler and outcome counters
// (simulate_p's shot source and counters), shared with capi_channel.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

// CSR of Hx and Hz (original column order), as qldpc_code holds them on the device.
struct PairTabs {
  const int32_t* rp_x;
  const int32_t* ci_x;
  const int32_t* rp_z;
  const int32_t* ci_z;
  int mx, mz, ex, ez;  // rows and edges of Hx / Hz
  int n, W;            // qubits, 64-bit words per packed error vector
  int udeg;            // row degree shared by every row of Hx and Hz, else 0
};

struct SampleArgs {
  PairTabs t;
  uint64_t* errx;  // [batch][W]
  uint64_t* errz;  // [batch][W]
  uint8_t* syz;    // [batch][mz]  Hz errX mod 2 (syn_bits: uint64 [batch][ceil(mz/64)])
  uint8_t* syx;    // [batch][mx]  Hx errZ mod 2
  int syn_bits;
  long long batch;
  uint64_t shot0;
  uint32_t key0, key1;
  uint64_t t1, t2, t3;  // X: u < t1, Y: t1 <= u < t2, Z: t2 <= u < t3 (u a 32-bit draw)
};

// channel_sample_vec_kernel: the same stream with thresholds per qubit
struct SampleVecArgs {
  SampleArgs s;         // s.t1 .. s.t3 unread
  const uint64_t* thr;  // [3][n]: T1_j, T2_j, T3_j (each <= 2^32), original qubit order
};

struct CountArgs {
  PairTabs t;
  const uint64_t* errx;  // [batch][W]
  const uint64_t* errz;
  const uint8_t* syz;    // [batch][mz]
  const uint8_t* syx;    // [batch][mx]
  const uint8_t* ehx;    // [batch][n] X-half estimate (decodes Hz)
  const uint8_t* ehz;    // [batch][n] Z-half estimate (decodes Hx)
  int syn_bits, eh_bits; // uint64 words instead of bytes (bit j % 64 of word j / 64)
  const int32_t* itx;    // [batch]
  const int32_t* itz;
  unsigned long long* acc;  // [6] accumulated
  long long batch;
};

// count_logical_kernel: the six counters of CountArgs plus the stabiliser-group
// test of the residuals against the pair's logical operators.
struct LogicalArgs {
  CountArgs c;             // c.acc: [9] accumulated (the six, then logX, logZ, success)
  const uint64_t* tab_z;   // Lz, word-major [W][kp]: word w of logical row i at w * kp + i (tests errX ^ eX)
  const uint64_t* tab_x;   // Lx, the same layout (tests errZ ^ eZ)
  int k, kp;               // logical qubits; k padded to a multiple of 64 (padding rows are zero)
  int tabs_lds;            // both tables staged into LDS, else read from global memory
  uint8_t* class_x;        // [batch] 0 success, 1 logical error, 2 decoder failure; may be null
  uint8_t* class_z;
  uint64_t* flip_x;        // [batch][kp / 64] Lz (errX ^ eX) mod 2, bit i % 64 of word i / 64; may be null
  uint64_t* flip_z;        // [batch][kp / 64] Lx (errZ ^ eZ) mod 2
};

constexpr int kChannelWaves = 4;  // waves per workgroup (one shot per wave at a time)
constexpr int kLogicalCounters = 9;

// Which instantiation runs a pair: all that the row degrees, n, the estimates'
// alignment and the table residency decide, without a HIP call; the launchers
// and qldpc_channel_kernel_name read it.
//   deg   the row degree shared by every row of Hx and Hz if it is 6, 7 or 8
//         (unrolled row reads), else 0 (generic CSR loop)
//   vec   counters: byte estimates read by 32-bit loads, which need every row
//         4-byte aligned (n % 4 == 0) and both bases 4-byte aligned
//   tlds  count_logical_kernel: both logical tables staged into LDS
struct ChannelChoice {
  int deg;
  bool vec, tlds;
};
ChannelChoice channel_choice(const PairTabs& t, bool est_aligned, bool tabs_lds);
enum ChannelKernel { kChannelSample = 0, kChannelSampleVec = 1, kChannelCount = 2, kChannelCountLogical = 3 };
// kind: a ChannelKernel (QLDPC_CHANNEL_* of qldpc_decoder.h). The name of that kernel's instance,
// "count_logical_kernel<6, true, false>"; false for an unknown kind.
bool channel_kernel_name(int kind, const ChannelChoice& c, char* buf, int len);

// LDS bytes the two kernels need for these tables
int channel_lds_bytes(const PairTabs& t, bool counters);
// LDS bytes of count_logical_kernel, with both logical tables staged or not
int logical_lds_bytes(const PairTabs& t, int kp, bool tabs_lds);
hipError_t launch_channel_sample(const SampleArgs& a, int grid, hipStream_t stream);
hipError_t launch_channel_sample_vec(const SampleVecArgs& a, int grid, hipStream_t stream);
hipError_t launch_count_outcomes(const CountArgs& a, int grid, hipStream_t stream);
hipError_t launch_count_logical(const LogicalArgs& a, int grid, hipStream_t stream);

}  // namespace qldpc
