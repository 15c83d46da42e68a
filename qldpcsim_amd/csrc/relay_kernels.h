// relay_kernels.h — relay min-sum: shared between
// relay_kernels.hip and the C-ABI host code (capi_relay.cpp).
#pragma once
#include "decoder_kernels.h"

namespace qldpc {

// relay_ms_kernel's arguments: the generic LDS kernel's (the graph image, the
// formats, the outputs, L / beta and the queue; max_iter is unread) and its
// own behind them, so DecodeArgs and every kernel taking it stay as they are.
// Per-wave slice: X f64[n] (what the check nodes read) | c2v f32[E + 8] |
// syndrome words | M f64[n] (posteriors) | hard-decision words | best-solution
// words; the words are 2 ceil(n / 64) (2 ceil(m / 64) for the syndrome).
struct RelayArgs {
  DecodeArgs d;
  const double* gamma;        // [legs][n] memory strengths, relabeled variable order (global)
  const int32_t* leg_iters;   // [legs] iteration counts (global)
  int legs, sols;
  int off_m, off_ew, off_best;  // inside a wave slice (X at 0, d.off_c2v, d.off_synw)
  int32_t* info;              // [batch][2] (found, best_leg or -1), or null
};

// relay_ms_kernel<dc> for dc = 0 (any row degrees <= 32), 7, 8
const void* select_relay_kernel(int dc, const char** name);
hipError_t launch_relay(const void* kernel, const RelayArgs& args, int grid, int block, int lds_bytes,
                        hipStream_t stream);
hipError_t configure_relay_kernel(const void* kernel, int lds_bytes);

// relay_vprior_kernel's arguments: relay_ms_kernel's, with
// the prior row in d.vprior / d.vprior_bytes as decode_vprior_kernel takes it
// (staged into LDS between the graph image and the wave slices; d.L is
// unread), and the solution cost behind them.
struct RelayVpriorArgs {
  RelayArgs r;
  const long long* wgt;       // [n] W_j = llrint(L_j 2^20), relabeled variable order (global)
  int cost;                   // 0: a solution weighs its set bits, 1: the sum of wgt over them
};

// relay_vprior_kernel<dc>, chosen as relay_ms_kernel<dc> is
const void* select_relay_vprior_kernel(int dc, const char** name);
hipError_t launch_relay_vprior(const void* kernel, const RelayVpriorArgs& args, int grid, int block, int lds_bytes,
                               hipStream_t stream);

}  // namespace qldpc
