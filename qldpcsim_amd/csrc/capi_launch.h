// capi_launch.h — what every decoder family's host path does around its
// kernel launch (capi_decode.cpp, capi_relay.cpp, capi_hard.cpp): the device's
// limits, the occupancy search over workgroup widths, the launch-plan cache,
// the grid size, which limit keeps the LDS kernels from a code, launch timing
// and the host staging round trip. Private to capi*.cpp.
#pragma once
#include "capi_internal.h"

#pragma GCC visibility push(hidden)
namespace capi {

// The current device's LDS bytes per workgroup and compute units, and (if asked) which device it is
int device_limits(int* max_lds, int* cus, int* dev = nullptr);

// The workgroup width in [lo, hi] waves that keeps the most waves on a CU, on
// ties the wider one; a width whose lds_of(w) is past max_lds is skipped without
// a query; zeros when none fits. An error of occupancy(w, lds, &blocks) ends the
// search. `overrides`: the tuning options apply (experiments, tests) —
// waves_per_wg if it lies in [lo, hi], fits, and its query gives blocks > 0;
// wg_per_cu only lowers blocks_per_cu, never below 1.
struct WaveChoice { int waves = 0, blocks_per_cu = 0, lds = 0; };
template <typename LdsOf, typename Occupancy>
hipError_t wave_search(int lo, int hi, int max_lds, LdsOf lds_of, Occupancy occupancy, bool overrides,
                       WaveChoice* out) {
  *out = WaveChoice{};
  for (int w = hi; w >= lo; --w) {
    const int lds = lds_of(w);
    if (lds > max_lds) continue;
    int nb = 0;
    if (hipError_t e = occupancy(w, lds, &nb)) return e;
    if (nb * w > out->blocks_per_cu * out->waves) *out = WaveChoice{w, nb, lds};
  }
  if (!overrides) return hipSuccess;
  if (const int w = (int)opt(&Options::waves_per_wg); w >= lo && w <= hi) {
    const int lds = lds_of(w);
    int nb = 0;
    if (lds <= max_lds && occupancy(w, lds, &nb) == hipSuccess && nb > 0) *out = WaveChoice{w, nb, lds};
  }
  if (const int k = (int)opt(&Options::wg_per_cu); k >= 1 && k < out->blocks_per_cu) out->blocks_per_cu = k;
  return hipSuccess;
}
// the query of the three families: hipOccupancyMaxActiveBlocksPerMultiprocessor on `kernel`
inline auto occupancy_of(const void* kernel) {
  return [kernel](int w, int lds, int* nb) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, kernel, 64 * w, (size_t)lds);
  };
}

// The one way to a cached plan: built aside under the owner's lock, published
// whole, rebuilt when an option changed (g_opt.gen); *out is the launch's own
// snapshot. A failing build(&plan) leaves the slot as it was.
template <typename Plan, typename Build>
int cached_plan(std::mutex& mu, Plan& slot, Plan* out, Build build) {
  std::lock_guard<std::mutex> lk(mu);
  const uint32_t gen = g_opt.gen.load();
  if (!slot.ok || slot.gen != gen) {
    Plan p{};
    if (int rc = build(&p)) return rc;
    p.ok = true, p.gen = gen;
    slot = p;
  }
  *out = slot;
  return QLDPC_OK;
}

// Workgroups of a launch: what the batch fills at `per_block` half-shots each, at most the resident ones, at least one
inline int launch_grid(int64_t batch, int64_t per_block, int blocks_per_cu, int cus) {
  return (int)std::max<int64_t>(1, std::min((batch + per_block - 1) / per_block, (int64_t)blocks_per_cu * cus));
}

// Which limit, if any, keeps the LDS-resident kernels from decoding `c` with
// `algo` (relay min-sum: QLDPC_ALGO_MS), tested in this order; `lds_ok` is the
// code's or the schedule's. Each caller words its own message. No HIP call.
enum LdsLimit { LDS_FITS = 0, LDS_TABLES16, LDS_MS_ROW_DEG, LDS_BP_COL_DEG, LDS_FORCE_HBM };
LdsLimit lds_limit(bool lds_ok, const qldpc_code* c, int algo);

// HIP events around a kernel launch when qldpc_timing_enable is on
struct TimedLaunch { hipEvent_t e0 = nullptr, e1 = nullptr; };
int timing_begin(TimedLaunch* t, hipStream_t st);
int timing_end(TimedLaunch* t, hipStream_t st);

// One call's buffers, device or host: syndromes in; estimates, iterations, flags and optional posteriors out
struct CallIO {
  const void* syn; int syn_format; int64_t batch;
  void* ehat; int ehat_format; int32_t *iters, *flags; double* post;
};
// a host entry point's buffers: bytes both ways
inline CallIO host_io(const uint8_t* syn, int64_t batch, uint8_t* ehat, int32_t* iters, double* post, int32_t* flags) {
  return {syn, QLDPC_FMT_BYTES, batch, ehat, QLDPC_FMT_BYTES, iters, flags, post};
}
// the per-call I/O fields of a kernel's DecodeArgs
inline void set_call_io(qldpc::DecodeArgs* a, const CallIO& io) {
  a->syn = (const uint8_t*)io.syn, a->ehat = (uint8_t*)io.ehat;
  a->syn_bits = io.syn_format == QLDPC_FMT_BITS, a->eh_bits = io.ehat_format == QLDPC_FMT_BITS;
  a->iters = io.iters, a->post = io.post, a->flags = io.flags;
  a->batch = io.batch;
}

// A decode from and to the host buffers `h` (bytes) through the code's staging
// workspace, under ws_mu: stage_in grows it and sends h.syn through its pinned
// mirror on ws_stream; launch(d, stream) enqueues the decode on the workspace's
// device buffers `d`; stage_out copies the results back, waits for that stream
// alone and fills h; after(), if given, runs last.
int stage_in(qldpc_code* code, const CallIO& h, CallIO* d);
int stage_out(qldpc_code* code, const CallIO& h);
template <typename Launch, typename After = int (*)()>
int staged_call(qldpc_code* code, const CallIO& h, Launch launch, After after = [] { return (int)QLDPC_OK; }) {
  std::lock_guard<std::mutex> lk(code->ws_mu);
  CallIO d{};
  if (int rc = stage_in(code, h, &d)) return rc;
  if (int rc = launch(d, code->ws_stream)) return rc;
  if (int rc = stage_out(code, h)) return rc;
  return after();
}

}  // namespace capi
#pragma GCC visibility pop
