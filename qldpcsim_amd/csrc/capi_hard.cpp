// capi_hard.cpp — the hard-decision decoders' entry points (NG, BF): argument
// validation, the per-code tables, LDS layout and launch plan, the device
// launch and its host-buffer twin. These decoders take no schedule, prior or
// posteriors. The plumbing shared with the other families is in capi_launch.h.

#include <cstdio>

#include "capi_launch.h"

using namespace capi;
using qldpc::HardArgs;

static bool is_hard(int algo) { return algo == QLDPC_ALGO_NG || algo == QLDPC_ALGO_BF; }

// per-wave slice: [BF: syndrome words | NG: scores u16[npad]] | residual words | estimate words
int capi::hard_layout(const qldpc_code* c, int algo, HardArgs* a) {
  if (!c->lds_ok)
    return fail(QLDPC_EUNSUP,
                "%s decoder: %d x %d with %d edges is past the kernels' 16-bit tables (m, n, edges <= 65535)",
                algo == QLDPC_ALGO_NG ? "NG" : "BF", c->m, c->n, c->E);
  a->m = c->m, a->n = c->n;
  a->wm = (c->m + 63) / 64, a->wn = (c->n + 63) / 64;
  a->npad = (c->n + 127) & ~127;
  const int rbytes = 8 * a->wm, ebytes = 8 * a->wn;
  int off = align16(algo == QLDPC_ALGO_NG ? 2 * a->npad : rbytes);
  a->off_res = off;
  off = align16(off + rbytes);
  a->off_est = off;
  a->wave_bytes = align16(off + ebytes);
  return QLDPC_OK;
}

// everything before the first HIP call; *done: nothing to launch
static int validate(const qldpc_code* code, int algo, int syn_format, int ehat_format, int64_t batch, int max_iter,
                    const void* syn, const void* ehat, const int32_t* iters, bool* done) {
  *done = false;
  if ((syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (!is_hard(algo)) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (algo == QLDPC_ALGO_BF && max_iter < 1) return fail(QLDPC_EINVAL, "max_iter must be >= 1");
  if (code->m == 0 || code->n == 0) return fail(QLDPC_EINVAL, "empty parity-check matrix");
  HardArgs a{};
  if (int rc = hard_layout(code, algo, &a)) return rc;
  if (batch == 0) {
    *done = true;
    return QLDPC_OK;
  }
  if (!syn || !ehat || !iters) return fail(QLDPC_EINVAL, "null buffer");
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  return QLDPC_OK;
}

static int build_plan(qldpc_code* c, int algo, HardPlan* p) {
  int max_lds = 0;
  if (int rc = device_limits(&max_lds, &p->cus)) return rc;
  if (!c->d_hard_tab) {
    // row_ell [m][8] | col_ell [n][8] | row_ptr | row_var | col_ptr | col_chk
    const int m = c->m, n = c->n, E = c->E;
    std::vector<int32_t> cp(n + 1, 0);
    for (int e = 0; e < E; ++e) cp[c->col_idx[e] + 1]++;
    for (int j = 0; j < n; ++j) cp[j + 1] += cp[j];
    std::vector<int32_t> fill(cp.begin(), cp.end() - 1);
    std::vector<uint16_t> chk(E);
    for (int r = 0; r < m; ++r)                      // ascending rows: each column's checks ascend
      for (int e = c->row_ptr[r]; e < c->row_ptr[r + 1]; ++e) chk[fill[c->col_idx[e]]++] = (uint16_t)r;
    std::vector<uint16_t> tab((size_t)8 * (m + n), 0);
    for (int r = 0; r < m; ++r)
      for (int e = c->row_ptr[r], k = 0; e < c->row_ptr[r + 1] && k < 8; ++e, ++k)
        tab[(size_t)8 * r + k] = (uint16_t)c->col_idx[e];
    for (int j = 0; j < n; ++j)
      for (int e = cp[j], k = 0; e < cp[j + 1] && k < 8; ++e, ++k) tab[(size_t)8 * (m + j) + k] = chk[e];
    tab.insert(tab.end(), c->row_ptr.begin(), c->row_ptr.end());
    tab.insert(tab.end(), c->col_idx.begin(), c->col_idx.end());
    tab.insert(tab.end(), cp.begin(), cp.end());
    tab.insert(tab.end(), chk.begin(), chk.end());
    HIP_TRY(c->d_hard_tab.upload(tab));
    HIP_TRY(c->hard_queue.buf.alloc(QueueRing::kSlots));
    HIP_TRY(hipMemset(c->hard_queue.buf, 0, sizeof(uint32_t) * QueueRing::kSlots));
  }
  if (int rc = hard_layout(c, algo, &p->args)) return rc;
  p->args.row_ell = c->d_hard_tab;
  p->args.col_ell = p->args.row_ell + (size_t)8 * c->m;
  p->args.row_ptr = p->args.col_ell + (size_t)8 * c->n;
  p->args.row_var = p->args.row_ptr + c->m + 1;
  p->args.col_ptr = p->args.row_var + c->E;
  p->args.col_chk = p->args.col_ptr + c->n + 1;
  p->kernel = qldpc::select_hard_kernel(algo, &p->name);
  HIP_TRY(qldpc::configure_hard_kernel(p->kernel, max_lds));
  // waves per workgroup: the width that keeps the most waves on a CU (the
  // tuning options waves_per_wg, wg_per_cu have no say here)
  auto lds_of = [&](int w) { return w * p->args.wave_bytes; };
  WaveChoice wc;
  HIP_TRY(wave_search(1, qldpc::kHardMaxWaves, max_lds, lds_of, occupancy_of(p->kernel), false, &wc));
  if (!wc.waves)
    return fail(QLDPC_EUNSUP, "%s: a wave's state of %d B does not fit the %d B of LDS", p->name, p->args.wave_bytes,
                max_lds);
  p->waves = wc.waves, p->blocks_per_cu = wc.blocks_per_cu, p->lds = wc.lds;
  return QLDPC_OK;
}

static int resolve_plan(qldpc_code* c, int algo, HardPlan* out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != c->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", c->device, dev);
  return cached_plan(c->hard_mu, c->hard_plan[algo - QLDPC_ALGO_NG], out,
                     [&](HardPlan* p) { return build_plan(c, algo, p); });
}

extern "C" int qldpc_hard_decode_device(const qldpc_code* code_c, int algo, const void* d_syn, int syn_format,
                                        int64_t batch, int max_iter, void* d_ehat, int ehat_format, int32_t* d_iters,
                                        int32_t* d_flags, void* stream) {
  auto* code = const_cast<qldpc_code*>(code_c);
  bool done = false;
  if (int rc = validate(code, algo, syn_format, ehat_format, batch, max_iter, d_syn, d_ehat, d_iters, &done)) return rc;
  if (done) return QLDPC_OK;
  HardPlan plan;
  if (int rc = resolve_plan(code, algo, &plan)) return rc;
  hipStream_t st = (hipStream_t)stream;
  HardArgs a = plan.args;
  a.syn = d_syn, a.ehat = d_ehat, a.iters = d_iters, a.flags = d_flags;
  a.syn_bits = syn_format == QLDPC_FMT_BITS, a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.batch = batch;
  a.max_iter = max_iter;
  a.queue = nullptr;
  if (!opt(&Options::static_sched))
    if (int rc = code->hard_queue.claim(st, &a.queue)) return rc;
  const int grid = launch_grid(batch, plan.waves, plan.blocks_per_cu, plan.cus);
  TimedLaunch t;
  if (int rc = timing_begin(&t, st)) return rc;
  HIP_TRY(qldpc::launch_hard(plan.kernel, a, grid, 64 * plan.waves, plan.lds, st));
  return timing_end(&t, st);
}

extern "C" int qldpc_hard_decode_host(const qldpc_code* code_c, int algo, const uint8_t* h_syn, int64_t batch,
                                      int max_iter, uint8_t* h_ehat, int32_t* h_iters, int32_t* h_flags) {
  auto* code = const_cast<qldpc_code*>(code_c);
  bool done = false;
  if (int rc = validate(code, algo, QLDPC_FMT_BYTES, QLDPC_FMT_BYTES, batch, max_iter, h_syn, h_ehat, h_iters, &done))
    return rc;
  if (done) return QLDPC_OK;
  return staged_call(code, host_io(h_syn, batch, h_ehat, h_iters, nullptr, h_flags), [&](const CallIO& d, hipStream_t st) {
    return qldpc_hard_decode_device(code, algo, d.syn, d.syn_format, batch, max_iter, d.ehat, d.ehat_format, d.iters,
                                    d.flags, st);
  });
}

extern "C" int qldpc_hard_kernel_name(const qldpc_code* code, int algo, char* buf, int len) {
  if (!code || !buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  if (!is_hard(algo)) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  HardArgs a{};
  if (int rc = hard_layout(code, algo, &a)) return rc;
  const char* name = "";
  (void)qldpc::select_hard_kernel(algo, &name);
  snprintf(buf, (size_t)len, "%s", name);
  return QLDPC_OK;
}

extern "C" int qldpc_hard_launch_info(const qldpc_code* code_c, int algo, int* waves_per_wg, int* wg_per_cu,
                                      int* lds_bytes) {
  auto* code = const_cast<qldpc_code*>(code_c);
  if (!code || !waves_per_wg || !wg_per_cu || !lds_bytes) return fail(QLDPC_EINVAL, "null argument");
  if (!is_hard(algo)) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  if (code->m == 0 || code->n == 0) return fail(QLDPC_EINVAL, "empty parity-check matrix");
  HardArgs a{};
  if (int rc = hard_layout(code, algo, &a)) return rc;
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  HardPlan plan;
  if (int rc = resolve_plan(code, algo, &plan)) return rc;
  *waves_per_wg = plan.waves;
  *wg_per_cu = plan.blocks_per_cu;
  *lds_bytes = plan.lds;
  return QLDPC_OK;
}
