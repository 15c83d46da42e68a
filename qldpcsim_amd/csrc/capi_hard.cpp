// capi_hard.cpp — the hard-decision decoders' entry points (NG, BF): argument
// validation, the per-code tables and launch plan, the device launch and its
// host-buffer twin. These decoders take no schedule, prior or posteriors.

#include <cstdio>

#include "capi_internal.h"

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
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, dev));
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
    HIP_TRY(c->d_hard_queue.alloc(qldpc_code::kHardQueueSlots));
    HIP_TRY(hipMemset(c->d_hard_queue, 0, sizeof(uint32_t) * qldpc_code::kHardQueueSlots));
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
  // waves per workgroup: the width that keeps the most waves on a CU
  int best = 0;
  for (int w = qldpc::kHardMaxWaves; w >= 1; --w) {
    const int lds = w * p->args.wave_bytes;
    if (lds > max_lds) continue;
    int nb = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, p->kernel, 64 * w, (size_t)lds));
    if (nb * w > best) p->waves = w, p->blocks_per_cu = nb, p->lds = lds, best = nb * w;
  }
  if (best == 0)
    return fail(QLDPC_EUNSUP, "%s: a wave's state of %d B does not fit the %d B of LDS", p->name, p->args.wave_bytes,
                max_lds);
  return QLDPC_OK;
}

static int resolve_plan(qldpc_code* c, int algo, HardPlan* out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != c->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", c->device, dev);
  std::lock_guard<std::mutex> lk(c->hard_mu);
  HardPlan& slot = c->hard_plan[algo - QLDPC_ALGO_NG];
  const uint32_t gen = g_opt.gen.load();
  if (!slot.ok || slot.gen != gen) {
    HardPlan p{};                                     // built aside, published whole
    if (int rc = build_plan(c, algo, &p)) return rc;
    p.ok = true;
    p.gen = gen;
    slot = p;
  }
  *out = slot;
  return QLDPC_OK;
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
  if (!opt(&Options::static_sched)) {
    a.queue = code->d_hard_queue + (code->hard_qnext.fetch_add(1) % qldpc_code::kHardQueueSlots);
    HIP_TRY(hipMemsetAsync(a.queue, 0, sizeof(uint32_t), st));
  }
  const int64_t need = (batch + plan.waves - 1) / plan.waves;
  const int64_t resident = (int64_t)plan.blocks_per_cu * plan.cus;
  const int grid = (int)std::max<int64_t>(1, std::min(need, resident));
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
  std::lock_guard<std::mutex> lk(code->ws_mu);
  const int64_t m = code->m, n = code->n;
  if (int rc = ws_reserve(code, batch, false)) return rc;
  hipStream_t st = code->ws_stream;
  memcpy(code->hp_syn, h_syn, batch * m);
  HIP_TRY(hipMemcpyAsync(code->ws_syn, code->hp_syn, batch * m, hipMemcpyHostToDevice, st));
  if (int rc = qldpc_hard_decode_device(code, algo, code->ws_syn, QLDPC_FMT_BYTES, batch, max_iter, code->ws_ehat,
                                        QLDPC_FMT_BYTES, code->ws_iters, code->ws_flags, st))
    return rc;
  HIP_TRY(hipMemcpyAsync(code->hp_ehat, code->ws_ehat, batch * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_iters, code->ws_iters, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_flags, code->ws_flags, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));                  // this stream only
  memcpy(h_ehat, code->hp_ehat, batch * n);
  memcpy(h_iters, code->hp_iters, sizeof(int32_t) * batch);
  if (h_flags) memcpy(h_flags, code->hp_flags, sizeof(int32_t) * batch);
  return QLDPC_OK;
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
