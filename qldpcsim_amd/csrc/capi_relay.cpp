// capi_relay.cpp — relay min-sum: the qldpc_relay handle
// (legs, memory strengths, a flooding schedule of its own), its launch plans
// and the decode entry points, the scalar-prior ones (relay_ms_kernel) and
// the per-variable-prior ones (relay_vprior_kernel, §3.18).

#include <cmath>
#include <cstdio>
#include <memory>

#include "capi_internal.h"
#include "relay_kernels.h"
#include "../../include/qldpc_libm.h"   // after hip_runtime.h

using namespace capi;
using qldpc::RelayArgs;
using qldpc::RelayVpriorArgs;

namespace {

struct RelayPlan {
  const void* kernel = nullptr;
  const char* name = "";
  int waves = 0, blocks_per_cu = 0, lds = 0, cus = 0;
  RelayArgs args{};          // every static field filled
  uint32_t gen = 0;
  bool ok = false;
};

}  // namespace

struct qldpc_relay {
  const qldpc_code* code = nullptr;
  qldpc_schedule* sched = nullptr;       // flooding: the generic table image and the queue ring
  int legs = 0, sols = 0;
  std::vector<int32_t> leg_iters;
  std::vector<double> gamma;             // [legs][n], relabeled variable order
  DevBuf<int32_t> d_leg_iters;
  DevBuf<double> d_gamma;
  std::mutex mu;                         // the plan, and the host path's info buffer
  RelayPlan plan[2];                     // [0] relay_ms_kernel, [1] relay_vprior_kernel
  DevBuf<int32_t> ws_info;
  int64_t ws_info_cap = 0;
  ~qldpc_relay() { qldpc_schedule_destroy(sched); }
};

// ---------------------------------------------------------------------------
// device-free half: limits, kernel, static arguments (no HIP function called)
// ---------------------------------------------------------------------------
static int relay_limits(const qldpc_code* c) {
  if (!c->lds_ok)
    return fail(QLDPC_EUNSUP, "relay min-sum: %d x %d with %d edges is past the LDS kernel's 16-bit tables "
                "(m, n, edges <= 65535); there is no HBM-resident variant", c->m, c->n, c->E);
  if (c->max_row_deg > 32)
    return fail(QLDPC_EUNSUP, "relay min-sum: row degree %d > 32 has no LDS kernel", c->max_row_deg);
  if (opt(&Options::force_hbm) != 0)
    return fail(QLDPC_EUNSUP, "relay min-sum: option force_hbm is set and there is no HBM-resident variant");
  return QLDPC_OK;
}

// `vp`: relay_vprior_kernel, the same instance of it
static const void* relay_choose(const qldpc_code* c, bool vp, const char** name) {
  return (vp ? qldpc::select_relay_vprior_kernel : qldpc::select_relay_kernel)(fast_table_ok(c) ? c->uniform_deg : 0,
                                                                              name);
}

// X f64[n] | c2v f32[E + 8] | syndrome words | M f64[n] | hard-decision words | best-solution words;
// `vp`: the prior row f64[n] between the image and the slices, counted in the
// bytes returned, the slices as without it
static int relay_plan_static(const qldpc_relay* r, bool vp, RelayArgs* ra) {
  const qldpc_code* c = r->code;
  const TableImage& t = r->sched->generic;
  qldpc::DecodeArgs& a = ra->d;
  a.blob = t.dev;
  a.blob_bytes = t.lds_bytes;
  a.off_cn_tab = t.off.cn_tab, a.off_row_ptr = t.off.row_ptr, a.off_vn_ptr = t.off.vn_ptr;
  a.off_chunk_dmax = t.off.chunk_dmax;
  a.m = c->m, a.n = c->n, a.E = c->E, a.n_layers = 1;
  a.wm = (c->m + 63) / 64, a.wn = (c->n + 63) / 64;
  a.vinv = c->d_vinv;
  int off = align16(8 * c->n);
  a.off_c2v = off;
  off = align16(off + 4 * (c->E + 8));              // +8: VN over-read pad
  a.off_synw = off;
  off = align16(off + 4 * 2 * a.wm);
  ra->off_m = off;
  off = align16(off + 8 * c->n);
  ra->off_ew = off;
  off = align16(off + 4 * 2 * a.wn);
  ra->off_best = off;
  off = align16(off + 4 * 2 * a.wn);
  a.wave_bytes = std::max(off, 16);
  ra->gamma = r->d_gamma, ra->leg_iters = r->d_leg_iters;
  ra->legs = r->legs, ra->sols = r->sols;
  a.vprior_bytes = vp ? align16(8 * c->n) : 0;
  return t.lds_bytes + a.vprior_bytes;
}

// ---------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------
extern "C" int qldpc_relay_create(const qldpc_code* code, int legs, const int32_t* h_leg_iters, const double* h_gamma,
                                  int n_gamma, int sols, qldpc_relay** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (legs < 1) return fail(QLDPC_EINVAL, "relay min-sum: at least one leg (got %d)", legs);
  if (!h_leg_iters || !h_gamma) return fail(QLDPC_EINVAL, "relay min-sum: null leg_iters / gamma");
  if (sols < 1) return fail(QLDPC_EINVAL, "relay min-sum: sols must be >= 1 (got %d)", sols);
  if (n_gamma != code->n)
    return fail(QLDPC_EINVAL, "relay min-sum: gamma rows have %d entries, the code has %d variables", n_gamma, code->n);
  int64_t total = 0;
  for (int r = 0; r < legs; ++r) {
    if (h_leg_iters[r] < 1) return fail(QLDPC_EINVAL, "relay min-sum: leg %d has %d iterations (>= 1)", r, h_leg_iters[r]);
    total += h_leg_iters[r];
    if (total > (1 << 20)) return fail(QLDPC_EINVAL, "relay min-sum: more than 2^20 iterations over all legs");
  }
  const int n = code->n;
  for (int64_t i = 0; i < (int64_t)legs * n; ++i)
    if (!std::isfinite(h_gamma[i]))
      return fail(QLDPC_EINVAL, "relay min-sum: gamma[%d][%d] is not finite", (int)(i / n), (int)(i % n));
  if (int rc = relay_limits(code)) return rc;

  std::unique_ptr<qldpc_relay> r(new qldpc_relay());
  r->code = code;
  r->legs = legs, r->sols = sols;
  r->leg_iters.assign(h_leg_iters, h_leg_iters + legs);
  r->gamma.resize((size_t)legs * n);
  for (int l = 0; l < legs; ++l)                     // relabeled variable j is original column vperm[j]
    for (int j = 0; j < n; ++j) r->gamma[(size_t)l * n + j] = h_gamma[(size_t)l * n + code->vperm[j]];
  std::vector<int32_t> lp{0, code->m}, rows(code->m);
  for (int i = 0; i < code->m; ++i) rows[i] = i;
  if (int rc = qldpc_schedule_create(code, 1, lp.data(), rows.data(), &r->sched)) return rc;
  if (code->device >= 0) {
    HIP_TRY(r->d_leg_iters.upload(r->leg_iters));
    HIP_TRY(r->d_gamma.upload(r->gamma));
  }
  *out = r.release();
  return QLDPC_OK;
}

extern "C" int qldpc_relay_destroy(qldpc_relay* relay) {
  delete relay;
  return QLDPC_OK;
}

static int relay_layout(const qldpc_relay* relay, bool vp, int32_t* out7) {
  if (!relay || !out7) return fail(QLDPC_EINVAL, "null argument");
  if (int rc = relay_limits(relay->code)) return rc;
  RelayArgs ra{};
  out7[0] = relay_plan_static(relay, vp, &ra);
  out7[1] = ra.d.wave_bytes, out7[2] = ra.d.off_c2v, out7[3] = ra.d.off_synw;
  out7[4] = ra.off_m, out7[5] = ra.off_ew, out7[6] = ra.off_best;
  return QLDPC_OK;
}

extern "C" int qldpc_relay_layout(const qldpc_relay* relay, int32_t* out7) { return relay_layout(relay, false, out7); }

extern "C" int qldpc_relay_vprior_layout(const qldpc_relay* relay, int32_t* out7) {
  return relay_layout(relay, true, out7);
}

static int relay_kernel_name(const qldpc_code* code, const qldpc_relay* relay, bool vp, char* buf, int len) {
  if (!code || !relay || !buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  if (relay->code != code) return fail(QLDPC_EINVAL, "relay handle was built for a different code");
  if (int rc = relay_limits(code)) return rc;
  const char* name = "";
  (void)relay_choose(code, vp, &name);
  snprintf(buf, (size_t)len, "%s", name);
  return QLDPC_OK;
}

extern "C" int qldpc_decode_relay_kernel_name(const qldpc_code* code, const qldpc_relay* relay, char* buf, int len) {
  return relay_kernel_name(code, relay, false, buf, len);
}

extern "C" int qldpc_decode_relay_vprior_kernel_name(const qldpc_code* code, const qldpc_relay* relay, char* buf,
                                                     int len) {
  return relay_kernel_name(code, relay, true, buf, len);
}

// ---------------------------------------------------------------------------
// launch plan, device half: occupancy; cached in the handle per option generation
// ---------------------------------------------------------------------------
static int build_plan(qldpc_relay* r, bool vp, RelayPlan* p) {
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, dev));
  p->kernel = relay_choose(r->code, vp, &p->name);
  const int image_lds = relay_plan_static(r, vp, &p->args);
  HIP_TRY(qldpc::configure_relay_kernel(p->kernel, max_lds));
  const int max_waves = QLDPC_MAX_THREADS / 64;
  const int wb = p->args.d.wave_bytes;
  int best = 0;
  auto occupancy = [&](int w, int lds, int* nb) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, p->kernel, 64 * w, (size_t)lds);
  };
  for (int w = max_waves; w >= 1; --w) {
    const int lds = image_lds + w * wb;
    if (lds > max_lds) continue;
    int nb = 0;
    HIP_TRY(occupancy(w, lds, &nb));
    if (nb * w > best) p->waves = w, p->blocks_per_cu = nb, p->lds = lds, best = nb * w;
  }
  if (best == 0)
    return fail(QLDPC_EUNSUP, "relay min-sum: the tables%s and one wave's state (%d + %d B) do not fit the %d B of "
                "LDS; there is no HBM-resident variant", vp ? ", the prior row" : "", image_lds, wb, max_lds);
  // Tuning overrides (experiments, tests): options waves_per_wg, wg_per_cu.
  if (const int64_t ow = opt(&Options::waves_per_wg)) {
    const int w = (int)ow, lds = image_lds + w * wb;
    int nb = 0;
    if (w >= 1 && w <= max_waves && lds <= max_lds && occupancy(w, lds, &nb) == hipSuccess && nb > 0)
      p->waves = w, p->blocks_per_cu = nb, p->lds = lds;
  }
  if (const int64_t ok = opt(&Options::wg_per_cu)) {
    const int k2 = (int)ok;
    if (k2 >= 1 && k2 < p->blocks_per_cu) p->blocks_per_cu = k2;
  }
  return QLDPC_OK;
}

static int resolve_plan(qldpc_relay* r, bool vp, RelayPlan* out) {
  std::lock_guard<std::mutex> lk(r->mu);
  const uint32_t gen = g_opt.gen.load();
  RelayPlan& slot = r->plan[vp ? 1 : 0];
  if (!slot.ok || slot.gen != gen) {
    RelayPlan p{};                                    // built aside, published whole
    if (int rc = build_plan(r, vp, &p)) return rc;
    p.ok = true;
    p.gen = gen;
    slot = p;
  }
  *out = slot;
  return QLDPC_OK;
}

static int relay_launch_info(const qldpc_code* code, const qldpc_relay* relay_c, bool vp, int* waves_per_wg,
                             int* wg_per_cu, int* lds_bytes) {
  auto* relay = const_cast<qldpc_relay*>(relay_c);
  if (!code || !relay || !waves_per_wg || !wg_per_cu || !lds_bytes) return fail(QLDPC_EINVAL, "null argument");
  if (relay->code != code) return fail(QLDPC_EINVAL, "relay handle was built for a different code");
  if (int rc = relay_limits(code)) return rc;
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  RelayPlan plan;
  if (int rc = resolve_plan(relay, vp, &plan)) return rc;
  *waves_per_wg = plan.waves, *wg_per_cu = plan.blocks_per_cu, *lds_bytes = plan.lds;
  return QLDPC_OK;
}

extern "C" int qldpc_decode_relay_launch_info(const qldpc_code* code, const qldpc_relay* relay, int* waves_per_wg,
                                              int* wg_per_cu, int* lds_bytes) {
  return relay_launch_info(code, relay, false, waves_per_wg, wg_per_cu, lds_bytes);
}

extern "C" int qldpc_decode_relay_vprior_launch_info(const qldpc_code* code, const qldpc_relay* relay,
                                                     int* waves_per_wg, int* wg_per_cu, int* lds_bytes) {
  return relay_launch_info(code, relay, true, waves_per_wg, wg_per_cu, lds_bytes);
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
// everything checked before any HIP call; *done: nothing to launch
// what a per-variable-prior call brings on top of the scalar one's arguments
struct VpriorCall {
  const qldpc_prior* prior;
  int cost;
};

static int validate(const qldpc_code* code, const qldpc_relay* relay, int syn_format, int ehat_format, int64_t batch,
                    const void* syn, const void* ehat, const void* iters, bool* done, const VpriorCall* vp = nullptr,
                    double eps = 0.0) {
  *done = false;
  if ((syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  if (!code || !relay) return fail(QLDPC_EINVAL, "code/relay is null");
  if (relay->code != code) return fail(QLDPC_EINVAL, "relay handle was built for a different code");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (vp) {
    const qldpc_prior* pr = vp->prior;
    if (!pr) return fail(QLDPC_EINVAL, "prior handle is null");
    if (pr->code != code || pr->n != code->n || pr->m != code->m || pr->E != code->E)
      return fail(QLDPC_EINVAL, "prior handle was built for a different code");
    if (!(eps == pr->eps))
      return fail(QLDPC_EINVAL, "relay min-sum: eps = %g, but the prior row was formed with eps = %g", eps, pr->eps);
    if (vp->cost != QLDPC_RELAY_COST_HAMMING && vp->cost != QLDPC_RELAY_COST_PRIOR)
      return fail(QLDPC_EINVAL, "relay min-sum: unknown solution cost %d (0: Hamming weight, 1: prior weight)",
                  vp->cost);
  }
  if (int rc = relay_limits(code)) return rc;
  if (batch == 0) {
    *done = true;
    return QLDPC_OK;
  }
  if (!syn || !ehat || !iters) return fail(QLDPC_EINVAL, "null buffer");
  if (code->device < 0 || !relay->sched->generic.dev)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code/relay handle was created");
  if (vp && (!vp->prior->d_L.p || !vp->prior->d_W.p))
    return fail(QLDPC_EHIP, "no HIP device was visible when the prior handle was created");
  return QLDPC_OK;
}

// qldpc_decode_device_relay, and with `vp` qldpc_decode_device_relay_vprior (p is then unread)
static int relay_device(const qldpc_code* code, const qldpc_relay* relay_c, const VpriorCall* vp, const void* d_syn,
                        int syn_format, int64_t batch, double p, double beta, double eps, void* d_ehat,
                        int ehat_format, int32_t* d_iters, double* d_post, int32_t* d_flags, int32_t* d_info,
                        void* stream) {
  auto* relay = const_cast<qldpc_relay*>(relay_c);
  bool done = false;
  if (int rc = validate(code, relay, syn_format, ehat_format, batch, d_syn, d_ehat, d_iters, &done, vp, eps))
    return rc;
  if (done) return QLDPC_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != code->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", code->device, dev);
  RelayPlan plan;
  if (int rc = resolve_plan(relay, vp != nullptr, &plan)) return rc;
  hipStream_t st = (hipStream_t)stream;
  RelayArgs ra = plan.args;
  qldpc::DecodeArgs& a = ra.d;
  a.syn = (const uint8_t*)d_syn, a.ehat = (uint8_t*)d_ehat;
  a.syn_bits = syn_format == QLDPC_FMT_BITS, a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.iters = d_iters, a.post = d_post, a.flags = d_flags;
  ra.info = d_info;
  a.batch = batch;
  if (vp) {
    a.vprior = vp->prior->d_L;
    a.L = 0.0, a.L32 = 0.0f;                          // (unread: every prior comes from the row)
  } else {
    a.L = qldpc_prior_llr(p, eps);                    // np.log prior, as MS takes it
    a.L32 = (float)a.L;
  }
  a.beta = beta, a.eps = eps;
  a.max_iter = relay->leg_iters[0];                   // (unread: the legs carry the counts)
  qldpc_schedule* s = relay->sched;
  a.queue = nullptr;
  if (!opt(&Options::static_sched)) {
    a.queue = s->d_queue + (s->qnext.fetch_add(1) % qldpc_schedule::kQueueSlots);
    HIP_TRY(hipMemsetAsync(a.queue, 0, sizeof(uint32_t), st));
  }
  const int64_t need = (batch + plan.waves - 1) / plan.waves;
  const int64_t resident = (int64_t)plan.blocks_per_cu * plan.cus;
  const int grid = (int)std::max<int64_t>(1, std::min(need, resident));
  TimedLaunch t;
  if (int rc = timing_begin(&t, st)) return rc;
  if (vp)
    HIP_TRY(qldpc::launch_relay_vprior(plan.kernel, RelayVpriorArgs{ra, (const long long*)vp->prior->d_W.p, vp->cost},
                                       grid, 64 * plan.waves, plan.lds, st));
  else
    HIP_TRY(qldpc::launch_relay(plan.kernel, ra, grid, 64 * plan.waves, plan.lds, st));
  return timing_end(&t, st);
}

extern "C" int qldpc_decode_device_relay(const qldpc_code* code, const qldpc_relay* relay, const void* d_syn,
                                         int syn_format, int64_t batch, double p, double beta, double eps,
                                         void* d_ehat, int ehat_format, int32_t* d_iters, double* d_post,
                                         int32_t* d_flags, int32_t* d_info, void* stream) {
  return relay_device(code, relay, nullptr, d_syn, syn_format, batch, p, beta, eps, d_ehat, ehat_format, d_iters,
                      d_post, d_flags, d_info, stream);
}

extern "C" int qldpc_decode_device_relay_vprior(const qldpc_code* code, const qldpc_relay* relay,
                                                const qldpc_prior* prior, int cost, const void* d_syn, int syn_format,
                                                int64_t batch, double beta, double eps, void* d_ehat, int ehat_format,
                                                int32_t* d_iters, double* d_post, int32_t* d_flags, int32_t* d_info,
                                                void* stream) {
  const VpriorCall vp{prior, cost};
  return relay_device(code, relay, &vp, d_syn, syn_format, batch, 0.0, beta, eps, d_ehat, ehat_format, d_iters,
                      d_post, d_flags, d_info, stream);
}

// qldpc_decode_host_relay, and with `vp` qldpc_decode_host_relay_vprior
static int relay_host(const qldpc_code* code_c, const qldpc_relay* relay_c, const VpriorCall* vp, const uint8_t* h_syn,
                      int64_t batch, double p, double beta, double eps, uint8_t* h_ehat, int32_t* h_iters,
                      double* h_post, int32_t* h_flags, int32_t* h_info) {
  auto* code = const_cast<qldpc_code*>(code_c);
  auto* relay = const_cast<qldpc_relay*>(relay_c);
  bool done = false;
  if (int rc = validate(code, relay, QLDPC_FMT_BYTES, QLDPC_FMT_BYTES, batch, h_syn, h_ehat, h_iters, &done, vp, eps))
    return rc;
  if (done) return QLDPC_OK;
  std::lock_guard<std::mutex> lk(code->ws_mu);
  const int64_t m = code->m, n = code->n;
  if (int rc = ws_reserve(code, batch, h_post != nullptr)) return rc;
  hipStream_t st = code->ws_stream;
  if (h_info) {
    std::lock_guard<std::mutex> lr(relay->mu);
    if (relay->ws_info_cap < batch) {
      HIP_TRY(hipStreamSynchronize(st));
      HIP_TRY(relay->ws_info.alloc((size_t)2 * batch));
      relay->ws_info_cap = batch;
    }
  }
  if (batch * m) {
    memcpy(code->hp_syn, h_syn, batch * m);
    HIP_TRY(hipMemcpyAsync(code->ws_syn, code->hp_syn, batch * m, hipMemcpyHostToDevice, st));
  }
  if (int rc = relay_device(code, relay, vp, code->ws_syn, QLDPC_FMT_BYTES, batch, p, beta, eps, code->ws_ehat,
                            QLDPC_FMT_BYTES, code->ws_iters, h_post ? code->ws_post.p : nullptr, code->ws_flags,
                            h_info ? relay->ws_info.p : nullptr, st))
    return rc;
  if (batch * n) HIP_TRY(hipMemcpyAsync(code->hp_ehat, code->ws_ehat, batch * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_iters, code->ws_iters, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_flags, code->ws_flags, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  if (h_post && batch * n)
    HIP_TRY(hipMemcpyAsync(code->hp_post, code->ws_post, sizeof(double) * batch * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));                  // this stream only
  if (h_info) HIP_TRY(hipMemcpy(h_info, relay->ws_info, sizeof(int32_t) * 2 * batch, hipMemcpyDeviceToHost));
  if (batch * n) memcpy(h_ehat, code->hp_ehat, batch * n);
  memcpy(h_iters, code->hp_iters, sizeof(int32_t) * batch);
  if (h_flags) memcpy(h_flags, code->hp_flags, sizeof(int32_t) * batch);
  if (h_post && batch * n) memcpy(h_post, code->hp_post, sizeof(double) * batch * n);
  return QLDPC_OK;
}

extern "C" int qldpc_decode_host_relay(const qldpc_code* code, const qldpc_relay* relay, const uint8_t* h_syn,
                                       int64_t batch, double p, double beta, double eps, uint8_t* h_ehat,
                                       int32_t* h_iters, double* h_post, int32_t* h_flags, int32_t* h_info) {
  return relay_host(code, relay, nullptr, h_syn, batch, p, beta, eps, h_ehat, h_iters, h_post, h_flags, h_info);
}

extern "C" int qldpc_decode_host_relay_vprior(const qldpc_code* code, const qldpc_relay* relay,
                                              const qldpc_prior* prior, int cost, const uint8_t* h_syn, int64_t batch,
                                              double beta, double eps, uint8_t* h_ehat, int32_t* h_iters,
                                              double* h_post, int32_t* h_flags, int32_t* h_info) {
  const VpriorCall vp{prior, cost};
  return relay_host(code, relay, &vp, h_syn, batch, 0.0, beta, eps, h_ehat, h_iters, h_post, h_flags, h_info);
}
