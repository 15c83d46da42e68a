// capi_relay.cpp — relay min-sum: the qldpc_relay handle
// (legs, memory strengths, a flooding schedule of its own), its LDS layout and
// launch plans and the decode entry points, the scalar-prior ones
// (relay_ms_kernel) and the per-variable-prior ones (relay_vprior_kernel,
// §3.18). The plumbing shared with the other families is in capi_launch.h.

#include <cmath>
#include <cstdio>
#include <memory>

#include "capi_launch.h"
#include "relay_kernels.h"
#include "../../include/qldpc_libm.h"   // after hip_runtime.h

using namespace capi;
using qldpc::RelayArgs;
using qldpc::RelayVpriorArgs;

namespace {

struct RelayPlan : PlanBase {
  RelayArgs args{};          // every static field filled
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
  const LdsLimit l = lds_limit(c->lds_ok, c, QLDPC_ALGO_MS);
  if (l == LDS_TABLES16)
    return fail(QLDPC_EUNSUP, "relay min-sum: %d x %d with %d edges is past the LDS kernel's 16-bit tables "
                "(m, n, edges <= 65535); there is no HBM-resident variant", c->m, c->n, c->E);
  if (l == LDS_MS_ROW_DEG) return fail(QLDPC_EUNSUP, "relay min-sum: row degree %d > 32 has no LDS kernel", c->max_row_deg);
  if (l == LDS_FORCE_HBM)
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
  int max_lds = 0;
  if (int rc = device_limits(&max_lds, &p->cus)) return rc;
  p->kernel = relay_choose(r->code, vp, &p->name);
  const int image_lds = relay_plan_static(r, vp, &p->args);
  HIP_TRY(qldpc::configure_relay_kernel(p->kernel, max_lds));
  const int wb = p->args.d.wave_bytes;
  auto lds_of = [&](int w) { return image_lds + w * wb; };
  WaveChoice wc;
  HIP_TRY(wave_search(1, QLDPC_MAX_THREADS / 64, max_lds, lds_of, occupancy_of(p->kernel), true, &wc));
  if (!wc.waves)
    return fail(QLDPC_EUNSUP, "relay min-sum: the tables%s and one wave's state (%d + %d B) do not fit the %d B of "
                "LDS; there is no HBM-resident variant", vp ? ", the prior row" : "", image_lds, wb, max_lds);
  p->waves = wc.waves, p->blocks_per_cu = wc.blocks_per_cu, p->lds = wc.lds;
  return QLDPC_OK;
}

static int resolve_plan(qldpc_relay* r, bool vp, RelayPlan* out) {
  return cached_plan(r->mu, r->plan[vp ? 1 : 0], out, [&](RelayPlan* p) { return build_plan(r, vp, p); });
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

static int validate(const qldpc_code* code, const qldpc_relay* relay, const CallIO& io, bool* done,
                    const VpriorCall* vp, double eps) {
  *done = false;
  if ((io.syn_format != QLDPC_FMT_BYTES && io.syn_format != QLDPC_FMT_BITS) ||
      (io.ehat_format != QLDPC_FMT_BYTES && io.ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  if (!code || !relay) return fail(QLDPC_EINVAL, "code/relay is null");
  if (relay->code != code) return fail(QLDPC_EINVAL, "relay handle was built for a different code");
  if (io.batch < 0) return fail(QLDPC_EINVAL, "negative batch");
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
  if (io.batch == 0) {
    *done = true;
    return QLDPC_OK;
  }
  if (!io.syn || !io.ehat || !io.iters) return fail(QLDPC_EINVAL, "null buffer");
  if (code->device < 0 || !relay->sched->generic.dev)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code/relay handle was created");
  if (vp && (!vp->prior->d_L.p || !vp->prior->d_W.p))
    return fail(QLDPC_EHIP, "no HIP device was visible when the prior handle was created");
  return QLDPC_OK;
}

// qldpc_decode_device_relay, and with `vp` qldpc_decode_device_relay_vprior (p is then unread)
static int relay_device(const qldpc_code* code, const qldpc_relay* relay_c, const VpriorCall* vp, const CallIO& io,
                        double p, double beta, double eps, int32_t* d_info, hipStream_t st) {
  auto* relay = const_cast<qldpc_relay*>(relay_c);
  bool done = false;
  if (int rc = validate(code, relay, io, &done, vp, eps)) return rc;
  if (done) return QLDPC_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != code->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", code->device, dev);
  RelayPlan plan;
  if (int rc = resolve_plan(relay, vp != nullptr, &plan)) return rc;
  RelayArgs ra = plan.args;
  qldpc::DecodeArgs& a = ra.d;
  set_call_io(&a, io);
  ra.info = d_info;
  if (vp) {
    a.vprior = vp->prior->d_L;
    a.L = 0.0, a.L32 = 0.0f;                          // (unread: every prior comes from the row)
  } else {
    a.L = qldpc_prior_llr(p, eps);                    // np.log prior, as MS takes it
    a.L32 = (float)a.L;
  }
  a.beta = beta, a.eps = eps;
  a.max_iter = relay->leg_iters[0];                   // (unread: the legs carry the counts)
  a.queue = nullptr;
  if (!opt(&Options::static_sched))
    if (int rc = relay->sched->queue.claim(st, &a.queue)) return rc;
  const int grid = launch_grid(io.batch, plan.waves, plan.blocks_per_cu, plan.cus);
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
  return relay_device(code, relay, nullptr, {d_syn, syn_format, batch, d_ehat, ehat_format, d_iters, d_flags, d_post}, p,
                      beta, eps, d_info, (hipStream_t)stream);
}

extern "C" int qldpc_decode_device_relay_vprior(const qldpc_code* code, const qldpc_relay* relay,
                                                const qldpc_prior* prior, int cost, const void* d_syn, int syn_format,
                                                int64_t batch, double beta, double eps, void* d_ehat, int ehat_format,
                                                int32_t* d_iters, double* d_post, int32_t* d_flags, int32_t* d_info,
                                                void* stream) {
  const VpriorCall vp{prior, cost};
  return relay_device(code, relay, &vp, {d_syn, syn_format, batch, d_ehat, ehat_format, d_iters, d_flags, d_post}, 0.0,
                      beta, eps, d_info, (hipStream_t)stream);
}

// qldpc_decode_host_relay, and with `vp` qldpc_decode_host_relay_vprior
static int relay_host(const qldpc_code* code_c, const qldpc_relay* relay_c, const VpriorCall* vp, const CallIO& h,
                      double p, double beta, double eps, int32_t* h_info) {
  auto* code = const_cast<qldpc_code*>(code_c);
  auto* relay = const_cast<qldpc_relay*>(relay_c);
  bool done = false;
  if (int rc = validate(code, relay, h, &done, vp, eps)) return rc;
  if (done) return QLDPC_OK;
  // the info rows: a device buffer of the handle, grown once the stream is done with the old one
  auto launch = [&](const CallIO& d, hipStream_t st) {
    if (h_info) {
      std::lock_guard<std::mutex> lr(relay->mu);
      if (relay->ws_info_cap < h.batch) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(relay->ws_info.alloc((size_t)2 * h.batch));
        relay->ws_info_cap = h.batch;
      }
    }
    return relay_device(code, relay, vp, d, p, beta, eps, h_info ? relay->ws_info.p : nullptr, st);
  };
  return staged_call(code, h, launch, [&] {
    if (h_info) HIP_TRY(hipMemcpy(h_info, relay->ws_info, sizeof(int32_t) * 2 * h.batch, hipMemcpyDeviceToHost));
    return (int)QLDPC_OK;
  });
}

extern "C" int qldpc_decode_host_relay(const qldpc_code* code, const qldpc_relay* relay, const uint8_t* h_syn,
                                       int64_t batch, double p, double beta, double eps, uint8_t* h_ehat,
                                       int32_t* h_iters, double* h_post, int32_t* h_flags, int32_t* h_info) {
  return relay_host(code, relay, nullptr, host_io(h_syn, batch, h_ehat, h_iters, h_post, h_flags), p, beta, eps, h_info);
}

extern "C" int qldpc_decode_host_relay_vprior(const qldpc_code* code, const qldpc_relay* relay,
                                              const qldpc_prior* prior, int cost, const uint8_t* h_syn, int64_t batch,
                                              double beta, double eps, uint8_t* h_ehat, int32_t* h_iters,
                                              double* h_post, int32_t* h_flags, int32_t* h_info) {
  const VpriorCall vp{prior, cost};
  return relay_host(code, relay, &vp, host_io(h_syn, batch, h_ehat, h_iters, h_post, h_flags), 0.0, beta, eps, h_info);
}
