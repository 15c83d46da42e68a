// capi_launch.cpp — the launch plumbing every decoder family shares (capi_launch.h): device limits, the queue
// ring's claim, the LDS-limit predicate, launch timing (qldpc_timing_*) and the host staging round trip.

#include "capi_launch.h"

using namespace capi;

int capi::device_limits(int* max_lds, int* cus, int* dev) {
  int d = 0;
  HIP_TRY(hipGetDevice(&d));
  HIP_TRY(hipDeviceGetAttribute(max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, d));
  HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, d));
  if (dev) *dev = d;
  return QLDPC_OK;
}

int QueueRing::claim(hipStream_t st, uint32_t** slot) {
  *slot = buf + (next.fetch_add(1) % kSlots);
  HIP_TRY(hipMemsetAsync(*slot, 0, sizeof(uint32_t), st));
  return QLDPC_OK;
}

LdsLimit capi::lds_limit(bool lds_ok, const qldpc_code* c, int algo) {
  if (!lds_ok) return LDS_TABLES16;
  if (algo == QLDPC_ALGO_MS && c->max_row_deg > 32) return LDS_MS_ROW_DEG;
  if (algo == QLDPC_ALGO_BP && c->max_col_deg > 128) return LDS_BP_COL_DEG;   // np.sum's last unsplit length
  if (opt(&Options::force_hbm) != 0) return LDS_FORCE_HBM;
  return LDS_FITS;
}

// ---------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------
static std::mutex g_tmu;
static bool g_timing = false;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_events;
static double g_total_ms = 0.0;
static int64_t g_launches = 0;

extern "C" int qldpc_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_tmu);
  g_timing = on != 0;
  return QLDPC_OK;
}

static int drain_events_locked() {
  for (auto& ev : g_events) {
    HIP_TRY(hipEventSynchronize(ev.second));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
    g_total_ms += ms;
    g_launches++;
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  g_events.clear();
  return QLDPC_OK;
}

extern "C" int qldpc_timing_reset(void) {
  std::lock_guard<std::mutex> lk(g_tmu);
  int rc = drain_events_locked();
  g_total_ms = 0.0;
  g_launches = 0;
  return rc;
}

extern "C" int qldpc_timing_read(double* total_ms, int64_t* launches) {
  std::lock_guard<std::mutex> lk(g_tmu);
  int rc = drain_events_locked();
  if (total_ms) *total_ms = g_total_ms;
  if (launches) *launches = g_launches;
  return rc;
}

// A timed launch: timing_begin before the kernel is enqueued, timing_end
// after. The event pair goes to g_events; drain_events_locked destroys it.
int capi::timing_begin(TimedLaunch* t, hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(g_tmu);
    if (!g_timing) return QLDPC_OK;
  }
  HIP_TRY(hipEventCreate(&t->e0));
  HIP_TRY(hipEventCreate(&t->e1));
  HIP_TRY(hipEventRecord(t->e0, st));
  return QLDPC_OK;
}

int capi::timing_end(TimedLaunch* t, hipStream_t st) {
  if (!t->e0) return QLDPC_OK;
  HIP_TRY(hipEventRecord(t->e1, st));
  std::lock_guard<std::mutex> lk(g_tmu);
  g_events.emplace_back(t->e0, t->e1);
  return QLDPC_OK;
}

// ---------------------------------------------------------------------------
// host staging
// ---------------------------------------------------------------------------
// the code's workspace (under ws_mu), grown to `batch` half-shots; posterior buffers only when wanted
static int ws_reserve(qldpc_code* code, int64_t batch, bool want_post) {
  const int m = code->m, n = code->n;
  if (!code->ws_stream) HIP_TRY(hipStreamCreateWithFlags(&code->ws_stream, hipStreamNonBlocking));
  if (batch > code->ws_cap) {
    code->ws_cap = 0;
    code->ws_post_cap = 0;
    const int64_t cap = std::max<int64_t>(batch, 64);
    const size_t cm = std::max<int64_t>(1, cap * m), cn = std::max<int64_t>(1, cap * n);
    HIP_TRY(code->ws_syn.alloc(cm));
    HIP_TRY(code->ws_ehat.alloc(cn));
    HIP_TRY(code->ws_iters.alloc(cap));
    HIP_TRY(code->ws_flags.alloc(cap));
    HIP_TRY(code->hp_syn.alloc(cm));
    HIP_TRY(code->hp_ehat.alloc(cn));
    HIP_TRY(code->hp_iters.alloc(cap));
    HIP_TRY(code->hp_flags.alloc(cap));
    code->ws_cap = cap;
  }
  if (want_post && code->ws_post_cap < code->ws_cap) {
    const size_t cn = std::max<int64_t>(1, code->ws_cap * n);
    HIP_TRY(code->ws_post.alloc(cn));
    HIP_TRY(code->hp_post.alloc(cn));
    code->ws_post_cap = code->ws_cap;
  }
  return QLDPC_OK;
}

int capi::stage_in(qldpc_code* code, const CallIO& h, CallIO* d) {
  if (int rc = ws_reserve(code, h.batch, h.post != nullptr)) return rc;
  const int64_t bm = h.batch * code->m;
  if (bm) {
    memcpy(code->hp_syn, h.syn, bm);
    HIP_TRY(hipMemcpyAsync(code->ws_syn, code->hp_syn, bm, hipMemcpyHostToDevice, code->ws_stream));
  }
  *d = CallIO{code->ws_syn.p, QLDPC_FMT_BYTES, h.batch, code->ws_ehat.p, QLDPC_FMT_BYTES, code->ws_iters.p,
              code->ws_flags.p, h.post ? code->ws_post.p : nullptr};
  return QLDPC_OK;
}

int capi::stage_out(qldpc_code* code, const CallIO& h) {
  hipStream_t st = code->ws_stream;
  const int64_t b = h.batch, bn = b * code->n;
  if (bn) HIP_TRY(hipMemcpyAsync(code->hp_ehat, code->ws_ehat, bn, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_iters, code->ws_iters, sizeof(int32_t) * b, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_flags, code->ws_flags, sizeof(int32_t) * b, hipMemcpyDeviceToHost, st));
  if (h.post && bn) HIP_TRY(hipMemcpyAsync(code->hp_post, code->ws_post, sizeof(double) * bn, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));                  // this stream only
  if (bn) memcpy(h.ehat, code->hp_ehat, bn);
  memcpy(h.iters, code->hp_iters, sizeof(int32_t) * b);
  if (h.flags) memcpy(h.flags, code->hp_flags, sizeof(int32_t) * b);
  if (h.post && bn) memcpy(h.post, code->hp_post, sizeof(double) * bn);
  return QLDPC_OK;
}
