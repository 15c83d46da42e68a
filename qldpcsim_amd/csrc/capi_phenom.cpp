// capi_phenom.cpp — phenomenological noise (multi-round space-time decoding of
// one CSS half): the device shot source, the outcome counter, the half's
// logical table and the step between sliding windows (phenom_kernels.hip).

#include <cmath>
#include <memory>

#include "capi_internal.h"
#include "phenom_kernels.h"

using namespace capi;

// the logical table is staged into LDS up to this size when it fits next to
// H's CSR and the wave slices, else read from global memory (L2-resident)
static constexpr long long kPhenomLdsTabBytes = 64 * 1024;

struct qldpc_phenom {
  const qldpc_code* code = nullptr;
  int m = 0, n = 0, E = 0;            // the code's shape when the table was built
  int W = 0, k = 0, kp = 0, device = -1;
  DevBuf<uint64_t> d_tab;             // L, word-major [W][kp]
};

// Every check that needs no device: the code, the rounds and the limits of
// the kernels' tables (n <= 4096: one lane per word of an n-bit vector; m, E
// <= 65535: 16-bit column indices and the CSR's LDS budget).
static int phenom_tabs(const qldpc_code* code, int rounds, qldpc::PhenomTabs* t) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (rounds < 1) return fail(QLDPC_EINVAL, "rounds must be >= 1 (got %d)", rounds);
  if (code->n > 4096 || code->m > 65535 || code->E > 65535)
    return fail(QLDPC_EUNSUP, "the phenomenological kernels support n <= 4096 and m, E <= 65535 (got n = %d, m = %d, "
                "E = %d)", code->n, code->m, code->E);
  const long long N = (long long)rounds * code->n + (long long)(rounds - 1) * code->m;
  const long long M = (long long)rounds * code->m;
  if (N > (1ll << 24) || M > (1ll << 24))
    return fail(QLDPC_EUNSUP, "%d rounds give %lld space-time columns: past any wave's LDS slice", rounds, N);
  t->rp = code->d_row_ptr;
  t->ci = code->d_col_idx;
  t->m = code->m;
  t->n = code->n;
  t->e = code->E;
  t->udeg = code->m > 0 ? code->uniform_deg : 0;
  t->W = (code->n + 63) / 64;
  t->rounds = rounds;
  t->N = (int)N;
  t->M = (int)M;
  t->NW = (int)((N + 63) / 64);
  t->MW = (int)((M + 63) / 64);
  return QLDPC_OK;
}

// floor(prob 2^32), the threshold qldpc_channel_table(prob, 0, 0) yields
static int phenom_threshold(const char* name, double prob, uint64_t* thr) {
  if (!(prob >= 0.0 && prob < 1.0)) return fail(QLDPC_EINVAL, "%s must lie in [0, 1) (got %g)", name, prob);
  *thr = (uint64_t)std::min(4294967296.0, std::floor(prob * 4294967296.0));
  return QLDPC_OK;
}

static int phenom_device(const qldpc_code* code, int* max_lds) {
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != code->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", code->device, dev);
  HIP_TRY(hipDeviceGetAttribute(max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  return QLDPC_OK;
}

static int phenom_grid(int64_t batch) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  const int64_t need = (batch + qldpc::kPhenomWaves - 1) / qldpc::kPhenomWaves;
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, (int64_t)cus * 8));
}

extern "C" int qldpc_phenom_create(const qldpc_code* code, const uint8_t* h_L, int k, qldpc_phenom** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (k < 0 || k > code->n) return fail(QLDPC_EINVAL, "k = %d logical rows for n = %d", k, code->n);
  if (k > 0 && !h_L) return fail(QLDPC_EINVAL, "logical table is null");
  if (code->n > 4096) return fail(QLDPC_EUNSUP, "the phenomenological kernels support n <= 4096 (got %d)", code->n);
  std::unique_ptr<qldpc_phenom> ph(new qldpc_phenom());
  ph->code = code;
  ph->m = code->m, ph->n = code->n, ph->E = code->E;
  ph->W = (code->n + 63) / 64, ph->k = k, ph->kp = (k + 63) & ~63, ph->device = code->device;
  // No visible device: the handle is still made (argument checks work); the
  // counter entry point then fails loudly.
  if (ph->device >= 0) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ph->device)
      return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", ph->device, dev);
    std::vector<uint64_t> tab((size_t)ph->W * ph->kp, 0);
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < ph->n; ++j)
        if (h_L[(size_t)i * ph->n + j] & 1) tab[(size_t)(j >> 6) * ph->kp + i] |= 1ull << (j & 63);
    HIP_TRY(ph->d_tab.upload(tab));
  }
  *out = ph.release();
  return QLDPC_OK;
}

extern "C" int qldpc_phenom_destroy(qldpc_phenom* ph) {
  delete ph;                                         // the table owns itself
  return QLDPC_OK;
}

extern "C" int qldpc_phenom_sample(const qldpc_code* code, int rounds, double p_data, double q, uint64_t seed,
                                   uint64_t shot0, int64_t batch, void* d_det, int det_format, uint64_t* d_E,
                                   uint64_t* d_fired, void* stream) {
  // every argument check comes before the first HIP call
  qldpc::PhenomSampleArgs a{};
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (rounds < 1) return fail(QLDPC_EINVAL, "rounds must be >= 1 (got %d)", rounds);
  if (det_format != QLDPC_FMT_BYTES && det_format != QLDPC_FMT_BITS)
    return fail(QLDPC_EINVAL, "unknown detector format");
  if (int rc = phenom_threshold("p_data", p_data, &a.thr_data)) return rc;
  if (int rc = phenom_threshold("q", q, &a.thr_meas)) return rc;
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if ((code->m && !d_det) || !d_E) return fail(QLDPC_EINVAL, "null device buffer");
  if (int rc = phenom_tabs(code, rounds, &a.t)) return rc;
  if (batch == 0) return QLDPC_OK;
  int max_lds = 0;
  if (int rc = phenom_device(code, &max_lds)) return rc;
  if (qldpc::phenom_sample_lds_bytes(a.t) > max_lds)
    return fail(QLDPC_EUNSUP, "the phenomenological sampler needs %lld B of LDS for %d rounds of this code (%d "
                "columns), the device has %d", qldpc::phenom_sample_lds_bytes(a.t), rounds, a.t.N, max_lds);
  a.det = (uint8_t*)d_det;
  a.det_bits = det_format == QLDPC_FMT_BITS;
  a.E = d_E;
  a.fired = d_fired;
  a.batch = batch;
  a.shot0 = shot0;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32);
  HIP_TRY(qldpc::launch_phenom_sample(a, phenom_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

extern "C" int qldpc_phenom_count(const qldpc_code* code, const qldpc_phenom* ph, int rounds, int64_t batch,
                                  const void* d_det, int det_format, const uint64_t* d_E, const void* d_ehat,
                                  int ehat_format, const int32_t* d_iters, int64_t* d_counters, uint8_t* d_class,
                                  uint64_t* d_flips, uint64_t* d_resid, void* stream) {
  // every argument check comes before the first HIP call
  qldpc::PhenomCountArgs a{};
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (!ph) return fail(QLDPC_EINVAL, "logical table handle is null");
  if (rounds < 1) return fail(QLDPC_EINVAL, "rounds must be >= 1 (got %d)", rounds);
  if (ph->code != code || ph->n != code->n || ph->m != code->m || ph->E != code->E)
    return fail(QLDPC_EINVAL, "the logical table handle was built for another code");
  if ((det_format != QLDPC_FMT_BYTES && det_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown detector / estimate format");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if ((code->m && !d_det) || !d_E || !d_ehat || !d_iters || !d_counters)
    return fail(QLDPC_EINVAL, "null device buffer");
  if (int rc = phenom_tabs(code, rounds, &a.t)) return rc;
  if (batch == 0) return QLDPC_OK;
  int max_lds = 0;
  if (int rc = phenom_device(code, &max_lds)) return rc;
  if (ph->device != code->device) return fail(QLDPC_EINVAL, "the logical table handle was built on another device");
  a.tab_lds = 8ll * a.t.W * ph->kp <= kPhenomLdsTabBytes &&
              qldpc::phenom_count_lds_bytes(a.t, ph->kp, true) <= max_lds;
  if (qldpc::phenom_count_lds_bytes(a.t, ph->kp, a.tab_lds != 0) > max_lds)
    return fail(QLDPC_EUNSUP, "the phenomenological counter needs %lld B of LDS for %d rounds of this code (%d "
                "columns), the device has %d", qldpc::phenom_count_lds_bytes(a.t, ph->kp, a.tab_lds != 0), rounds,
                a.t.N, max_lds);
  a.det = (const uint8_t*)d_det;
  a.det_bits = det_format == QLDPC_FMT_BITS;
  a.E = d_E;
  a.ehat = (const uint8_t*)d_ehat;
  a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.iters = d_iters;
  a.tab = ph->d_tab;
  a.k = ph->k;
  a.kp = ph->kp;
  a.acc = reinterpret_cast<unsigned long long*>(d_counters);
  a.cls = d_class;
  a.flips = d_flips;
  a.resid = d_resid;
  a.batch = batch;
  HIP_TRY(qldpc::launch_phenom_count(a, phenom_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

extern "C" int qldpc_phenom_window(const qldpc_code* code, int rounds, int64_t batch, int done_start, int done_rounds,
                                   int done_closed, int done_commit, const void* d_west, int west_format,
                                   const int32_t* d_witers, void* d_ehat, int ehat_format, int32_t* d_iters,
                                   int next_start, int next_rounds, const void* d_det, int det_format, void* d_syn,
                                   int syn_format, void* stream) {
  // every argument check comes before the first HIP call
  qldpc::PhenomWindowArgs a{};
  qldpc::PhenomTabs t{};
  auto fmt_ok = [](int f) { return f == QLDPC_FMT_BYTES || f == QLDPC_FMT_BITS; };
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (rounds < 1) return fail(QLDPC_EINVAL, "rounds must be >= 1 (got %d)", rounds);
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (done_rounds < 0 || next_rounds < 0 || (done_rounds == 0 && next_rounds == 0))
    return fail(QLDPC_EINVAL, "neither a decoded window nor a next one");
  if (int rc = phenom_tabs(code, rounds, &t)) return rc;
  const int nm = t.n + t.m;
  if (done_rounds > 0) {
    if (done_start < 0 || done_start > rounds - done_rounds)
      return fail(QLDPC_EINVAL, "window [%d, %d + %d) lies outside [0, %d)", done_start, done_start, done_rounds,
                  rounds);
    if (done_commit < 1 || done_commit > done_rounds)
      return fail(QLDPC_EINVAL, "commit = %d rounds of a window of %d", done_commit, done_rounds);
    if (done_closed && (done_start + done_rounds != rounds || done_commit != done_rounds || next_rounds > 0))
      return fail(QLDPC_EINVAL, "a closed window ends at the last round, commits all its rounds and has no successor");
    if (!done_closed && done_start + done_rounds >= rounds)
      return fail(QLDPC_EINVAL, "an open window has measurement columns in every round: it ends before round %d",
                  rounds - 1);
    if (!fmt_ok(west_format) || !fmt_ok(ehat_format)) return fail(QLDPC_EINVAL, "unknown estimate format");
    if (!d_west || !d_witers || !d_ehat || !d_iters) return fail(QLDPC_EINVAL, "null device buffer");
    a.has_done = 1;
    a.commit_off = done_start * nm;
    a.west_len = done_closed ? done_rounds * t.n + (done_rounds - 1) * t.m : done_rounds * nm;
    a.commit_len = done_closed ? a.west_len : done_commit * nm;
    a.corr_off = (done_commit - 1) * nm + t.n;
  }
  if (next_rounds > 0) {
    if (next_start < 0 || next_start > rounds - next_rounds)
      return fail(QLDPC_EINVAL, "window [%d, %d + %d) lies outside [0, %d)", next_start, next_start, next_rounds,
                  rounds);
    if (done_rounds > 0 && next_start != done_start + done_commit)
      return fail(QLDPC_EINVAL, "the next window starts at round %d, the decoded one committed up to %d", next_start,
                  done_start + done_commit);
    if (!fmt_ok(det_format) || !fmt_ok(syn_format)) return fail(QLDPC_EINVAL, "unknown detector / syndrome format");
    if (t.m && (!d_det || !d_syn)) return fail(QLDPC_EINVAL, "null device buffer");
    a.has_next = t.m > 0;
    a.syn_off = next_start * t.m;
    a.syn_len = next_rounds * t.m;
  }
  if (batch == 0) return QLDPC_OK;
  int max_lds = 0;                                   // the kernel uses no LDS
  if (int rc = phenom_device(code, &max_lds)) return rc;
  a.n = t.n, a.m = t.m, a.N = t.N, a.M = t.M;
  a.west = (const uint8_t*)d_west;
  a.west_bits = west_format == QLDPC_FMT_BITS;
  a.witers = d_witers;
  a.ehat = (uint8_t*)d_ehat;
  a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.iters = d_iters;
  a.det = (const uint8_t*)d_det;
  a.det_bits = det_format == QLDPC_FMT_BITS;
  a.syn = (uint8_t*)d_syn;
  a.syn_bits = syn_format == QLDPC_FMT_BITS;
  a.batch = batch;
  HIP_TRY(qldpc::launch_phenom_window(a, phenom_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

static_assert(QLDPC_PHENOM_SAMPLE == qldpc::kPhenomSample && QLDPC_PHENOM_COUNT == qldpc::kPhenomCount,
              "qldpc_decoder.h names the kernels as phenom_kernels.h does");

// The instance phenom_choice picks, as the launchers do. Needs no device.
extern "C" int qldpc_phenom_kernel_name(const qldpc_code* code, int kind, char* buf, int len) {
  if (!buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  qldpc::PhenomTabs t{};
  if (int rc = phenom_tabs(code, 1, &t)) return rc;      // (the instance does not depend on the rounds)
  if (!qldpc::phenom_kernel_name(kind, qldpc::phenom_choice(t), buf, len))
    return fail(QLDPC_EINVAL, "unknown phenomenological kernel kind %d", kind);
  return QLDPC_OK;
}
