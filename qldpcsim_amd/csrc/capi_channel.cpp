// capi_channel.cpp — device channel sampler, outcome counters and the
// logical-operator tables of a CSS pair (channel_kernels.hip).

#include <cmath>
#include <memory>

#include "capi_internal.h"
#include "channel_kernels.h"

using namespace capi;

// automatic residency: the most table bytes (both tables) staged into LDS.
// Measured faster than global memory at 18 KB (LP118_0) and 49 KB (LP118_2);
// larger tables leave a CU one or two workgroups and go to global memory
// 
static constexpr long long kLogicalLdsTabBytes = 64 * 1024;

// The pair's shape as the kernels and channel_choice read it: every check
// and field that needs no device
static int pair_shape(const qldpc_code* hx, const qldpc_code* hz, qldpc::PairTabs* t) {
  if (!hx || !hz) return fail(QLDPC_EINVAL, "code is null");
  if (hx->n != hz->n)
    return fail(QLDPC_EINVAL, "Hx and Hz must have the same number of columns (physical qubits).");
  t->mx = hx->m;
  t->mz = hz->m;
  t->ex = hx->E;
  t->ez = hz->E;
  t->n = hx->n;
  t->W = (hx->n + 63) / 64;
  t->udeg = (hx->uniform_deg == hz->uniform_deg && hx->m > 0 && hz->m > 0) ? hx->uniform_deg : 0;
  return QLDPC_OK;
}

static int pair_limit(const qldpc::PairTabs& t) {
  if (t.W > 64) return fail(QLDPC_EUNSUP, "the channel kernels support n <= 4096 qubits (got %d)", t.n);
  return QLDPC_OK;
}

static int pair_tabs(const qldpc_code* hx, const qldpc_code* hz, qldpc::PairTabs* t) {
  if (int rc = pair_shape(hx, hz, t)) return rc;
  if (hx->device < 0 || hz->device < 0)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  if (hx->device != hz->device) return fail(QLDPC_EINVAL, "Hx and Hz live on different devices");
  if (int rc = pair_limit(*t)) return rc;
  t->rp_x = hx->d_row_ptr;
  t->ci_x = hx->d_col_idx;
  t->rp_z = hz->d_row_ptr;
  t->ci_z = hz->d_col_idx;
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  if (qldpc::channel_lds_bytes(*t, true) > max_lds)
    return fail(QLDPC_EUNSUP, "the channel kernels need %d B of LDS for these codes",
                qldpc::channel_lds_bytes(*t, true));
  return QLDPC_OK;
}

static int channel_grid(int64_t batch) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  const int64_t need = (batch + qldpc::kChannelWaves - 1) / qldpc::kChannelWaves;
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, (int64_t)cus * 8));
}

extern "C" int qldpc_channel_thresholds(double p, uint64_t* t1, uint64_t* t2, uint64_t* t3) {
  if (!(p >= 0.0 && p <= 1.0)) return fail(QLDPC_EINVAL, "p must lie in [0, 1] (got %g)", p);
  const double q = p / 3.0, two32 = 4294967296.0;
  uint64_t t[3];
  for (int k = 0; k < 3; ++k) t[k] = (uint64_t)std::min(two32, std::floor((k + 1) * q * two32));
  if (t1) *t1 = t[0];
  if (t2) *t2 = t[1];
  if (t3) *t3 = t[2];
  return QLDPC_OK;
}

extern "C" int qldpc_channel_sample(const qldpc_code* hx, const qldpc_code* hz, double p, uint64_t seed,
                                    uint64_t shot0, int64_t batch, uint64_t* d_errx, uint64_t* d_errz,
                                    uint8_t* d_syn_z, uint8_t* d_syn_x, void* stream) {
  return qldpc_channel_sample_ex(hx, hz, p, seed, shot0, batch, d_errx, d_errz, d_syn_z, d_syn_x,
                                 QLDPC_FMT_BYTES, stream);
}

extern "C" int qldpc_channel_sample_ex(const qldpc_code* hx, const qldpc_code* hz, double p, uint64_t seed,
                                       uint64_t shot0, int64_t batch, uint64_t* d_errx, uint64_t* d_errz,
                                       void* d_syn_z, void* d_syn_x, int syn_format, void* stream) {
  if (syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS) return fail(QLDPC_EINVAL, "unknown syndrome format");
  qldpc::SampleArgs a{};
  int rc = pair_tabs(hx, hz, &a.t);
  if (rc != QLDPC_OK) return rc;
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  rc = qldpc_channel_thresholds(p, &a.t1, &a.t2, &a.t3);
  if (rc != QLDPC_OK) return rc;
  if (batch == 0) return QLDPC_OK;
  if (!d_errx || !d_errz || (a.t.mz && !d_syn_z) || (a.t.mx && !d_syn_x))
    return fail(QLDPC_EINVAL, "null device buffer");
  a.errx = d_errx;
  a.errz = d_errz;
  a.syz = (uint8_t*)d_syn_z;
  a.syx = (uint8_t*)d_syn_x;
  a.syn_bits = syn_format == QLDPC_FMT_BITS;
  a.batch = batch;
  a.shot0 = shot0;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32);
  HIP_TRY(qldpc::launch_channel_sample(a, channel_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

// ---------------------------------------------------------------------------
// inhomogeneous Pauli channel: per-qubit thresholds, uploaded once per handle
// ---------------------------------------------------------------------------
struct qldpc_channel {
  const qldpc_code* hx = nullptr;
  const qldpc_code* hz = nullptr;
  int mx = 0, mz = 0, ex = 0, ez = 0, n = 0;   // the pair's shapes when the table was built
  int device = -1;
  std::vector<uint64_t> thr;                   // [3][n]
  DevBuf<uint64_t> d_thr;
};

extern "C" int qldpc_channel_table(const double* px, const double* py, const double* pz, int n, uint64_t* t) {
  if (n < 0) return fail(QLDPC_EINVAL, "negative n");
  if (n > 0 && (!px || !py || !pz || !t)) return fail(QLDPC_EINVAL, "null argument");
  const double two32 = 4294967296.0;
  for (int j = 0; j < n; ++j) {
    const double xy = px[j] + py[j], xyz = xy + pz[j];
    if (!(px[j] >= 0.0 && py[j] >= 0.0 && pz[j] >= 0.0 && xyz <= 1.0))   // (NaN fails)
      return fail(QLDPC_EINVAL, "qubit %d: (px, py, pz) = (%g, %g, %g) must be >= 0 with a sum <= 1", j, px[j], py[j],
                  pz[j]);
    t[j] = (uint64_t)std::min(two32, std::floor(px[j] * two32));
    t[(size_t)n + j] = (uint64_t)std::min(two32, std::floor(xy * two32));
    t[2 * (size_t)n + j] = (uint64_t)std::min(two32, std::floor(xyz * two32));
  }
  return QLDPC_OK;
}

extern "C" int qldpc_channel_create(const qldpc_code* hx, const qldpc_code* hz, const double* h_px, const double* h_py,
                                    const double* h_pz, qldpc_channel** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!hx || !hz) return fail(QLDPC_EINVAL, "code is null");
  if (hx->n != hz->n)
    return fail(QLDPC_EINVAL, "Hx and Hz must have the same number of columns (physical qubits).");
  if (hx->device != hz->device) return fail(QLDPC_EINVAL, "Hx and Hz live on different devices");
  if ((hx->n + 63) / 64 > 64) return fail(QLDPC_EUNSUP, "the channel kernels support n <= 4096 qubits (got %d)", hx->n);
  std::unique_ptr<qldpc_channel> ch(new qldpc_channel());
  ch->hx = hx, ch->hz = hz;
  ch->mx = hx->m, ch->mz = hz->m, ch->ex = hx->E, ch->ez = hz->E, ch->n = hx->n, ch->device = hx->device;
  ch->thr.resize(3 * (size_t)ch->n);
  if (int rc = qldpc_channel_table(h_px, h_py, h_pz, ch->n, ch->thr.data())) return rc;
  if (ch->device >= 0) {                               // (no visible device: the handle is still made)
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ch->device)
      return fail(QLDPC_EINVAL, "codes live on device %d, current device is %d", ch->device, dev);
    HIP_TRY(ch->d_thr.upload(ch->thr));
  }
  *out = ch.release();
  return QLDPC_OK;
}

extern "C" int qldpc_channel_destroy(qldpc_channel* ch) {
  delete ch;
  return QLDPC_OK;
}

extern "C" int qldpc_channel_sample_vec(const qldpc_channel* ch, uint64_t seed, uint64_t shot0, int64_t batch,
                                        uint64_t* d_errx, uint64_t* d_errz, void* d_syn_z, void* d_syn_x,
                                        int syn_format, void* stream) {
  if (!ch) return fail(QLDPC_EINVAL, "channel handle is null");
  if (syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS)
    return fail(QLDPC_EINVAL, "unknown syndrome format");
  const qldpc_code *hx = ch->hx, *hz = ch->hz;
  if (ch->n != hx->n || ch->n != hz->n || ch->mx != hx->m || ch->mz != hz->m || ch->ex != hx->E || ch->ez != hz->E)
    return fail(QLDPC_EINVAL, "the channel handle was built for another code pair");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (batch == 0) return QLDPC_OK;
  if (!d_errx || !d_errz || (hz->m && !d_syn_z) || (hx->m && !d_syn_x))
    return fail(QLDPC_EINVAL, "null device buffer");
  qldpc::SampleVecArgs va{};
  qldpc::SampleArgs& a = va.s;
  int rc = pair_tabs(hx, hz, &a.t);                    // no device: QLDPC_EHIP
  if (rc != QLDPC_OK) return rc;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != ch->device) return fail(QLDPC_EINVAL, "codes live on device %d, current device is %d", ch->device, dev);
  va.thr = ch->d_thr;
  a.errx = d_errx;
  a.errz = d_errz;
  a.syz = (uint8_t*)d_syn_z;
  a.syx = (uint8_t*)d_syn_x;
  a.syn_bits = syn_format == QLDPC_FMT_BITS;
  a.batch = batch;
  a.shot0 = shot0;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32);
  HIP_TRY(qldpc::launch_channel_sample_vec(va, channel_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

extern "C" int qldpc_count_outcomes(const qldpc_code* hx, const qldpc_code* hz, int64_t batch,
                                    const uint64_t* d_errx, const uint64_t* d_errz, const uint8_t* d_syn_z,
                                    const uint8_t* d_syn_x, const uint8_t* d_ehat_x, const uint8_t* d_ehat_z,
                                    const int32_t* d_iters_x, const int32_t* d_iters_z, int64_t* d_counters,
                                    void* stream) {
  return qldpc_count_outcomes_ex(hx, hz, batch, d_errx, d_errz, d_syn_z, d_syn_x, QLDPC_FMT_BYTES, d_ehat_x,
                                 d_ehat_z, QLDPC_FMT_BYTES, d_iters_x, d_iters_z, d_counters, stream);
}

extern "C" int qldpc_count_outcomes_ex(const qldpc_code* hx, const qldpc_code* hz, int64_t batch,
                                       const uint64_t* d_errx, const uint64_t* d_errz, const void* d_syn_z,
                                       const void* d_syn_x, int syn_format, const void* d_ehat_x,
                                       const void* d_ehat_z, int ehat_format, const int32_t* d_iters_x,
                                       const int32_t* d_iters_z, int64_t* d_counters, void* stream) {
  if ((syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  qldpc::CountArgs a{};
  int rc = pair_tabs(hx, hz, &a.t);
  if (rc != QLDPC_OK) return rc;
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (batch == 0) return QLDPC_OK;
  if (!d_errx || !d_errz || (a.t.mz && !d_syn_z) || (a.t.mx && !d_syn_x) || !d_ehat_x || !d_ehat_z ||
      !d_iters_x || !d_iters_z || !d_counters)
    return fail(QLDPC_EINVAL, "null device buffer");
  a.errx = d_errx;
  a.errz = d_errz;
  a.syz = (const uint8_t*)d_syn_z;
  a.syx = (const uint8_t*)d_syn_x;
  a.ehx = (const uint8_t*)d_ehat_x;
  a.ehz = (const uint8_t*)d_ehat_z;
  a.syn_bits = syn_format == QLDPC_FMT_BITS;
  a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.itx = d_iters_x;
  a.itz = d_iters_z;
  a.acc = reinterpret_cast<unsigned long long*>(d_counters);
  a.batch = batch;
  HIP_TRY(qldpc::launch_count_outcomes(a, channel_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

// ---------------------------------------------------------------------------
// logical operators of a CSS pair: both tables bit-packed word-major
// ([W][kp], kp = k padded to 64) and uploaded once
// ---------------------------------------------------------------------------
struct qldpc_logicals {
  const qldpc_code* hx = nullptr;
  const qldpc_code* hz = nullptr;
  int mx = 0, mz = 0, ex = 0, ez = 0;   // the pair's shapes when the tables were built
  int n = 0, W = 0, k = 0, kp = 0, device = -1;
  DevBuf<uint64_t> d_tab_z, d_tab_x;    // Lz (tests errX ^ eX), Lx (tests errZ ^ eZ)
};

static std::vector<uint64_t> pack_word_major(const uint8_t* L, int k, int kp, int n, int W) {
  std::vector<uint64_t> tab((size_t)W * kp, 0);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < n; ++j)
      if (L[(size_t)i * n + j] & 1) tab[(size_t)(j >> 6) * kp + i] |= 1ull << (j & 63);
  return tab;
}

extern "C" int qldpc_logicals_create(const qldpc_code* hx, const qldpc_code* hz, const uint8_t* h_Lx,
                                     const uint8_t* h_Lz, int k, qldpc_logicals** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!hx || !hz) return fail(QLDPC_EINVAL, "code is null");
  if (hx->n != hz->n)
    return fail(QLDPC_EINVAL, "Hx and Hz must have the same number of columns (physical qubits).");
  if (hx->device != hz->device) return fail(QLDPC_EINVAL, "Hx and Hz live on different devices");
  if (k < 0 || k > hx->n) return fail(QLDPC_EINVAL, "k = %d logical qubits for n = %d", k, hx->n);
  if (k > 0 && (!h_Lx || !h_Lz)) return fail(QLDPC_EINVAL, "logical operator matrix is null");
  const int W = (hx->n + 63) / 64;
  if (W > 64) return fail(QLDPC_EUNSUP, "the channel kernels support n <= 4096 qubits (got %d)", hx->n);
  std::unique_ptr<qldpc_logicals> lg(new qldpc_logicals());
  lg->hx = hx, lg->hz = hz;
  lg->mx = hx->m, lg->mz = hz->m, lg->ex = hx->E, lg->ez = hz->E;
  lg->n = hx->n, lg->W = W, lg->k = k, lg->kp = (k + 63) & ~63, lg->device = hx->device;
  // No visible device: the handle is still made (argument checks work); the
  // counter entry point then fails loudly.
  if (lg->device >= 0) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != lg->device)
      return fail(QLDPC_EINVAL, "codes live on device %d, current device is %d", lg->device, dev);
    HIP_TRY(lg->d_tab_z.upload(pack_word_major(h_Lz, k, lg->kp, lg->n, W)));
    HIP_TRY(lg->d_tab_x.upload(pack_word_major(h_Lx, k, lg->kp, lg->n, W)));
  }
  *out = lg.release();
  return QLDPC_OK;
}

extern "C" int qldpc_logicals_destroy(qldpc_logicals* lg) {
  delete lg;                                         // the tables own themselves
  return QLDPC_OK;
}

extern "C" int qldpc_count_logical_ex(const qldpc_code* hx, const qldpc_code* hz, const qldpc_logicals* lg,
                                      int64_t batch, const uint64_t* d_errx, const uint64_t* d_errz,
                                      const void* d_syn_z, const void* d_syn_x, int syn_format,
                                      const void* d_ehat_x, const void* d_ehat_z, int ehat_format,
                                      const int32_t* d_iters_x, const int32_t* d_iters_z, int64_t* d_counters,
                                      uint8_t* d_class_x, uint8_t* d_class_z, uint64_t* d_flip_x,
                                      uint64_t* d_flip_z, void* stream) {
  // every argument check comes before the first HIP call
  if (!hx || !hz) return fail(QLDPC_EINVAL, "code is null");
  if (!lg) return fail(QLDPC_EINVAL, "logicals handle is null");
  if (hx->n != hz->n)
    return fail(QLDPC_EINVAL, "Hx and Hz must have the same number of columns (physical qubits).");
  if (lg->hx != hx || lg->hz != hz || lg->n != hx->n || lg->mx != hx->m || lg->mz != hz->m || lg->ex != hx->E ||
      lg->ez != hz->E)
    return fail(QLDPC_EINVAL, "the logicals handle was built for another code pair");
  if (lg->device != hx->device || lg->device != hz->device)
    return fail(QLDPC_EINVAL, "the logicals handle was built on another device");
  if ((syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  if ((hx->n + 63) / 64 > 64)
    return fail(QLDPC_EUNSUP, "the channel kernels support n <= 4096 qubits (got %d)", hx->n);
  const int64_t mode = opt(&Options::logical_tabs);
  if (mode < 0 || mode > 2) return fail(QLDPC_EINVAL, "option logical_tabs must be 0, 1 or 2");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (batch == 0) return QLDPC_OK;
  if (!d_errx || !d_errz || (hz->m && !d_syn_z) || (hx->m && !d_syn_x) || !d_ehat_x || !d_ehat_z || !d_iters_x ||
      !d_iters_z || !d_counters)
    return fail(QLDPC_EINVAL, "null device buffer");
  qldpc::LogicalArgs la{};
  qldpc::CountArgs& a = la.c;
  int rc = pair_tabs(hx, hz, &a.t);                  // no device: QLDPC_EHIP
  if (rc != QLDPC_OK) return rc;
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != lg->device) return fail(QLDPC_EINVAL, "codes live on device %d, current device is %d", lg->device, dev);
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  // table residency: staged in LDS when they fit a workgroup's LDS next to the
  // CSR tables and the per-wave slots and stay within kLogicalLdsTabBytes
  // (DESIGN.md §3.5), else read from global memory (L2-resident)
  const bool fits = qldpc::logical_lds_bytes(a.t, lg->kp, true) <= max_lds;
  if (mode == 1 && !fits)
    return fail(QLDPC_EUNSUP, "logical_tabs=1: the tables need %d B of LDS, the device has %d",
                qldpc::logical_lds_bytes(a.t, lg->kp, true), max_lds);
  la.tabs_lds = mode == 1 || (mode == 0 && fits && 2ll * 8 * a.t.W * lg->kp <= kLogicalLdsTabBytes);
  if (qldpc::logical_lds_bytes(a.t, lg->kp, la.tabs_lds != 0) > max_lds)
    return fail(QLDPC_EUNSUP, "the logical counter kernel needs %d B of LDS for these codes",
                qldpc::logical_lds_bytes(a.t, lg->kp, la.tabs_lds != 0));
  a.errx = d_errx;
  a.errz = d_errz;
  a.syz = (const uint8_t*)d_syn_z;
  a.syx = (const uint8_t*)d_syn_x;
  a.ehx = (const uint8_t*)d_ehat_x;
  a.ehz = (const uint8_t*)d_ehat_z;
  a.syn_bits = syn_format == QLDPC_FMT_BITS;
  a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.itx = d_iters_x;
  a.itz = d_iters_z;
  a.acc = reinterpret_cast<unsigned long long*>(d_counters);
  a.batch = batch;
  la.tab_z = lg->d_tab_z;
  la.tab_x = lg->d_tab_x;
  la.k = lg->k;
  la.kp = lg->kp;
  la.class_x = d_class_x;
  la.class_z = d_class_z;
  la.flip_x = d_flip_x;
  la.flip_z = d_flip_z;
  HIP_TRY(qldpc::launch_count_logical(la, channel_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

static_assert(QLDPC_CHANNEL_SAMPLE == qldpc::kChannelSample && QLDPC_CHANNEL_SAMPLE_VEC == qldpc::kChannelSampleVec &&
              QLDPC_CHANNEL_COUNT == qldpc::kChannelCount && QLDPC_CHANNEL_COUNT_LOGICAL == qldpc::kChannelCountLogical,
              "qldpc_decoder.h names the kernels as channel_kernels.h does");

// The instance channel_choice picks, as the launchers do. Needs no device.
extern "C" int qldpc_channel_kernel_name(const qldpc_code* hx, const qldpc_code* hz, int kind, int est_aligned,
                                         int tabs_lds, char* buf, int len) {
  if (!buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  qldpc::PairTabs t{};
  if (int rc = pair_shape(hx, hz, &t)) return rc;
  if (int rc = pair_limit(t)) return rc;
  if (!qldpc::channel_kernel_name(kind, qldpc::channel_choice(t, est_aligned != 0, tabs_lds != 0), buf, len))
    return fail(QLDPC_EINVAL, "unknown channel kernel kind %d", kind);
  return QLDPC_OK;
}
