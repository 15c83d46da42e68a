// capi_dem.cpp — detector error models: the handle (thresholds and the stacked
// matrix [H; L] column by column), the device shot source and the outcome
// counter (dem_kernels.hip).

#include <cmath>
#include <memory>

#include "capi_internal.h"
#include "dem_kernels.h"

using namespace capi;

struct qldpc_dem {
  const qldpc_code* code = nullptr;
  int m = 0, n = 0, E = 0;            // the code's shape when the handle was built
  int k = 0, device = -1;
  long long edges = 0;                // entries of [H; L]
  qldpc::DemTabs t{};                 // shapes; the table pointers only with a device
  DevBuf<uint32_t> d_thr;
  DevBuf<int32_t> d_cp;
  DevBuf<uint16_t> d_tg16;
  DevBuf<uint32_t> d_tg32;
};

static int dem_device(const qldpc_dem* dem, int* max_lds) {
  if (dem->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the model was created");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != dem->device) return fail(QLDPC_EINVAL, "model lives on device %d, current device is %d", dem->device, dev);
  HIP_TRY(hipDeviceGetAttribute(max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  if (qldpc::dem_lds_bytes(dem->t) > *max_lds)
    return fail(QLDPC_EUNSUP, "the detector error model kernels need %lld B of LDS for %d detectors and %d "
                "observables, the device has %d", qldpc::dem_lds_bytes(dem->t), dem->t.M, dem->t.K, *max_lds);
  return QLDPC_OK;
}

static int dem_grid(int64_t batch) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  const int64_t need = (batch + qldpc::kDemWaves - 1) / qldpc::kDemWaves;
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, (int64_t)cus * 8));
}

// the handle was built for this code as it is now
static int dem_alive(const qldpc_dem* dem) {
  if (!dem) return fail(QLDPC_EINVAL, "detector error model handle is null");
  const qldpc_code* c = dem->code;
  if (c->m != dem->m || c->n != dem->n || c->E != dem->E)
    return fail(QLDPC_EINVAL, "the detector error model handle was built for another code");
  return QLDPC_OK;
}

extern "C" int qldpc_dem_create(const qldpc_code* code, const uint8_t* h_L, int k, const double* h_priors,
                                qldpc_dem** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (k < 0) return fail(QLDPC_EINVAL, "k = %d observables", k);
  const int M = code->m, N = code->n;
  if (k > 0 && N > 0 && !h_L) return fail(QLDPC_EINVAL, "observable matrix is null");
  if (N > 0 && !h_priors) return fail(QLDPC_EINVAL, "priors are null");
  for (int j = 0; j < N; ++j)
    if (!(h_priors[j] >= 0.0 && h_priors[j] < 1.0))
      return fail(QLDPC_EINVAL, "prior %d must lie in [0, 1) (got %g)", j, h_priors[j]);
  const long long MW = (M + 63) / 64, KW = ((long long)k + 63) / 64;
  if (64 * (MW + KW) > qldpc::kDemMaxRowBits || N > qldpc::kDemMaxColumns)
    return fail(QLDPC_EUNSUP, "the detector error model kernels support ceil(M/64) + ceil(K/64) <= %d words and "
                "N <= %d (got M = %d, K = %d, N = %d)", qldpc::kDemMaxRowBits / 64, qldpc::kDemMaxColumns, M, k, N);
  std::unique_ptr<qldpc_dem> dem(new qldpc_dem());
  dem->code = code;
  dem->m = M, dem->n = N, dem->E = code->E, dem->k = k, dem->device = code->device;
  qldpc::DemTabs& t = dem->t;
  t.M = M, t.K = k, t.N = N;
  t.MW = (int)MW, t.KW = (int)KW, t.NW = (N + 63) / 64;
  t.wide = 64 * (MW + KW) > 65536;
  // column pointers of [H; L]: H's rows ascending (CSR order), then L's
  std::vector<int32_t> cp((size_t)N + 1, 0);
  for (int e = 0; e < code->E; ++e) cp[code->col_idx[e] + 1]++;
  long long edges = code->E;
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < N; ++j)
      if (h_L[(size_t)i * N + j] & 1) {
        cp[j + 1]++;
        ++edges;
      }
  if (edges > 0x7fffffffll) return fail(QLDPC_EUNSUP, "%lld entries in [H; L]: past 32-bit column pointers", edges);
  dem->edges = edges;
  for (int j = 0; j < N; ++j) cp[j + 1] += cp[j];
  // No visible device: the handle is still made (argument checks and the
  // kernel's name work); the launches then fail loudly.
  if (dem->device >= 0) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != dem->device)
      return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", dem->device, dev);
    std::vector<uint32_t> tg((size_t)edges, 0);
    std::vector<int32_t> fill(cp.begin(), cp.end() - 1);
    for (int r = 0; r < M; ++r)
      for (int e = code->row_ptr[r]; e < code->row_ptr[r + 1]; ++e) tg[fill[code->col_idx[e]]++] = (uint32_t)r;
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < N; ++j)
        if (h_L[(size_t)i * N + j] & 1) tg[fill[j]++] = (uint32_t)(64 * MW + i);
    std::vector<uint32_t> thr((size_t)N);
    // floor(p 2^32), what qldpc_channel_table(p, 0, 0) yields: below 2^32 for p < 1
    for (int j = 0; j < N; ++j) thr[j] = (uint32_t)std::floor(h_priors[j] * 4294967296.0);
    HIP_TRY(dem->d_thr.upload(thr));
    HIP_TRY(dem->d_cp.upload(cp));
    if (t.wide) {
      HIP_TRY(dem->d_tg32.upload(tg));
      t.tg = dem->d_tg32;
    } else {
      HIP_TRY(dem->d_tg16.upload(std::vector<uint16_t>(tg.begin(), tg.end())));
      t.tg = dem->d_tg16;
    }
    t.thr = dem->d_thr;
    t.cp = dem->d_cp;
  }
  *out = dem.release();
  return QLDPC_OK;
}

extern "C" int qldpc_dem_destroy(qldpc_dem* dem) {
  delete dem;                                        // the tables own themselves
  return QLDPC_OK;
}

extern "C" int qldpc_dem_sample(const qldpc_dem* dem, uint64_t seed, uint64_t shot0, int64_t batch, void* d_det,
                                int det_format, uint64_t* d_obs, uint64_t* d_fired, void* stream) {
  // every argument check comes before the first HIP call
  if (int rc = dem_alive(dem)) return rc;
  if (det_format != QLDPC_FMT_BYTES && det_format != QLDPC_FMT_BITS)
    return fail(QLDPC_EINVAL, "unknown detector format");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if ((dem->t.M && !d_det) || (dem->t.K && !d_obs)) return fail(QLDPC_EINVAL, "null device buffer");
  if (batch == 0) return QLDPC_OK;
  int max_lds = 0;
  if (int rc = dem_device(dem, &max_lds)) return rc;
  qldpc::DemSampleArgs a{};
  a.t = dem->t;
  a.det = (uint8_t*)d_det;
  a.det_bits = det_format == QLDPC_FMT_BITS;
  a.obs = d_obs;
  a.fired = d_fired;
  a.batch = batch;
  a.shot0 = shot0;
  a.key0 = (uint32_t)seed;
  a.key1 = (uint32_t)(seed >> 32);
  HIP_TRY(qldpc::launch_dem_sample(a, dem_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

extern "C" int qldpc_dem_count(const qldpc_dem* dem, int64_t batch, const void* d_det, int det_format,
                               const uint64_t* d_obs, const void* d_ehat, int ehat_format, const int32_t* d_iters,
                               int64_t* d_counters, uint8_t* d_class, uint64_t* d_flips, void* stream) {
  // every argument check comes before the first HIP call
  if (int rc = dem_alive(dem)) return rc;
  if ((det_format != QLDPC_FMT_BYTES && det_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown detector / estimate format");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if ((dem->t.M && !d_det) || (dem->t.K && !d_obs) || (dem->t.N && !d_ehat) || !d_iters || !d_counters)
    return fail(QLDPC_EINVAL, "null device buffer");
  if (batch == 0) return QLDPC_OK;
  int max_lds = 0;
  if (int rc = dem_device(dem, &max_lds)) return rc;
  qldpc::DemCountArgs a{};
  a.t = dem->t;
  a.det = (const uint8_t*)d_det;
  a.det_bits = det_format == QLDPC_FMT_BITS;
  a.obs = d_obs;
  a.ehat = (const uint8_t*)d_ehat;
  a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.iters = d_iters;
  a.acc = reinterpret_cast<unsigned long long*>(d_counters);
  a.cls = d_class;
  a.flips = d_flips;
  a.batch = batch;
  HIP_TRY(qldpc::launch_dem_count(a, dem_grid(batch), (hipStream_t)stream));
  return QLDPC_OK;
}

static_assert(QLDPC_DEM_SAMPLE == qldpc::kDemSample && QLDPC_DEM_COUNT == qldpc::kDemCount,
              "qldpc_decoder.h names the kernels as dem_kernels.h does");

// The instance the launchers pick. Needs no device.
extern "C" int qldpc_dem_kernel_name(const qldpc_dem* dem, int kind, char* buf, int len) {
  if (!buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  if (int rc = dem_alive(dem)) return rc;
  if (!qldpc::dem_kernel_name(kind, dem->t.wide != 0, buf, len))
    return fail(QLDPC_EINVAL, "unknown detector error model kernel kind %d", kind);
  return QLDPC_OK;
}
