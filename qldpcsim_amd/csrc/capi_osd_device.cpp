// capi_osd_device.cpp — GPU OSD launchers (osd_kernels.hip): one workgroup
// per shot.

#include <cstdio>

#include "capi_internal.h"
#include "osd_kernels.h"

using namespace capi;

static int setdiff_table_ints(int n) {
  // largest (new table + old table) CPython's set reaches inserting n keys
  size_t mask = 7, fill = 0, best = 16;
  for (int used = 1; used <= n; ++used) {
    ++fill;
    if (fill * 5 >= mask * 3) {
      const size_t minused = used > 50000 ? (size_t)used * 2 : (size_t)used * 4;
      size_t ns = 8;
      while (ns <= minused) ns <<= 1;
      best = std::max(best, ns + mask + 1);
      mask = ns - 1;
    }
  }
  return (int)best;
}

struct SpillCfg {  // status-2 spill buffers (OsdArgs::spill_*); empty = none
  double* post = nullptr;
  int32_t* idx = nullptr;
  int32_t* count = nullptr;
  int64_t cap = 0;
};

// Per-device state the launchers share, created on first use under mu and
// kept for the life of the process
static struct OsdDeviceState {
  std::mutex mu;
  unsigned long long* prof = nullptr;   // diagnostic builds (QLDPC_OSD_TIMING), option osd_prof
  // per-CU workgroup tickets of osd_block_kernel (engine SIMD choice), one
  // zeroed array per device; the counters only ever wrap
  uint32_t* tickets[64] = {};
} g_osd;

// launch(args of the chunk, its shots) for `count` shots in chunks of at most
// `chunk` (grid.x limit, scratch size); stops at the first error
template <typename Launch>
static hipError_t osd_chunks(const qldpc::OsdArgs& a, int64_t count, int64_t chunk, Launch launch) {
  hipError_t e = hipSuccess;
  for (int64_t done = 0; done < count && e == hipSuccess; done += chunk) {
    qldpc::OsdArgs ai = a;
    ai.perm += done * a.n;
    ai.syn += done * a.m;
    ai.ehat += done * a.n;
    ai.status += done;
    if (ai.tiepos) ai.tiepos += done;
    if (ai.post) ai.post += done * a.n;
    ai.shot_base = done;
    e = launch(ai, (unsigned)std::min<int64_t>(count - done, chunk));
  }
  return e;
}

// Which OSD kernel runs a code: all that (m, n, zero_col, the options, cs = 0,
// kOsdCsHamming or kOsdCsPrior) decide, without a HIP call; the launchers and qldpc_osd_kernel_name read it
struct OsdChoice {
  const void *kernel = nullptr, *kblk = nullptr;   // osd_hbm_kernel or osd_kernel<nw>; the block kernel in front of it, or null
  const char* name = "";              // of the kernel that does the work: kblk's, else kernel's
  bool hbm = false;
  int nw = 0, rt = 1;                 // row words of the instance (0 past 33); block kernel: rows per thread
  int block = 0, bblk = 0, mr = 0;    // threads of kernel and of kblk; kblk's rt * bblk row slots
};
static int cs_kind(int cs_lambda, const qldpc_prior* prior) {
  return cs_lambda < 0 ? 0 : prior ? qldpc::kOsdCsPrior : qldpc::kOsdCsHamming;
}
static int osd_threads(int rows) { return std::max(64, (rows + 63) / 64 * 64); }   // one per row, whole waves

// QLDPC_EUNSUP where cs asks for OSD-CS and the code cannot have it on the device:
// it is osd_block_kernel's epilogue (that kernel's range, and no other kernel)
static int choose_osd_kernel(const qldpc_code* code, int cs, OsdChoice* c) {
  const int m = code->m, n = code->n;
  const bool column = opt(&Options::osd_column) != 0, hbm = opt(&Options::osd_hbm) != 0;
  const char* why = !cs                     ? nullptr
                    : m > 512 || n > 1087   ? "m <= 512 and n <= 1087 (the block kernel's range)"
                    : code->zero_col        ? "an H without all-zero columns"
                    : column || hbm         ? "options osd_column and osd_hbm off"
                                            : nullptr;
  if (why) return fail(QLDPC_EUNSUP, "OSD-CS on the device needs %s", why);
  *c = OsdChoice{};
  c->nw = qldpc::osd_nw_of((n + 1 + 63) / 64);
  // past the register / LDS kernels (m > 1024 rows, n > 2111 columns) or option osd_hbm: osd_hbm_kernel
  c->hbm = m > 1024 || !c->nw || hbm;
  c->block = c->hbm ? std::min(1024, osd_threads(m)) : osd_threads(m);
  c->kernel = c->hbm ? qldpc::osd_hbm_kernel_ptr(&c->name) : qldpc::select_osd_kernel(c->nw, &c->name);
  // The block kernel leaves two cases to REF's own row order (osd_block.h): an
  // H with an all-zero column (the column kernel for the whole code) and a
  // syndrome outside H's column space (those shots to the column kernel's redo
  // pass behind it). Option osd_column: the column kernel alone (A/B, tests)
  if (c->hbm || column || code->zero_col) return QLDPC_OK;
  c->kblk = qldpc::select_osd_block_kernel(c->nw, m, cs, &c->rt, &c->name);
  c->bblk = osd_threads((m + c->rt - 1) / c->rt);
  c->mr = c->rt * c->bblk;
  return QLDPC_OK;
}

// osd_hbm_kernel: one workgroup per shot, the shot's working matrix in a
// per-shot slice of a stream-ordered scratch allocation (chunks of at most
// 1 GiB of slices), LDS = one 64-bit word per row + small
static int osd_hbm_impl(const qldpc_code* code, const OsdChoice& c, qldpc::OsdArgs a, int64_t count, int max_lds,
                        hipStream_t st) {
  const int m = code->m, n = code->n;
  const int nwr = (n + 1 + 63) / 64, mp = (m + 63) / 64 * 64;
  const size_t lds = qldpc::osd_hbm_lds(m, nwr);
  if (lds > (size_t)max_lds)
    return fail(QLDPC_EUNSUP, "GPU OSD keeps one word per row in LDS: m = %d needs %zu B (at most %d)", m, lds,
                max_lds);
  const void* k = c.kernel;
  // the device's limit, not this code's size: concurrent calls set one value
  HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
  code_osd_prep(code);
  a.rank = code->rank;
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  qldpc::OsdHbmArgs h{};
  size_t off = up((size_t)8 * nwr * mp);
  h.off_inv = (int)off;
  off = up(off + 4 * (size_t)n);
  h.off_jl = (int)off;
  off = up(off + 4 * ((size_t)m + 2));
  h.off_inj = (int)off;
  off = up(off + (size_t)n);
  h.off_table = (int)off;
  if (a.order == 1) off = up(off + 4 * (size_t)setdiff_table_ints(n));
  if (off > (size_t)INT32_MAX) return fail(QLDPC_EUNSUP, "GPU OSD scratch per shot exceeds 2 GiB (m = %d, n = %d)", m, n);
  h.stride = (long long)off;
  h.nwr = nwr;
  h.mp = mp;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(count, 1 << 30),
                                                                   ((int64_t)1 << 30) / (int64_t)off));
  void* scr = nullptr;
  HIP_TRY(hipMallocAsync(&scr, (size_t)chunk * off, st));
  h.scratch = (unsigned char*)scr;
  const hipError_t e = osd_chunks(a, count, chunk, [&](qldpc::OsdArgs& ai, unsigned g) {
    void* params[] = {(void*)&ai, (void*)&h};
    return hipLaunchKernel(k, dim3(g), dim3(c.block), params, lds, st);
  });
  const hipError_t ef = hipFreeAsync(scr, st);
  HIP_TRY(e);
  HIP_TRY(ef);
  return QLDPC_OK;
}

// cs_lambda < 0: the reference's OSD of `order`; else OSD-CS (order unused;
// the _cs entry points have checked lambda's range), with the prior-weighted
// cost where `prior` is given (checked by the _cs_prior entry points)
static int osd_device_impl(const qldpc_code* code, int64_t count, const uint8_t* d_syn, const int32_t* d_perm,
                           const int32_t* d_tiepos, const double* d_post, int order, int cs_lambda,
                           uint8_t* d_ehat, int32_t* d_status, void* stream, const SpillCfg& spill = {},
                           const qldpc_prior* prior = nullptr) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  const bool cs = cs_lambda >= 0;
  OsdChoice c;
  if (const int rc = choose_osd_kernel(code, cs_kind(cs_lambda, prior), &c)) return rc;
  if (cs) order = 0;                                // the base estimate, and the redo pass's semantics
  if (count < 0) return fail(QLDPC_EINVAL, "negative count");
  if (count == 0) return QLDPC_OK;
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  if (!d_syn || !d_perm || !d_ehat || !d_status) return fail(QLDPC_EINVAL, "null device buffer");
  const int m = code->m, n = code->n;
  hipStream_t st = (hipStream_t)stream;
  qldpc::OsdArgs a{};                                // buffers at the first shot; rank follows code_osd_prep
  a.row_ptr = code->d_row_ptr;
  a.col_idx = code->d_col_idx;
  a.perm = d_perm;
  a.syn = d_syn;
  a.ehat = d_ehat;
  a.status = d_status;
  a.m = m;
  a.n = n;
  a.order = order;
  a.tiepos = d_tiepos;
  a.post = d_tiepos ? d_post : nullptr;
  if (d_tiepos && spill.count) {
    a.spill_post = spill.post;
    a.spill_idx = spill.idx;
    a.spill_count = spill.count;
    a.spill_cap = spill.cap;
  }
  a.cs_lambda = cs ? cs_lambda : 0;
  if (cs && prior) {
    if (code->device >= 0 && !prior->d_Wo.p) return fail(QLDPC_EINVAL, "the prior handle holds no device weights");
    for (const int64_t w : prior->Wo)                 // (holds by construction: |L| < 750)
      if (w >= (1ll << 30) || w <= -(1ll << 30)) return fail(QLDPC_EUNSUP, "OSD-CS prior weight past 2^30");
    a.cs_w = prior->d_Wo.p;
  }
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  if (c.hbm) return osd_hbm_impl(code, c, a, count, max_lds, st);
  // the device's LDS limit is the one thing the choice does not know: past it
  // the column kernel refuses and the block kernel steps aside
  const int tab = order == 1 ? setdiff_table_ints(n) : 0;
  const size_t lds_col = qldpc::osd_column_lds(m, n, c.nw, tab), lds_blk = qldpc::osd_block_lds(m, n, c.nw, c.mr, tab);
  const void *kcol = c.kernel, *kblk = c.kblk;
  if (lds_col > (size_t)max_lds) return fail(QLDPC_EUNSUP, "GPU OSD needs %zu B LDS", lds_col);
  HIP_TRY(hipFuncSetAttribute(kcol, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
  if (kblk && lds_blk > (size_t)max_lds) kblk = nullptr;
  // OSD-CS has the block kernel alone, and works in its block-loop LDS (Wd .. CT)
  const size_t cs_need = prior ? qldpc::osd_cs_prior_lds(c.nw, c.mr) : qldpc::osd_cs_lds(c.nw, c.mr);
  if (cs && (!kblk || cs_need > qldpc::osd_block_cs_room(c.nw, c.mr)))
    return fail(QLDPC_EUNSUP, "OSD-CS on the device needs the block kernel (m = %d, n = %d)", m, n);
  if (kblk) HIP_TRY(hipFuncSetAttribute(kblk, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
  // rank(H) and the column bit-vectors: built on first use, after every
  // cheap refusal above (a large HBM-path code is refused without them)
  code_osd_prep(code);
  a.rank = code->rank;
  {
    std::lock_guard<std::mutex> lk(g_osd.mu);
    if (opt(&Options::osd_prof) && !g_osd.prof) {
      HIP_TRY(hipMalloc(&g_osd.prof, 16 * sizeof(unsigned long long)));
      HIP_TRY(hipMemset(g_osd.prof, 0, 16 * sizeof(unsigned long long)));
    }
    a.prof = g_osd.prof;
    const bool use_tickets = opt(&Options::osd_tickets) != 0 && dev >= 0 && dev < 64;
    if (use_tickets && !g_osd.tickets[dev]) {
      HIP_TRY(hipMalloc(&g_osd.tickets[dev], sizeof(uint32_t) * qldpc::kOsdCuSlots));
      HIP_TRY(hipMemset(g_osd.tickets[dev], 0, sizeof(uint32_t) * qldpc::kOsdCuSlots));
    }
    a.cu_tickets = use_tickets ? g_osd.tickets[dev] : nullptr;
  }
  const hipError_t launched = osd_chunks(a, count, 1 << 30, [&](qldpc::OsdArgs& ai, unsigned g) {
    void* params[] = {(void*)&ai};
    hipError_t e = hipSuccess;
    if (kblk) {
      e = hipLaunchKernel(kblk, dim3(g), dim3(c.bblk), params, lds_blk, st);
      ai.redo = 1;                                    // same stream: runs after the block pass
    }
    if (e == hipSuccess) e = hipLaunchKernel(kcol, dim3(g), dim3(c.block), params, lds_col, st);
    return e;
  });
  HIP_TRY(launched);
  if (a.prof) {
    unsigned long long h[16];
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(h, a.prof, sizeof(h), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(a.prof, 0, sizeof(h)));
    fprintf(stderr, "osd_prof shots=%lld", (long long)count);
    for (int i = 0; i < 14; ++i) fprintf(stderr, " %.0f", (double)h[i] / (double)count);
    fprintf(stderr, "\n");
  }
  return QLDPC_OK;
}

extern "C" int qldpc_osd_device(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                const int32_t* d_perm, int order, uint8_t* d_ehat, int32_t* d_status,
                                void* stream) {
  return osd_device_impl(code, count, d_syn, d_perm, nullptr, nullptr, order, -1, d_ehat, d_status, stream);
}

static int cs_lambda_checked(int lambda) {
  if (lambda < 0 || lambda > QLDPC_OSD_CS_MAX_LAMBDA)
    return fail(QLDPC_EINVAL, "OSD-CS lambda must lie in 0..%d (got %d)", QLDPC_OSD_CS_MAX_LAMBDA, lambda);
  return QLDPC_OK;
}

extern "C" int qldpc_osd_device_cs(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                   const int32_t* d_perm, int lambda, uint8_t* d_ehat, int32_t* d_status,
                                   void* stream) {
  if (const int rc = cs_lambda_checked(lambda)) return rc;
  return osd_device_impl(code, count, d_syn, d_perm, nullptr, nullptr, 0, lambda, d_ehat, d_status, stream);
}

extern "C" int qldpc_osd_order_device(const qldpc_code* code, int64_t count, const double* d_post,
                                      int32_t* d_perm, int32_t* d_tiepos, void* stream) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (count < 0) return fail(QLDPC_EINVAL, "negative count");
  if (count == 0) return QLDPC_OK;
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  if (!d_post || !d_perm || !d_tiepos) return fail(QLDPC_EINVAL, "null device buffer");
  const int n = code->n;
  if (n < 1 || n > 2048) return fail(QLDPC_EUNSUP, "the device reliability order supports 1 <= n <= 2048 (got %d)", n);
  qldpc::OrderArgs a{};
  a.post = d_post;
  a.perm = d_perm;
  a.tiepos = d_tiepos;
  a.n = n;
  HIP_TRY(qldpc::launch_osd_order(a, count, (hipStream_t)stream));
  return QLDPC_OK;
}

extern "C" int qldpc_osd_device_ordered(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                        const double* d_post, int order, uint8_t* d_ehat, int32_t* d_status,
                                        int32_t* d_perm, int32_t* d_tiepos, void* stream) {
  return qldpc_osd_device_ordered_ex(code, count, d_syn, d_post, order, d_ehat, d_status, d_perm, d_tiepos,
                                     nullptr, nullptr, nullptr, 0, stream);
}

static int osd_ordered_impl(const qldpc_code* code, int64_t count, const uint8_t* d_syn, const double* d_post,
                            int order, int cs_lambda, uint8_t* d_ehat, int32_t* d_status, int32_t* d_perm,
                            int32_t* d_tiepos, double* d_spill_post, int32_t* d_spill_idx, int32_t* d_spill_count,
                            int64_t spill_cap, void* stream, const qldpc_prior* prior = nullptr) {
  if (d_spill_count && (!d_spill_post || !d_spill_idx || spill_cap < 0))
    return fail(QLDPC_EINVAL, "spill buffers incomplete");
  if (d_spill_count && count > INT32_MAX) return fail(QLDPC_EINVAL, "spill indices are int32");
  OsdChoice c;                                       // (OSD-CS is refused before the order kernel's launch too)
  if (cs_lambda >= 0 && code)
    if (const int rc = choose_osd_kernel(code, cs_kind(cs_lambda, prior), &c)) return rc;
  const int rc = qldpc_osd_order_device(code, count, d_post, d_perm, d_tiepos, stream);
  if (rc != QLDPC_OK) return rc;
  return osd_device_impl(code, count, d_syn, d_perm, d_tiepos, d_post, order, cs_lambda, d_ehat, d_status, stream,
                         SpillCfg{d_spill_post, d_spill_idx, d_spill_count, spill_cap}, prior);
}

extern "C" int qldpc_osd_device_ordered_ex(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                           const double* d_post, int order, uint8_t* d_ehat, int32_t* d_status,
                                           int32_t* d_perm, int32_t* d_tiepos, double* d_spill_post,
                                           int32_t* d_spill_idx, int32_t* d_spill_count, int64_t spill_cap,
                                           void* stream) {
  return osd_ordered_impl(code, count, d_syn, d_post, order, -1, d_ehat, d_status, d_perm, d_tiepos, d_spill_post,
                          d_spill_idx, d_spill_count, spill_cap, stream);
}

extern "C" int qldpc_osd_device_ordered_cs(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                           const double* d_post, int lambda, uint8_t* d_ehat, int32_t* d_status,
                                           int32_t* d_perm, int32_t* d_tiepos, void* stream) {
  return qldpc_osd_device_ordered_ex_cs(code, count, d_syn, d_post, lambda, d_ehat, d_status, d_perm, d_tiepos,
                                        nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int qldpc_osd_device_ordered_ex_cs(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                              const double* d_post, int lambda, uint8_t* d_ehat, int32_t* d_status,
                                              int32_t* d_perm, int32_t* d_tiepos, double* d_spill_post,
                                              int32_t* d_spill_idx, int32_t* d_spill_count, int64_t spill_cap,
                                              void* stream) {
  if (const int rc = cs_lambda_checked(lambda)) return rc;
  return osd_ordered_impl(code, count, d_syn, d_post, 0, lambda, d_ehat, d_status, d_perm, d_tiepos, d_spill_post,
                          d_spill_idx, d_spill_count, spill_cap, stream);
}

extern "C" int qldpc_osd_device_cs_prior(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                         const int32_t* d_perm, int lambda, const qldpc_prior* prior,
                                         uint8_t* d_ehat, int32_t* d_status, void* stream) {
  if (const int rc = cs_lambda_checked(lambda)) return rc;
  if (const int rc = osd_cs_prior_checked(code, prior)) return rc;
  return osd_device_impl(code, count, d_syn, d_perm, nullptr, nullptr, 0, lambda, d_ehat, d_status, stream, {},
                         prior);
}

extern "C" int qldpc_osd_device_ordered_cs_prior(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                                 const double* d_post, int lambda, const qldpc_prior* prior,
                                                 uint8_t* d_ehat, int32_t* d_status, int32_t* d_perm,
                                                 int32_t* d_tiepos, void* stream) {
  return qldpc_osd_device_ordered_ex_cs_prior(code, count, d_syn, d_post, lambda, prior, d_ehat, d_status, d_perm,
                                              d_tiepos, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int qldpc_osd_device_ordered_ex_cs_prior(const qldpc_code* code, int64_t count, const uint8_t* d_syn,
                                                    const double* d_post, int lambda, const qldpc_prior* prior,
                                                    uint8_t* d_ehat, int32_t* d_status, int32_t* d_perm,
                                                    int32_t* d_tiepos, double* d_spill_post, int32_t* d_spill_idx,
                                                    int32_t* d_spill_count, int64_t spill_cap, void* stream) {
  if (const int rc = cs_lambda_checked(lambda)) return rc;
  if (const int rc = osd_cs_prior_checked(code, prior)) return rc;
  return osd_ordered_impl(code, count, d_syn, d_post, 0, lambda, d_ehat, d_status, d_perm, d_tiepos, d_spill_post,
                          d_spill_idx, d_spill_count, spill_cap, stream, prior);
}

// The kernel choose_osd_kernel picks: the block kernel's instance (NW row
// words, SL engine slots, RT rows per thread), or the kernel that runs instead
extern "C" int qldpc_osd_kernel_name(const qldpc_code* code, int cs, char* buf, int len) {
  if (!code || !buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  OsdChoice c;
  if (const int rc = choose_osd_kernel(code, cs == 2 ? qldpc::kOsdCsPrior : cs != 0 ? qldpc::kOsdCsHamming : 0, &c))
    return rc;
  snprintf(buf, len, "%s", c.name);
  return QLDPC_OK;
}
