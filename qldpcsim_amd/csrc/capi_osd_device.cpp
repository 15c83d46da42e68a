// capi_osd_device.cpp — GPU OSD launchers (osd_kernels.hip): one workgroup
// per shot.

#include <cstdio>

#include "capi_internal.h"
#include "osd_kernels.h"
#include "tuning.h"

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

// The OsdArgs fields both launchers fill alike, buffers at the first shot
// (rank follows code_osd_prep, after the launcher's cheap refusals)
static qldpc::OsdArgs osd_args(const qldpc_code* code, const uint8_t* d_syn, const int32_t* d_perm,
                               const int32_t* d_tiepos, const double* d_post, int order, uint8_t* d_ehat,
                               int32_t* d_status, const SpillCfg& spill) {
  qldpc::OsdArgs a{};
  a.row_ptr = code->d_row_ptr;
  a.col_idx = code->d_col_idx;
  a.perm = d_perm;
  a.syn = d_syn;
  a.ehat = d_ehat;
  a.status = d_status;
  a.m = code->m;
  a.n = code->n;
  a.order = order;
  a.tiepos = d_tiepos;
  a.post = d_tiepos ? d_post : nullptr;
  if (d_tiepos && spill.count) {
    a.spill_post = spill.post;
    a.spill_idx = spill.idx;
    a.spill_count = spill.count;
    a.spill_cap = spill.cap;
  }
  return a;
}

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

// osd_hbm_kernel: one workgroup per shot, the shot's working matrix in a
// per-shot slice of a stream-ordered scratch allocation (chunks of at most
// 1 GiB of slices), LDS = one 64-bit word per row + small
static int osd_hbm_impl(const qldpc_code* code, qldpc::OsdArgs a, int64_t count, int max_lds, hipStream_t st) {
  const int m = code->m, n = code->n;
  const int nwr = (n + 1 + 63) / 64, mp = (m + 63) / 64 * 64;
  const size_t lds = qldpc::osd_hbm_lds(m, nwr);
  if (lds > (size_t)max_lds)
    return fail(QLDPC_EUNSUP, "GPU OSD keeps one word per row in LDS: m = %d needs %zu B (at most %d)", m, lds,
                max_lds);
  const void* k = qldpc::osd_hbm_kernel_ptr();
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
  const int block = std::min(1024, std::max(64, mp));
  const hipError_t e = osd_chunks(a, count, chunk, [&](qldpc::OsdArgs& ai, unsigned g) {
    void* params[] = {(void*)&ai, (void*)&h};
    return hipLaunchKernel(k, dim3(g), dim3(block), params, lds, st);
  });
  const hipError_t ef = hipFreeAsync(scr, st);
  HIP_TRY(e);
  HIP_TRY(ef);
  return QLDPC_OK;
}

// The reason OSD-CS cannot run this code on the device (it is osd_block_kernel's
// epilogue: that kernel's range, and no other kernel), or null
static const char* osd_cs_refusal(const qldpc_code* code) {
  if (code->m > 512 || code->n > 1087) return "m <= 512 and n <= 1087 (the block kernel's range)";
  if (code->zero_col) return "an H without all-zero columns";
  if (opt(&Options::osd_column) != 0 || opt(&Options::osd_hbm) != 0) return "options osd_column and osd_hbm off";
  return nullptr;
}

// cs_lambda < 0: the reference's OSD of `order`; else OSD-CS (order unused)
static int osd_device_impl(const qldpc_code* code, int64_t count, const uint8_t* d_syn, const int32_t* d_perm,
                           const int32_t* d_tiepos, const double* d_post, int order, int cs_lambda,
                           uint8_t* d_ehat, int32_t* d_status, void* stream, const SpillCfg& spill = {}) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  const bool cs = cs_lambda >= 0;
  if (cs_lambda > QLDPC_OSD_CS_MAX_LAMBDA)
    return fail(QLDPC_EINVAL, "OSD-CS lambda must lie in 0..%d (got %d)", QLDPC_OSD_CS_MAX_LAMBDA, cs_lambda);
  if (cs) {
    order = 0;                                       // the base estimate, and the redo pass's semantics
    if (const char* why = osd_cs_refusal(code)) return fail(QLDPC_EUNSUP, "OSD-CS on the device needs %s", why);
  }
  if (count < 0) return fail(QLDPC_EINVAL, "negative count");
  if (count == 0) return QLDPC_OK;
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  if (!d_syn || !d_perm || !d_ehat || !d_status) return fail(QLDPC_EINVAL, "null device buffer");
  const int m = code->m, n = code->n;
  hipStream_t st = (hipStream_t)stream;
  qldpc::OsdArgs a = osd_args(code, d_syn, d_perm, d_tiepos, d_post, order, d_ehat, d_status, spill);
  a.cs_lambda = cs ? cs_lambda : 0;
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const int nw = qldpc::osd_nw_of((n + 1 + 63) / 64);
  const void* kcol = qldpc::select_osd_kernel(nw);
  // past the register / LDS kernels (m > 1024 rows, n > 2111 columns), or
  // option osd_hbm: the working matrix in global memory (osd_hbm_kernel)
  if (m > 1024 || !kcol || opt(&Options::osd_hbm) != 0) return osd_hbm_impl(code, a, count, max_lds, st);
  // The block kernel picks pivot rows by row index instead of REF's row
  // order: same J, same e_J (the unique solution), except when column 0 of
  // H[:, perm] has no pivot (an all-zero column of H: column kernel for the
  // whole code) or the syndrome lies outside H's column space (the block
  // kernel marks those shots, a second column-kernel pass redoes them).
  // option osd_column: the column kernel alone (A/B reference, tests).
  const bool column = opt(&Options::osd_column) != 0 || code->zero_col;
  int rt = 1;                                        // block kernel: rows per thread
  const void* kblk = column ? nullptr : qldpc::select_osd_block_kernel(nw, m, &rt, cs);
  const int block = std::max(64, (m + 63) / 64 * 64);
  const int bblk = std::max(64, ((m + rt - 1) / rt + 63) / 64 * 64);   // block kernel threads
  const int mr = rt * bblk;                          // its row slots
  const int base = align16(4 * n + 4 * (m + 2) + n) + (order == 1 ? 4 * setdiff_table_ints(n) : 0);
  const int lds_col = base + 8 * nw * (1 + 2 * 16 + 2) + 4 * 32 + 16;         // emask, candidate / xrow rows, slots, misc
  const int lds_blk = base + 8 * nw * (1 + 64 + (QLDPC_OSD_PAIRS ? 32 : 0)) + 8 * 64 + 8 * 2 * mr + 4 * 3 * mr + 4 * 64 + 64;
                      // emask, PW, PX, CT, Wd / Cm, pkof / pidx / crow, pk, misc
  if (lds_col > max_lds) return fail(QLDPC_EUNSUP, "GPU OSD needs %d B LDS", lds_col);
  HIP_TRY(hipFuncSetAttribute(kcol, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
  if (kblk && lds_blk > max_lds) kblk = nullptr;
  // OSD-CS has the block kernel alone, and works in its block-loop LDS (Wd .. CT)
  const size_t cs_room = (size_t)(16 * mr + 8 * nw * (64 + (QLDPC_OSD_PAIRS ? 32 : 0)) + 512);
  if (cs && (!kblk || qldpc::osd_cs_lds(nw, mr) > cs_room))
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
      e = hipLaunchKernel(kblk, dim3(g), dim3(bblk), params, (size_t)lds_blk, st);
      ai.redo = 1;                                    // same stream: runs after the block pass
    }
    if (e == hipSuccess) e = hipLaunchKernel(kcol, dim3(g), dim3(block), params, (size_t)lds_col, st);
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
                            int64_t spill_cap, void* stream) {
  if (d_spill_count && (!d_spill_post || !d_spill_idx || spill_cap < 0))
    return fail(QLDPC_EINVAL, "spill buffers incomplete");
  if (d_spill_count && count > INT32_MAX) return fail(QLDPC_EINVAL, "spill indices are int32");
  if (cs_lambda >= 0 && code)                        // (refused before the order kernel's launch too)
    if (const char* why = osd_cs_refusal(code)) return fail(QLDPC_EUNSUP, "OSD-CS on the device needs %s", why);
  const int rc = qldpc_osd_order_device(code, count, d_post, d_perm, d_tiepos, stream);
  if (rc != QLDPC_OK) return rc;
  return osd_device_impl(code, count, d_syn, d_perm, d_tiepos, d_post, order, cs_lambda, d_ehat, d_status, stream,
                         SpillCfg{d_spill_post, d_spill_idx, d_spill_count, spill_cap});
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

// The block kernel's instance as select_osd_block_kernel picks it (NW row
// words, SL engine slots, RT rows per thread), or the kernel that runs instead
extern "C" int qldpc_osd_kernel_name(const qldpc_code* code, int cs, char* buf, int len) {
  if (!code || !buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  const int m = code->m, n = code->n, nw = qldpc::osd_nw_of((n + 1 + 63) / 64);
  int rt = 1;
  const bool hbm = m > 1024 || !nw || opt(&Options::osd_hbm) != 0;
  const bool column = opt(&Options::osd_column) != 0 || code->zero_col;
  if (cs && osd_cs_refusal(code)) return fail(QLDPC_EUNSUP, "OSD-CS on the device needs %s", osd_cs_refusal(code));
  if (hbm) snprintf(buf, len, "osd_hbm_kernel");
  else if (column || !qldpc::select_osd_block_kernel(nw, m, &rt, cs != 0)) snprintf(buf, len, "osd_kernel<%d>", nw);
  else snprintf(buf, len, "osd_block%s_kernel<%d, %d, %d>", cs ? "_cs" : "", nw, rt == 1 ? 4 : 8, rt);
  return QLDPC_OK;
}
