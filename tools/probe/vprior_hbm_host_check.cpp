// vprior_hbm_host_check.cpp — the host side of library option vprior_hbm under
// a sanitizer, without a device and without Python: the filter word formed
// with the prior handle, the routing of each refusal to hbm_tile_vprior_kernel
// (kernel names need no device) and every validation path of the decode entry
// points that returns before a HIP call, with the option off and on. Built as
// vprior_host_check.cpp is, from the library's own translation units; the
// kernel units hold no host code worth instrumenting, so they may be compiled
// once without the sanitizer and linked in (objects first on the line: behind
// a source file hipcc reads them as HIP text), e.g.
//   cd qldpcsim_amd/csrc && for f in *_kernels.hip; do hipcc --offload-arch=gfx950 -O1 -std=c++17 -fPIC \
//     -ffp-contract=off -c $f -o /tmp/$f.o; done && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -ffp-contract=off -Xarch_host -fsanitize=address,undefined /tmp/*_kernels.hip.o \
//     ../../tools/probe/vprior_hbm_host_check.cpp capi*.cpp np_order.cpp -o vprior_hbm_host_check && \
//     ./vprior_hbm_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../qldpcsim_amd/csrc/capi_internal.h"

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, qldpc_last_error()); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static qldpc_schedule* flooding(const qldpc_code* code, int m) {
  std::vector<int32_t> rows(m);
  for (int i = 0; i < m; ++i) rows[i] = i;
  const int32_t lp[2] = {0, m};
  qldpc_schedule* s = nullptr;
  CHECK(qldpc_schedule_create(code, 1, lp, rows.data(), &s) == QLDPC_OK);
  return s;
}

static void name_is(const qldpc_code* c, const qldpc_schedule* s, int algo, int rc, const char* want) {
  char name[64] = "";
  CHECK(qldpc_decode_vprior_kernel_name(c, s, algo, name, 64) == rc);
  if (rc == QLDPC_OK) CHECK(std::strcmp(name, want) == 0);
}

int main() {
  const uint8_t H[3 * 7] = {0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1};
  qldpc_code* code = nullptr;
  CHECK(qldpc_code_create(H, 3, 7, &code) == QLDPC_OK);
  qldpc_schedule* sched = flooding(code, 3);

  // the filter word: the XOR of avar over the variables with a negative prior,
  // in relabeled order, for none, one, several and all of them
  std::vector<double> p(7, 0.01);
  qldpc_prior* pr = nullptr;
  CHECK(qldpc_prior_create(code, p.data(), 1e-9, &pr) == QLDPC_OK);
  CHECK(pr->filt0 == 0);
  CHECK(qldpc_prior_destroy(pr) == QLDPC_OK);
  for (int mask = 1; mask < 128; mask += (mask < 8 ? 1 : 17)) {
    uint32_t want = 0;
    for (int j = 0; j < 7; ++j) {
      p[j] = ((mask >> j) & 1) ? 0.5 + 0.05 * (j + 1) : (j == 3 ? 0.5 : 0.02 * j);   // (0.5 and 0: not negative)
      if ((mask >> j) & 1) want ^= code->avar[code->vinv[j]];
    }
    CHECK(qldpc_prior_create(code, p.data(), 1e-9, &pr) == QLDPC_OK);
    CHECK(pr->filt0 == want && pr->filt0 == capi::prior_filter_word(code, pr->L));
    CHECK(qldpc_prior_destroy(pr) == QLDPC_OK);
  }
  std::fill(p.begin(), p.end(), 0.9);
  CHECK(qldpc_prior_create(code, p.data(), 1e-9, &pr) == QLDPC_OK);
  CHECK(pr->filt0 == code->filt_all);                 // every prior negative: the scalar kernel's word
  std::vector<double> none;
  CHECK(capi::prior_filter_word(code, none) == 0);    // (a shorter row reads no further)

  // routing, option off: as before
  uint8_t syn[2 * 3] = {0}, eh[2 * 7];
  int32_t it[2];
  auto dev = [&](const qldpc_code* c, const qldpc_schedule* s, int algo, int64_t batch, int mi) {
    return qldpc_decode_device_vprior(c, s, algo, syn, 0, batch, pr, mi, 0.75, eh, 0, it, nullptr, nullptr, nullptr);
  };
  auto host = [&](const qldpc_code* c, const qldpc_schedule* s, int algo, int64_t batch, int mi) {
    return qldpc_decode_host_vprior(c, s, algo, syn, batch, pr, mi, 0.75, eh, it, nullptr, nullptr);
  };
  int64_t v = -1;
  CHECK(qldpc_get_option("vprior_hbm", &v) == QLDPC_OK && v == 0);
  name_is(code, sched, QLDPC_ALGO_MS, QLDPC_OK, "decode_vprior_kernel<0, false, 0>");
  CHECK(qldpc_set_option("force_hbm", 1) == QLDPC_OK);
  name_is(code, sched, QLDPC_ALGO_MS, QLDPC_EUNSUP, "");
  CHECK(dev(code, sched, QLDPC_ALGO_MS, 2, 5) == QLDPC_EUNSUP && host(code, sched, QLDPC_ALGO_BP, 2, 5) == QLDPC_EUNSUP);

  // both options on: routed to the HBM instance; the argument checks stay
  CHECK(qldpc_set_option("vprior_hbm", 1) == QLDPC_OK);
  name_is(code, sched, QLDPC_ALGO_MS, QLDPC_OK, "hbm_tile_vprior_kernel<0, 8, 4>");
  name_is(code, sched, QLDPC_ALGO_BP, QLDPC_OK, "hbm_tile_vprior_kernel<1, 8, 4>");
  name_is(code, sched, QLDPC_ALGO_NG, QLDPC_EINVAL, "");
  name_is(code, nullptr, QLDPC_ALGO_MS, QLDPC_EINVAL, "");
  CHECK(dev(code, sched, QLDPC_ALGO_NG, 2, 5) == QLDPC_EINVAL && dev(code, sched, QLDPC_ALGO_MS, 2, 0) == QLDPC_EINVAL);
  CHECK(dev(code, sched, QLDPC_ALGO_MS, -1, 5) == QLDPC_EINVAL && dev(nullptr, sched, QLDPC_ALGO_MS, 2, 5) == QLDPC_EINVAL);
  CHECK(host(code, nullptr, QLDPC_ALGO_MS, 2, 5) == QLDPC_EINVAL && host(code, sched, QLDPC_ALGO_BF, 2, 5) == QLDPC_EINVAL);
  CHECK(dev(code, sched, QLDPC_ALGO_BP, 0, 5) == QLDPC_OK && host(code, sched, QLDPC_ALGO_MS, 0, 5) == QLDPC_OK);
  // no device here: past the validation a decode ends at the device check, not at a refusal
  if (qldpc_device_count() == 0)
    CHECK(dev(code, sched, QLDPC_ALGO_MS, 2, 5) == QLDPC_EHIP && host(code, sched, QLDPC_ALGO_BP, 2, 5) == QLDPC_EHIP);
  // the two-level twin has no HBM-resident variant
  char name[64];
  CHECK(qldpc_decode_prior_kernel_name(code, sched, QLDPC_ALGO_MS, name, 64) == QLDPC_EUNSUP);
  CHECK(qldpc_set_option("force_hbm", 0) == QLDPC_OK);
  if (qldpc_device_count() == 0) name_is(code, sched, QLDPC_ALGO_MS, QLDPC_OK, "decode_vprior_kernel<0, false, 0>");

  // past each device-free limit: the instance by row degree (8, 16, 32, 64)
  struct Case { int m, n, ones_per_row; int algo; const char* want; };
  const Case cases[] = {{1, 40, 40, QLDPC_ALGO_MS, "hbm_tile_vprior_kernel<0, 64, 4>"},
                        {1, 33, 33, QLDPC_ALGO_MS, "hbm_tile_vprior_kernel<0, 64, 4>"},
                        {1, 65536, 3, QLDPC_ALGO_MS, "hbm_tile_vprior_kernel<0, 8, 4>"},
                        {1, 65536, 9, QLDPC_ALGO_BP, "hbm_tile_vprior_kernel<1, 16, 4>"},
                        {130, 2, 2, QLDPC_ALGO_BP, "hbm_tile_vprior_kernel<1, 8, 4>"}};
  for (const Case& k : cases) {
    std::vector<uint8_t> M((size_t)k.m * k.n, 0);
    for (int r = 0; r < k.m; ++r)
      for (int j = 0; j < k.ones_per_row; ++j) M[(size_t)r * k.n + j] = 1;
    qldpc_code* c = nullptr;
    CHECK(qldpc_code_create(M.data(), k.m, k.n, &c) == QLDPC_OK);
    qldpc_schedule* s = flooding(c, k.m);
    name_is(c, s, k.algo, QLDPC_OK, k.want);
    CHECK(qldpc_set_option("vprior_hbm", 0) == QLDPC_OK);
    name_is(c, s, k.algo, QLDPC_EUNSUP, "");
    CHECK(qldpc_set_option("vprior_hbm", 1) == QLDPC_OK);
    std::vector<double> q(k.n, 0.01);
    q[0] = 0.8;
    qldpc_prior* x = nullptr;
    CHECK(qldpc_prior_create(c, q.data(), 1e-9, &x) == QLDPC_OK);
    CHECK(x->filt0 == c->avar[c->vinv[0]]);
    CHECK(qldpc_prior_destroy(x) == QLDPC_OK);
    CHECK(qldpc_schedule_destroy(s) == QLDPC_OK && qldpc_code_destroy(c) == QLDPC_OK);
  }
  CHECK(qldpc_set_option("vprior_hbm", 0) == QLDPC_OK);

  CHECK(qldpc_prior_destroy(pr) == QLDPC_OK);
  CHECK(qldpc_schedule_destroy(sched) == QLDPC_OK && qldpc_code_destroy(code) == QLDPC_OK);
  std::puts("vprior_hbm_host_check OK");
  return 0;
}
