// vprior_host_check.cpp — the host side of the per-variable-prior and channel
// handles under a sanitizer, without a device and without Python: create /
// destroy, threshold-table formation and every validation path that returns
// before a HIP call. Built from the library's own translation units (the
// Makefile's SRC and the <unit>_kernels.hip of its UNITS; the kernel headers
// wave_common.h ... bp_team.h come in through them), e.g.
//   cd qldpcsim_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined ../../tools/probe/vprior_host_check.cpp \
//     decoder_kernels.hip bp_team_kernels.hip ms_flood_kernels.hip decode_prior_kernels.hip \
//     decode_vprior_kernels.hip relay_kernels.hip osd_kernels.hip channel_kernels.hip hbm_kernels.hip \
//     hard_kernels.hip capi*.cpp np_order.cpp -o vprior_host_check && ./vprior_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/qldpc_decoder.h"

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, qldpc_last_error()); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

int main() {
  // the Steane code's H (7 columns), and a second code of the same shape
  const uint8_t H[3 * 7] = {0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1};
  const uint8_t G[3 * 7] = {1, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0};
  qldpc_code *code = nullptr, *other = nullptr;
  CHECK(qldpc_code_create(H, 3, 7, &code) == QLDPC_OK);
  CHECK(qldpc_code_create(G, 3, 7, &other) == QLDPC_OK);
  const int32_t lp[2] = {0, 3}, rows[3] = {0, 1, 2};
  qldpc_schedule* sched = nullptr;
  CHECK(qldpc_schedule_create(code, 1, lp, rows, &sched) == QLDPC_OK);

  std::vector<double> p(7, 0.01);
  p[1] = 0.0, p[2] = 0.5, p[3] = 0.9;
  qldpc_prior *pr = nullptr, *foreign = nullptr;
  CHECK(qldpc_prior_create(code, p.data(), 1e-9, &pr) == QLDPC_OK && pr);
  CHECK(qldpc_prior_create(other, p.data(), 1e-9, &foreign) == QLDPC_OK && foreign);
  for (double bad : {-1e-9, 1.0, 2.0, (double)NAN, (double)INFINITY}) {
    std::vector<double> q(p);
    q[6] = bad;
    qldpc_prior* x = nullptr;
    CHECK(qldpc_prior_create(code, q.data(), 1e-9, &x) == QLDPC_EINVAL && !x);
  }
  qldpc_prior* x = nullptr;
  CHECK(qldpc_prior_create(code, p.data(), 0.0, &x) == QLDPC_EINVAL);       // p = 0, eps = 0: no finite prior
  CHECK(qldpc_prior_create(code, nullptr, 1e-9, &x) == QLDPC_EINVAL);
  CHECK(qldpc_prior_create(nullptr, p.data(), 1e-9, &x) == QLDPC_EINVAL);
  CHECK(qldpc_prior_create(code, p.data(), 1e-9, nullptr) == QLDPC_EINVAL);

  uint8_t syn[2 * 3] = {0}, eh[2 * 7];
  int32_t it[2];
  CHECK(qldpc_decode_device_vprior(code, sched, QLDPC_ALGO_MS, syn, 0, 2, nullptr, 5, 0.75, eh, 0, it, nullptr,
                                   nullptr, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_decode_device_vprior(code, sched, QLDPC_ALGO_MS, syn, 0, 2, foreign, 5, 0.75, eh, 0, it, nullptr,
                                   nullptr, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_decode_device_vprior(code, sched, QLDPC_ALGO_NG, syn, 0, 2, pr, 5, 0.75, eh, 0, it, nullptr, nullptr,
                                   nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_decode_device_vprior(code, sched, QLDPC_ALGO_BP, syn, 0, 2, pr, 0, 0.75, eh, 0, it, nullptr, nullptr,
                                   nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_decode_device_vprior(code, sched, QLDPC_ALGO_BP, syn, 0, 0, pr, 5, 0.75, nullptr, 0, nullptr, nullptr,
                                   nullptr, nullptr) == QLDPC_OK);
  CHECK(qldpc_decode_host_vprior(code, sched, QLDPC_ALGO_MS, syn, 2, foreign, 5, 0.75, eh, it, nullptr, nullptr) ==
        QLDPC_EINVAL);
  CHECK(qldpc_decode_host_vprior(code, sched, QLDPC_ALGO_MS, nullptr, 0, pr, 5, 0.75, eh, it, nullptr, nullptr) ==
        QLDPC_OK);
  CHECK(qldpc_set_option("force_hbm", 1) == QLDPC_OK);
  CHECK(qldpc_decode_device_vprior(code, sched, QLDPC_ALGO_MS, syn, 0, 2, pr, 5, 0.75, eh, 0, it, nullptr, nullptr,
                                   nullptr) == QLDPC_EUNSUP);
  char name[64];
  CHECK(qldpc_decode_vprior_kernel_name(code, sched, QLDPC_ALGO_MS, name, 64) == QLDPC_EUNSUP);
  CHECK(qldpc_set_option("force_hbm", 0) == QLDPC_OK);
  CHECK(qldpc_decode_vprior_kernel_name(code, sched, QLDPC_ALGO_BP, name, 64) == QLDPC_OK);
  std::printf("%s\n", name);

  // threshold table: depolarizing triples equal the scalar thresholds
  for (double pp : {0.0, 1e-12, 0.1, 0.3, 0.7, 1.0}) {
    std::vector<double> q(7, pp / 3);
    std::vector<uint64_t> t(3 * 7);
    uint64_t t1, t2, t3;
    CHECK(qldpc_channel_table(q.data(), q.data(), q.data(), 7, t.data()) == QLDPC_OK);
    CHECK(qldpc_channel_thresholds(pp, &t1, &t2, &t3) == QLDPC_OK);
    for (int j = 0; j < 7; ++j) CHECK(t[j] == t1 && t[7 + j] == t2 && t[14 + j] == t3);
  }
  std::vector<double> a(7, 0.1), b(7, 0.1), c(7, 0.1);
  std::vector<uint64_t> t(3 * 7);
  c[6] = 0.81;
  CHECK(qldpc_channel_table(a.data(), b.data(), c.data(), 7, t.data()) == QLDPC_EINVAL);
  c[6] = NAN;
  CHECK(qldpc_channel_table(a.data(), b.data(), c.data(), 7, t.data()) == QLDPC_EINVAL);
  c[6] = 0.8;
  CHECK(qldpc_channel_table(a.data(), b.data(), c.data(), 7, t.data()) == QLDPC_OK);
  CHECK(qldpc_channel_table(a.data(), b.data(), c.data(), 0, nullptr) == QLDPC_OK);
  qldpc_channel* ch = nullptr;
  CHECK(qldpc_channel_create(code, other, a.data(), b.data(), c.data(), &ch) == QLDPC_OK && ch);
  qldpc_channel* bad = nullptr;
  a[0] = -0.1;
  CHECK(qldpc_channel_create(code, other, a.data(), b.data(), c.data(), &bad) == QLDPC_EINVAL && !bad);
  CHECK(qldpc_channel_create(code, other, nullptr, b.data(), c.data(), &bad) == QLDPC_EINVAL);
  uint64_t w[2];
  CHECK(qldpc_channel_sample_vec(nullptr, 1, 0, 2, w, w, syn, syn, 0, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_channel_sample_vec(ch, 1, 0, 2, w, w, syn, syn, 9, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_channel_sample_vec(ch, 1, 0, -1, w, w, syn, syn, 0, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_channel_sample_vec(ch, 1, 0, 2, nullptr, w, syn, syn, 0, nullptr) == QLDPC_EINVAL);
  CHECK(qldpc_channel_sample_vec(ch, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == QLDPC_OK);

  CHECK(qldpc_channel_destroy(ch) == QLDPC_OK && qldpc_channel_destroy(nullptr) == QLDPC_OK);
  CHECK(qldpc_prior_destroy(pr) == QLDPC_OK && qldpc_prior_destroy(foreign) == QLDPC_OK);
  CHECK(qldpc_prior_destroy(nullptr) == QLDPC_OK);
  CHECK(qldpc_schedule_destroy(sched) == QLDPC_OK);
  CHECK(qldpc_code_destroy(code) == QLDPC_OK && qldpc_code_destroy(other) == QLDPC_OK);
  std::puts("vprior_host_check OK");
  return 0;
}
